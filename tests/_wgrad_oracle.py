"""fp64 oracle of the weight-gradient product dW[N][K] = dz[R][N]^T . x[R][K], shared by the
weight-gradient tests (CPU and GPU).

Method: dz and x are integers in [-2, 2] stored as bf16, so every product is an integer of
magnitude <= 4 and every partial sum over R <= 2^22 rows an integer below 2^24: exact in fp32
AND in fp64, in any summation order. Every split-K slab, every reduced gradient and every column
sum must then equal the fp64 reference bit for bit; there is no tolerance anywhere in this file
except the derived bound of :func:`random_ratio`.

Storage mirrors the engine: an operand is a micro-batch cut out of a larger buffer -- a row slice
of a taller, wider [rows_total][width + pad] buffer (row-major form, layouts MNMAJ / MNMAJ), or
a column slice of an [N][rows_total] buffer (K-major form ``dzt`` / ``xt``, layouts KMAJ /
KMAJ). Everything outside the slice is NaN. A kernel may read those neighbours (an edge tile
clamps its addresses, the register-prefetched loop restages past the end of its range); it may
never let one reach a result. Outputs are views into buffers filled with ``SENTINEL`` (1.5: no
integer, so an exact result never equals it and an unwritten element always shows), with a
leading dimension above the width, spare rows and one spare slab.

The device of the tensors decides between the HIP kernels and the CPU reference of the ops, as
in tests/_act_oracle.py and tests/_loss_oracle.py. Every checker takes the launch as a callable
(``run``), so tests/test_wgrad_oracle.py can hand it deliberately wrong implementations and see
them rejected.
"""
from __future__ import annotations

import torch

from docker_dist_nn_amd import ops
from docker_dist_nn_amd.ops import KMAJ, MNMAJ

PAD = 8        # elements of padding in front of / behind a view (16 bytes of bf16: aligned)
MB = 64        # rows (columns in the K-major form) of the neighbouring micro-batches
SENTINEL = 1.5
CPU = torch.device("cpu")
ROWS, COLS = "rows", "cols"  # operand forms: row slices (MNMAJ) / column slices (KMAJ)
FORMS = (ROWS, COLS)
NAN = float("nan")


# ---- shared case lists (run on the GPU by test_wgrad_forms_gpu.py and, through the CPU path of
# the same ops, by test_wgrad_oracle.py, which also checks that each case has the edge it names)

# (id, R, N, K, nwg, what streamk_geometry must say about it)
STREAMK_CASES = [
    ("128x64-straddle", 448, 128, 192, 5, dict(bm=128, bn=64, ipw=5, launched=5, straddle=True)),
    ("128x64-three-contributors", 448, 128, 192, 7, dict(ipw=3, launched=7, straddle=True)),
    ("128x128-straddle", 448, 128, 256, 3, dict(bm=128, bn=128, ipw=5, launched=3,
                                                straddle=True)),
    ("64x128-straddle", 448, 192, 128, 5, dict(bm=64, bn=128, ipw=5, launched=5, straddle=True)),
    ("64x64-straddle", 320, 192, 192, 13, dict(bm=64, bn=64, ipw=4, launched=12, straddle=True)),
    ("nwg-below-tiles", 448, 192, 192, 4, dict(tiles=9, ipw=7, launched=9, straddle=False)),
    ("nwg-above-iterations", 128, 128, 192, 100, dict(total=6, ipw=1, launched=6,
                                                      straddle=False)),
    ("one-step-per-tile", 64, 128, 192, 5, dict(ksteps=1, ipw=1, launched=3, straddle=False)),
]

# (N, K, R, accumulate) of the grouped launch: all planned on the 64x64 tile with workgroup
# counts 135, 21, 30 and 5 (none a multiple of 8: every item is followed by padding blocks), 3, 7,
# 10 and 5 splits; the first has 9 column tiles and 5 row tiles (grouped raster, tail group 1)
GROUP_SHAPES = [(320, 576, 448, False), (64, 192, 448, True), (192, 64, 640, False),
                (64, 64, 320, True)]


def group_problems(seed=0):
    """(case, S, accumulate) of GROUP_SHAPES, S = the planner's own split count (the grouped
    launch takes an item only with that count)."""
    return [(wgrad_case(R, N, K, seed + 31 * i), ops.plan("wgrad", N, K, R).splits, acc)
            for i, (N, K, R, acc) in enumerate(GROUP_SHAPES)]


# ---- cases ----------------------------------------------------------------------------------

def wgrad_case(R, N, K, seed, random=False):
    """dz[R][N], x[R][K] as bf16 (integers in [-2, 2]; ``random``: normal deviates rounded to
    bf16) with the fp64 product ``full`` = dz^T . x and ``absprod`` = |dz|^T . |x|."""
    assert R % 64 == 0 and N % 8 == 0 and K % 8 == 0
    g = torch.Generator().manual_seed(seed)
    if random:
        dz = torch.randn(R, N, generator=g).to(torch.bfloat16)
        x = torch.randn(R, K, generator=g).to(torch.bfloat16)
    else:
        dz = torch.randint(-2, 3, (R, N), generator=g).to(torch.bfloat16)
        x = torch.randint(-2, 3, (R, K), generator=g).to(torch.bfloat16)
    d64, x64 = dz.double(), x.double()
    return dict(R=R, N=N, K=K, dz=dz, x=x, full=d64.t() @ x64, absprod=d64.abs().t() @ x64.abs(),
                random=random)


def slab_range(s, S, R):
    """Rows of split s of S: the project's range rule (64-row steps, sizes differ by <= 1)."""
    ks = R // 64
    return (s * ks // S) * 64, ((s + 1) * ks // S) * 64


def slab_ref(case, s, S):
    a, b = slab_range(s, S, case["R"])
    return case["dz"][a:b].double().t() @ case["x"][a:b].double()


def slabs_ref(case, S):
    return torch.stack([slab_ref(case, s, S) for s in range(S)])


# ---- operand storage ------------------------------------------------------------------------

def _row_slice(t, dev):
    R, W = t.shape
    buf = torch.full((MB + R + MB, W + 3 * PAD), NAN, dtype=torch.bfloat16)
    buf[MB:MB + R, PAD:PAD + W] = t
    buf = buf.to(dev)
    return buf[MB:MB + R, PAD:PAD + W]


def _col_slice(t, dev):
    R, W = t.shape
    buf = torch.full((W + 2 * PAD, MB + R + MB + PAD), NAN, dtype=torch.bfloat16)
    buf[PAD:PAD + W, MB:MB + R] = t.t()
    buf = buf.to(dev)
    return buf[PAD:PAD + W, MB:MB + R]


def operands(case, form, dev):
    """(a, b, layout): dz and x of the case as the A and B operand of the product in ``form``,
    NaN all around (rows before and after, columns past the width; ld > width)."""
    if form == ROWS:
        return _row_slice(case["dz"], dev), _row_slice(case["x"], dev), MNMAJ
    assert form == COLS, form
    return _col_slice(case["dz"], dev), _col_slice(case["x"], dev), KMAJ


# ---- output storage -------------------------------------------------------------------------

def out_slabs(S, N, K, dev, dtype=torch.float32, prior=None):
    """(buffer, view): [S][N][K] at (0, PAD, PAD) of a sentinel-filled [S + 1][N + 2 PAD]
    [K + 3 PAD] buffer (ldc = K + 3 PAD > K, spare rows, one spare slab); ``prior`` [S][N][K]:
    the view's contents (what an accumulating launch adds to)."""
    buf = torch.full((S + 1, N + 2 * PAD, K + 3 * PAD), SENTINEL, dtype=dtype)
    if prior is not None:
        buf[:S, PAD:PAD + N, PAD:PAD + K] = prior.to(dtype)
    buf = buf.to(dev)
    return buf, buf[:S, PAD:PAD + N, PAD:PAD + K]


def assert_outside_untouched(buf, S, N, K, what=""):
    outside = torch.ones(buf.shape, dtype=torch.bool)
    outside[:S, PAD:PAD + N, PAD:PAD + K] = False
    b = buf.detach().to(CPU)
    bad = outside & (b != SENTINEL)
    assert not bool(bad.any()), (f"{what}: wrote outside [S][N][K] at "
                                 f"{bad.nonzero()[:4].tolist()} of {tuple(buf.shape)}")


def guarded(n, dev, guard=64):
    """(buffer, view): exactly ``n`` fp32 elements between two sentinel guards."""
    buf = torch.full((n + 2 * guard,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[guard:guard + n]


def assert_guard_intact(buf, n, what="", guard=64):
    b = buf.detach().to(CPU)
    assert bool((b[:guard] == SENTINEL).all()) and bool((b[guard + n:] == SENTINEL).all()), \
        f"{what}: wrote outside the {n}-element buffer"


def assert_exact(got, ref64, what=""):
    """Every element of ``got`` equals the fp64 reference bit for bit; no NaN."""
    got = got.detach().to(CPU).double()
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    assert not bool(torch.isnan(got).any()), \
        f"{what}: NaN in the result at {torch.isnan(got).nonzero()[:4].tolist()}"
    bad = got != ref64
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from "
                                 f"fp64, first at {bad.nonzero()[:4].tolist()}: got "
                                 f"{got[bad][:4].tolist()} want {ref64[bad][:4].tolist()}")


# ---- split-K --------------------------------------------------------------------------------

def gemm_wgrad(a, b, slabs, layout, N, K, R, S, accumulate=False, **launch):
    """ops.gemm called exactly as ops.linear_wgrad calls it."""
    ops.gemm(a, b, slabs, layout_a=layout, layout_b=layout, M=N, N=K, K=R, k_total=R,
             accumulate=accumulate, splits=S, **launch)


def linear_wgrad_run(case, dev):
    """A ``run`` that goes through ops.linear_wgrad itself (the planner's configuration)."""
    dz, x, _ = operands(case, ROWS, dev)

    def run(a, b, slabs, layout, N, K, R, S, accumulate=False):
        if layout == KMAJ:
            ops.linear_wgrad(dz, x, slabs, splits=S, accumulate=accumulate, dzt=a, xt=b)
        else:
            ops.linear_wgrad(a, b, slabs, splits=S, accumulate=accumulate)
    return run


def check_split_k(case, form, S, dev, run=gemm_wgrad, accumulate=True, what="", **launch):
    """Every slab on its own, then their sum, then (``accumulate``) a second accumulating pass
    giving exactly twice; nothing outside [S][N][K] written."""
    R, N, K = case["R"], case["N"], case["K"]
    what = f"{what} split-K {form} R={R} N={N} K={K} S={S} {launch}"
    a, b, layout = operands(case, form, dev)
    buf, slabs = out_slabs(S, N, K, dev)
    run(a, b, slabs, layout, N, K, R, S, **launch)
    want, got = slabs_ref(case, S), slabs.detach().to(CPU)
    for s in range(S):
        assert_exact(got[s], want[s], f"{what} slab {s} rows {slab_range(s, S, R)}")
    assert_exact(got.double().sum(0), case["full"], f"{what} sum of slabs")
    assert_outside_untouched(buf, S, N, K, what)
    if accumulate:
        run(a, b, slabs, layout, N, K, R, S, accumulate=True, **launch)
        assert_exact(slabs, 2.0 * want, f"{what} accumulate")
        assert_outside_untouched(buf, S, N, K, f"{what} accumulate")


# ---- raster walk ----------------------------------------------------------------------------

def raster_case(tiles_m, tiles_n, tiles, S, seed):
    """A product of tiles_m x tiles_n output tiles whose last tile is partial in both dimensions
    (24 rows, 40 columns of it) with one 64-row k-step per split."""
    bm, bn = tiles
    return wgrad_case(64 * S, (tiles_m - 1) * bm + 24, (tiles_n - 1) * bn + 40, seed)


def check_raster_bf16(case, form, dev, tiles, **launch):
    """One split into a bf16 output with bias, ReLU and colsum: the stored output is
    RN_bf16(relu(dz^T x + bias)) bit for bit (integers up to 260: one rounding above 256) and the
    per-row-tile column sums of the stored integers EQUAL their fp64 sums."""
    import _act_oracle as ao

    R, N, K = case["R"], case["N"], case["K"]
    what = f"raster bf16 {form} N={N} K={K} {tiles} {launch}"
    a, b, layout = operands(case, form, dev)
    g = torch.Generator().manual_seed(N + K)
    bias = torch.randint(-4, 5, (K,), generator=g).float()
    buf, out = out_slabs(1, N, K, dev, dtype=torch.bfloat16)
    n_part = -(-N // tiles[0])
    cs = torch.full((n_part + 1, K + PAD), SENTINEL, dtype=torch.float32, device=dev)
    ops.gemm(a, b, out[0], layout_a=layout, layout_b=layout, M=N, N=K, K=R, bias=bias.to(dev),
             act="relu", tiles=tiles, colsum=cs[:n_part], **launch)
    ao.assert_bf16_close(out[0], (case["full"] + bias.double()).clamp_min(0.0), 0, what)
    assert_outside_untouched(buf, 1, N, K, what)
    assert_exact(cs[:n_part, :K], ao.colsum_ref(out[0], tiles[0]), f"{what} colsum")
    c = cs.detach().to(CPU)
    assert bool((c[:, K:] == SENTINEL).all()) and bool((c[n_part:] == SENTINEL).all()), \
        f"{what}: colsum wrote outside [{n_part}][{K}]"


# ---- stream-K -------------------------------------------------------------------------------

def streamk_geometry(N, K, R, nwg):
    """The launch arithmetic of the stream-K kernel (csrc/kernels/gemm.hip gemm_bf16_streamk):
    tile, tiles, k-steps per tile, iterations per workgroup, launched workgroups, and whether
    some workgroup's share crosses a tile boundary (two segments)."""
    bm, bn = ops.streamk_tiles(N, K)
    tiles, ksteps = (N // bm) * (K // bn), R // 64
    total = tiles * ksteps
    nwg = max(nwg, tiles)
    ipw = -(-total // nwg)
    launched = -(-total // ipw)
    straddle = any(w * ipw // ksteps != (min(total, (w + 1) * ipw) - 1) // ksteps
                   for w in range(launched))
    return dict(bm=bm, bn=bn, tiles=tiles, tiles_n=K // bn, ksteps=ksteps, total=total, ipw=ipw,
                launched=launched, straddle=straddle)


def streamk_model(case, nwg, first_segment_always=False):
    """fp64 model of the two stream-K kernels: every workgroup's partial tiles per segment,
    then the reduce that picks segment 0 for the tile a workgroup started in and 1 for the
    next. ``first_segment_always``: the defect of a reduce that takes segment 0 everywhere."""
    N, K, R = case["N"], case["K"], case["R"]
    g = streamk_geometry(N, K, R, nwg)
    bm, bn, ksteps, ipw = g["bm"], g["bn"], g["ksteps"], g["ipw"]
    dz, x = case["dz"].double(), case["x"].double()
    part = {}
    for w in range(g["launched"]):
        it, end, seg = w * ipw, min(g["total"], (w + 1) * ipw), 0
        while it < end:
            tile, k0 = divmod(it, ksteps)
            k1 = min(ksteps, k0 + end - it)
            tm, tn = divmod(tile, g["tiles_n"])
            rows = slice(k0 * 64, k1 * 64)
            part[(w, seg)] = dz[rows, tm * bm:(tm + 1) * bm].t() @ x[rows, tn * bn:(tn + 1) * bn]
            it += k1 - k0
            seg += 1
    out = torch.zeros(N, K, dtype=torch.float64)
    for tile in range(g["tiles"]):
        tm, tn = divmod(tile, g["tiles_n"])
        first, last = tile * ksteps, tile * ksteps + ksteps - 1
        for w in range(first // ipw, last // ipw + 1):
            seg = 0 if (first_segment_always or w * ipw // ksteps == tile) else 1
            out[tm * bm:(tm + 1) * bm, tn * bn:(tn + 1) * bn] += part[(w, seg)]
    return out


def streamk_run(dz, x, grad, part, accumulate, nwg):
    ops.linear_wgrad_streamk(dz, x, grad, part, accumulate=accumulate, nwg=nwg)


def check_streamk(case, dev, nwg, run=streamk_run, what=""):
    """Exact result, exact doubling under accumulate, a bit-identical repeat; the scratch is
    exactly streamk_partial_elems long between guards that must stay intact."""
    R, N, K = case["R"], case["N"], case["K"]
    what = f"{what} stream-K R={R} N={N} K={K} nwg={nwg} {streamk_geometry(N, K, R, nwg)}"
    dz, x, _ = operands(case, ROWS, dev)
    n_part = ops.streamk_partial_elems(N, K, nwg)
    pbuf, part = guarded(n_part, dev)
    buf, grad = out_slabs(1, N, K, dev)
    run(dz, x, grad[0], part, False, nwg)
    assert_exact(grad[0], case["full"], what)
    assert_outside_untouched(buf, 1, N, K, what)
    assert_guard_intact(pbuf, n_part, what)
    first = grad[0].detach().to(CPU).clone()
    run(dz, x, grad[0], part, True, nwg)
    assert_exact(grad[0], 2.0 * case["full"], f"{what} accumulate")
    buf2, grad2 = out_slabs(1, N, K, dev)
    run(dz, x, grad2[0], part, False, nwg)
    assert torch.equal(grad2[0].detach().to(CPU), first), f"{what}: repeat run differs"
    assert_outside_untouched(buf2, 1, N, K, f"{what} repeat")
    assert_guard_intact(pbuf, n_part, f"{what} repeat")


# ---- grouped launch -------------------------------------------------------------------------

def group_run(items):
    """ops.linear_wgrad_group; what it returns (did not launch) runs through ops.linear_wgrad,
    as the engine does. Returns the indices it did not launch."""
    rest = ops.linear_wgrad_group(items)
    for i in rest:
        dz, x, slabs, S, acc = items[i]
        ops.linear_wgrad(dz, x, slabs, splits=S, accumulate=acc)
    return rest


def check_group(problems, dev, run=group_run, must_launch=None, what=""):
    """``problems``: (case, S, accumulate). One grouped call over all of them; every slab exact
    (an accumulating item adds to integer contents), nothing outside written. ``must_launch``
    (default: on the GPU) asserts that the grouped launch took every item."""
    if must_launch is None:
        must_launch = dev.type != "cpu"
    items, outs = [], []
    for i, (case, S, acc) in enumerate(problems):
        R, N, K = case["R"], case["N"], case["K"]
        dz, x, _ = operands(case, ROWS, dev)
        g = torch.Generator().manual_seed(1000 + i)
        prior = torch.randint(-8, 9, (S, N, K), generator=g).double() if acc else None
        buf, slabs = out_slabs(S, N, K, dev, prior=prior)
        items.append((dz, x, slabs, S, acc))
        outs.append((buf, slabs, prior))
    rest = run(items)
    if must_launch:
        assert rest == [], f"{what}: the grouped launch left out items {rest}"
    for i, ((case, S, acc), (buf, slabs, prior)) in enumerate(zip(problems, outs)):
        w = f"{what} group item {i} R={case['R']} N={case['N']} K={case['K']} S={S} acc={acc}"
        want = slabs_ref(case, S) + (prior if acc else 0.0)
        for s in range(S):
            assert_exact(slabs[s], want[s], f"{w} slab {s}")
        assert_outside_untouched(buf, S, case["N"], case["K"], w)
    return rest


# ---- reductions -----------------------------------------------------------------------------

def reduce_case(n_src, n, seed, accumulate):
    """Integer slabs [n_src][n] in [-4, 4] inside a [n_src][n + PAD] source whose gaps are NaN,
    and integer contents of the output."""
    g = torch.Generator().manual_seed(seed)
    src = torch.full((n_src, n + PAD), NAN, dtype=torch.float32)
    src[:, :n] = torch.randint(-4, 5, (n_src, n), generator=g).float()
    prior = torch.randint(-64, 65, (n,), generator=g).float()
    return dict(n_src=n_src, n=n, stride=n + PAD, src=src, prior=prior, accumulate=accumulate)


def reduce_ref(rc, scale):
    want = scale * rc["src"][:, :rc["n"]].double().sum(0)
    return want + rc["prior"].double() if rc["accumulate"] else want


def _reduce_out(rc, dev):
    out = torch.full((rc["n"] + PAD,), SENTINEL, dtype=torch.float32)
    out[:rc["n"]] = rc["prior"]
    return out.to(dev)


def _assert_reduced(out, rc, scale, what):
    assert_exact(out[:rc["n"]], reduce_ref(rc, scale), what)
    assert bool((out[rc["n"]:].detach().to(CPU) == SENTINEL).all()), f"{what}: wrote past n"


def check_reduce_slabs(rc, scale, dev, run=ops.reduce_slabs):
    """out[:n] (+)= scale * sum of the sources, exact for a power-of-two scale."""
    out = _reduce_out(rc, dev)
    run(rc["src"].to(dev), rc["n_src"], rc["stride"], rc["n"], out, scale=scale,
        accumulate=rc["accumulate"])
    _assert_reduced(out, rc, scale,
                    f"reduce_slabs n_src={rc['n_src']} n={rc['n']} scale={scale} "
                    f"acc={rc['accumulate']}")


def check_reduce_multi(rcs, scales, dev, max_blocks=0, run=ops.reduce_multi):
    outs = [_reduce_out(rc, dev) for rc in rcs]
    jobs = [(rc["src"].to(dev), rc["n_src"], rc["stride"], rc["n"], out, scale, rc["accumulate"])
            for rc, out, scale in zip(rcs, outs, scales)]
    run(jobs, max_blocks=max_blocks)
    for rc, out, scale in zip(rcs, outs, scales):
        _assert_reduced(out, rc, scale, f"reduce_multi max_blocks={max_blocks} "
                                        f"n_src={rc['n_src']} n={rc['n']} scale={scale}")


def check_chain(case, form, S, scale, dev):
    """ops.linear_wgrad slabs -> ops.reduce_slabs -> the final gradient = scale * dz^T x in
    fp64 (contiguous slabs, as the engine's: the reduce reads them flat)."""
    R, N, K = case["R"], case["N"], case["K"]
    a, b, layout = operands(case, form, dev)
    slabs = torch.full((S, N, K), SENTINEL, dtype=torch.float32, device=dev)
    linear_wgrad_run(case, dev)(a, b, slabs, layout, N, K, R, S)
    gbuf, grad = guarded(N * K, dev)
    ops.reduce_slabs(slabs, S, N * K, N * K, grad, scale=scale)
    assert_exact(grad.view(N, K), scale * case["full"], f"chain R={R} N={N} K={K} S={S}")
    assert_guard_intact(gbuf, N * K, "chain")


# ---- random operands ------------------------------------------------------------------------

def random_bound(case, S):
    """Worst case of any summation order with round-to-nearest fp32 additions. The bf16 x bf16
    products are exact in fp32 (8 + 8 significand bits); an element is the sum of R of them in
    S partial sums that are then added, R + S - 1 < R + S additions in all, each with a relative
    error of at most 2^-24 of a partial sum that never exceeds sum |dz| |x|: the first-order
    bound (R + S) * 2^-24 * (|dz|^T |x|) (Higham, Accuracy and Stability, section 4.2; the
    second-order term is (R + S) * 2^-24 < 1e-4 of it)."""
    return (case["R"] + S) * 2.0 ** -24 * case["absprod"]


def random_ratio(got, case, S, what=""):
    """max |got - fp64| / bound over the elements; asserts no NaN. The caller asserts <= 1."""
    got = got.detach().to(CPU).double()
    assert not bool(torch.isnan(got).any()), f"{what}: NaN in the result"
    return float(((got - case["full"]).abs() / random_bound(case, S)).max())


def reduced_gradient(case, form, S, dev, run=gemm_wgrad, **launch):
    """The fp32 gradient of the case: split-K slabs (views into sentinel storage, NaN-padded
    operands) summed by ops.reduce_slabs from a contiguous copy."""
    R, N, K = case["R"], case["N"], case["K"]
    a, b, layout = operands(case, form, dev)
    buf, slabs = out_slabs(S, N, K, dev)
    run(a, b, slabs, layout, N, K, R, S, **launch)
    assert_outside_untouched(buf, S, N, K, f"random {form} {launch}")
    flat = slabs.contiguous()
    grad = torch.empty(N * K, dtype=torch.float32, device=dev)
    ops.reduce_slabs(flat, S, N * K, N * K, grad)
    return grad.view(N, K)
