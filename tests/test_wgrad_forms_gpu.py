"""Every form of the weight gradient dW[N][K] = dz[R][N]^T . x[R][K] and the grouped raster walk
against the exact fp64 oracle of tests/_wgrad_oracle.py.

Integer operands in [-2, 2] make every product and partial sum exact, so every split-K slab,
every reduced gradient and every column sum must equal fp64 bit for bit. Operands are
micro-batch slices of NaN-filled buffers (row slices: layouts MNMAJ / MNMAJ; column slices of
[N][rows_total]: KMAJ / KMAJ), outputs views into sentinel-filled buffers.

What each test pins is in its parameter ids:
* ``test_split_k_forms`` -- tile x main-loop form x operand form; S = 1, 3 (uneven 2 / 2 / 3
  steps) and 7 (ONE k-step per split: shorter than every pipeline, the register-prefetched loop
  restages past the end from its prologue on);
* ``test_table_configuration`` -- each distinct (tile, splits, stages, persist) the shipped
  table runs a wgrad on, ranges of one or two k-steps;
* ``test_raster_walk`` -- each launch path with 8 / 9 column tiles (the grouped walk switches
  itself on at 8) and 5 / 6 row tiles (tail groups of 1 / 2 under group_m = 4);
* ``test_streamk`` -- shares that straddle a tile boundary, and the degenerate share sizes;
* ``test_group_*`` -- the grouped launch with padding blocks between its items.
"""
import json

import pytest
import torch

import _wgrad_oracle as wo
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.ops import MNMAJ, tuning
from test_activation_epilogues_gpu import FORMS as ACT_FORMS, TILES

pytestmark = pytest.mark.gpu

FOUR_WAVE = [(128, 128), (128, 64), (64, 128), (64, 64)]
# every (tile, form) of the activation tests, stages 3 and 4 where the LDS holds them (4-wave
# tiles), a persistent launch of 3 workgroups (each walks several tiles and splits), ping-pong
SPLIT_FORMS = (ACT_FORMS + [(t, dict(stages=3)) for t in FOUR_WAVE] +
               [(t, dict(stages=4)) for t in FOUR_WAVE] + [(t, dict(persist=3)) for t in TILES] +
               [((256, 256), dict(stages=8))])
# what gemm_bf16 does not build (gemm_error_string -12)
REJECTED = [((256, 256), dict(stages=3)),              # 3 stages of 256x256 exceed the LDS
            ((256, 128), dict(stages=4)),              # 8-wave tiles: 2, 3 or 5
            ((128, 256), dict(stages=9)),              # no register-prefetched 128x256
            ((64, 128), dict(stages=6)),               # ... nor 64x128
            ((128, 64), dict(stages=11)),              # ring-direct: 256x256, 256x128, 128x128
            ((128, 128), dict(stages=8)),              # ping-pong is the 256x256 tile only
            ((128, 128), dict(stages=5, persist=-1)),  # the A3/B2 ring is a one-tile form
            ((128, 128), dict(stages=4, persist=-1)),  # persistent rings are 2 or 3 deep
            ((128, 128), dict(stages=9, persist=-1))]  # the prefetched loop is a one-tile form


def _fid(tiles, form):
    return f"{tiles[0]}x{tiles[1]}-" + "-".join(f"{k}{v}" for k, v in form.items())


def _seed(*parts):
    return sum((i + 1) * 7919 * int(p) for i, p in enumerate(parts)) % (2 ** 31)


R7 = 64 * 7
_CASES = {}


def _case(R, N, K, random=False):
    """One case per shape for the whole module (the fp64 reference is computed once)."""
    key = (R, N, K, random)
    if key not in _CASES:
        _CASES[key] = wo.wgrad_case(R, N, K, _seed(R, N, K), random=random)
    return _CASES[key]


# ---- 3. split-K forms -----------------------------------------------------------------------

@pytest.mark.parametrize("form", wo.FORMS)
@pytest.mark.parametrize("tiles,launch", SPLIT_FORMS, ids=[_fid(t, f) for t, f in SPLIT_FORMS])
def test_split_k_forms(dev, tiles, launch, form):
    """N = bm + 64, K = bn + 64: a full and a partial tile each way wherever the tile exceeds
    64. Every slab exact, their sum exact, an accumulating pass exactly twice."""
    bm, bn = tiles
    case = _case(R7, bm + 64, bn + 64)
    for S in (1, 3, 7):
        wo.check_split_k(case, form, S, dev, tiles=tiles, **launch)


@pytest.mark.parametrize("form", wo.FORMS)
@pytest.mark.parametrize("tiles,launch", REJECTED, ids=[_fid(t, f) for t, f in REJECTED])
def test_unsupported_forms_are_rejected(dev, tiles, launch, form):
    """The launcher's rule (csrc/kernels/gemm.hip gemm_bf16): stage codes 2..5 on 4-wave tiles,
    2 / 3 / 5 on 8-wave tiles (256x256: 2 / 5 / 8); the register-prefetched codes 6 / 9 on
    256x256, 256x128, 128x128, 128x64 and 64x64, 11 on the first three; a persistent launch only
    with a 2- or 3-deep plain ring. Anything else raises -- it does not run another kernel --
    and writes nothing."""
    bm, bn = tiles
    case = _case(R7, bm + 64, bn + 64)
    a, b, layout = wo.operands(case, form, dev)
    buf, slabs = wo.out_slabs(3, case["N"], case["K"], dev)
    with pytest.raises(ValueError):
        wo.gemm_wgrad(a, b, slabs, layout, case["N"], case["K"], R7, 3, tiles=tiles, **launch)
    torch.cuda.synchronize()
    assert bool((buf == wo.SENTINEL).all())


@pytest.mark.parametrize("form", wo.FORMS)
@pytest.mark.parametrize("N,K", [(128, 192), (512, 832)])
def test_linear_wgrad_planned(dev, form, N, K):
    """ops.linear_wgrad itself, the planner's tile / stage code / persist through launch_args:
    a shape outside the table and one whose signature family is in it."""
    case = _case(R7, N, K)
    for S in (1, 3, 7):
        wo.check_split_k(case, form, S, dev, run=wo.linear_wgrad_run(case, dev))


# ---- 4. the shipped table's wgrad configurations --------------------------------------------

def _table_configs():
    with open(tuning.DEFAULT_PATH) as f:
        entries = json.load(f)["entries"]
    return sorted({(tuple(e["tile"]), int(e["splits"]), int(e.get("stages", 0)),
                    int(e.get("persist", 0)))
                   for k, e in entries.items() if k.startswith("wgrad:")})


TABLE = _table_configs()


def test_table_has_wgrad_configurations():
    assert len(TABLE) >= 12 and {c[1] for c in TABLE} >= {1, 256}


@pytest.mark.parametrize("form", wo.FORMS)
@pytest.mark.parametrize("tiles,S,stages,persist", TABLE,
                         ids=[f"{t[0]}x{t[1]}-S{s}-stages{st}-persist{p}"
                              for t, s, st, p in TABLE])
def test_table_configuration(dev, tiles, S, stages, persist, form):
    """R = 64 * (S + S // 2 + 1): the ranges hold one or two k-steps each."""
    bm, bn = tiles
    R = 64 * (S + S // 2 + 1)
    steps = {(b - a) // 64 for a, b in (wo.slab_range(s, S, R) for s in range(S))}
    assert steps <= {1, 2}
    case = _case(R, bm + 64, bn + 64)
    wo.check_split_k(case, form, S, dev, tiles=tiles, stages=stages,
                     persist=-1 if persist == 1 else persist)  # gemm_plan._persist


# ---- 5. raster walk -------------------------------------------------------------------------

PATHS = [("classic-stages2", (64, 64), dict(stages=2)),
         ("rp-stages9", (64, 64), dict(stages=9)),
         ("ring-direct-stages11", (128, 128), dict(stages=11)),
         ("pingpong-stages8", (256, 256), dict(stages=8)),
         ("persist-round", (64, 64), dict(persist=-1)),
         ("persist-3wg", (64, 64), dict(persist=3))]


@pytest.mark.parametrize("tiles_m,tiles_n", [(5, 8), (5, 9), (6, 8), (6, 9)],
                         ids=lambda v: f"tiles{v}")  # ids: ...-tiles<rows>-tiles<columns>
@pytest.mark.parametrize("name,tiles,launch", PATHS, ids=[p[0] for p in PATHS])
def test_raster_walk(dev, name, tiles, launch, tiles_m, tiles_n):
    """Each launch path's copy of the grouped walk: group_m = 0 (the default, 4 from 8 column
    tiles on: tail groups of 1 / 2 row tiles), 3 (odd: a tail group of 2 at 5 row tiles) and 16
    (more than the row tiles: one group); one and two splits of one k-step; last tile partial
    both ways.
    A tile visited twice, one never, or a swapped pair shows as an inexact or unwritten
    element."""
    for S in (1, 2):
        case = wo.raster_case(tiles_m, tiles_n, tiles, S, _seed(tiles_m, tiles_n, S))
        for group_m in (0, 3, 16):
            wo.check_split_k(case, wo.ROWS, S, dev, accumulate=False, tiles=tiles,
                             group_m=group_m, **launch)
        wo.check_split_k(case, wo.COLS, S, dev, accumulate=False, tiles=tiles, **launch)
        if S == 1:
            for group_m in (0, 3):
                wo.check_raster_bf16(case, wo.ROWS, dev, tiles, group_m=group_m, **launch)


def _native_group(layout, tiles=(64, 64)):
    """The grouped kernel launched directly (any shape: edge tiles, any split count)."""
    def rows(a):
        return a.shape[0] if layout == MNMAJ else a.shape[1]

    def run(items):
        probs = [(ops.kernels._p(a), a.stride(0), ops.kernels._p(b), b.stride(0),
                  ops.kernels._p(sl), sl.stride(1), sl.stride(0), sl.shape[1], sl.shape[2],
                  rows(a), rows(a), int(acc), S) for (a, b, sl, S, acc) in items]
        ops.kernels.native().gemm_bf16_group(probs, layout, layout, 1, tiles[0], tiles[1], 2,
                                             torch.cuda.current_stream().cuda_stream)
        return []
    return run


@pytest.mark.parametrize("tiles_m", [5, 6], ids=lambda v: f"tiles_m{v}")
def test_group_raster_walk(dev, tiles_m):
    """gemm_group_kernel's copy of the walk: 9 column tiles, last tile partial both ways, two
    splits, beside a second item, with padding blocks after both (workgroup counts 90 / 108 and 9:
    no multiples of 8)."""
    probs = [(wo.raster_case(tiles_m, 9, (64, 64), 2, _seed(tiles_m, 9)), 2, False),
             (_case(64 * 3, 64, 128 + 40), 3, True)]
    assert all((-(-c["N"] // 64) * -(-c["K"] // 64) * S) % 8 for c, S, _ in probs)
    wo.check_group(probs, dev, run=_native_group(MNMAJ))


# ---- 6. grouped launch and stream-K ---------------------------------------------------------

def test_group_op(dev):
    """ops.linear_wgrad_group over four items of different shapes, split counts (3, 7, 10, 5)
    and accumulate flags, each followed by padding blocks; the op launched all of them."""
    rest = wo.check_group(wo.group_problems(), dev)
    assert rest == []


@pytest.mark.parametrize("cid,R,N,K,nwg,expect", wo.STREAMK_CASES,
                         ids=[c[0] for c in wo.STREAMK_CASES])
def test_streamk(dev, cid, R, N, K, nwg, expect):
    g = wo.streamk_geometry(N, K, R, nwg)
    assert {k: g[k] for k in expect} == expect
    wo.check_streamk(_case(R, N, K), dev, nwg)


# ---- 7. reductions and the random bound -----------------------------------------------------

@pytest.mark.parametrize("n_src", [1, 3, 8, 17, 40, 64, 128, 300])  # every source-group class
def test_reduce_slabs_exact(dev, n_src):
    for acc in (False, True):
        wo.check_reduce_slabs(wo.reduce_case(n_src, 4096 + 64, n_src, acc), 0.25, dev)


@pytest.mark.parametrize("max_blocks", [0, 7, 128])
def test_reduce_multi_exact(dev, max_blocks):
    classes = [1, 3, 8, 17, 40, 64, 128, 300]
    rcs = [wo.reduce_case(n_src, n, n_src + n, bool(k % 2))
           for k, (n_src, n) in enumerate(zip(classes, [64, 4096, 832 * 64, 256, 128, 1024,
                                                        2048 + 64, 4096]))]
    wo.check_reduce_multi(rcs, [2.0 ** (k % 5 - 3) for k in range(len(rcs))], dev,
                          max_blocks=max_blocks)


@pytest.mark.parametrize("form", wo.FORMS)
@pytest.mark.parametrize("N,K,S", [(128, 192, 7), (512, 832, 3)])
def test_chain_wgrad_reduce(dev, form, N, K, S):
    """ops.linear_wgrad slabs through ops.reduce_slabs: the final gradient = scale * dz^T x."""
    wo.check_chain(_case(R7, N, K), form, S, 2.0 ** -4, dev)


RB_R, RB_S, RB_N, RB_K = 64 * 23, 5, 128, 192


def _streamk_native(a, b, slabs, layout, N, K, R, S, **_):
    bm, bn = ops.streamk_tiles(N, K)
    part = torch.empty(ops.streamk_partial_elems(N, K, S), device=a.device)
    ops.kernels.native().gemm_bf16_streamk(
        ops.kernels._p(a), a.stride(0), ops.kernels._p(b), b.stride(0), ops.kernels._p(slabs[0]),
        slabs[0].stride(0), N, K, R, 0, layout, layout, bm, bn, S, ops.kernels._p(part),
        torch.cuda.current_stream().cuda_stream)


def _group_native(a, b, slabs, layout, N, K, R, S, **_):
    _native_group(layout)([(a, b, slabs, S, False)])


FAMILIES = [("stages2", wo.gemm_wgrad, dict(tiles=(128, 64), stages=2), RB_S),
            ("stages9", wo.gemm_wgrad, dict(tiles=(128, 64), stages=9), RB_S),
            ("persist", wo.gemm_wgrad, dict(tiles=(128, 64), persist=-1), RB_S),
            ("grouped", _group_native, {}, RB_S),
            ("stream-k", _streamk_native, {}, 1)]  # 5 workgroups; one fp32 result, no slabs


@pytest.mark.parametrize("form", wo.FORMS)
@pytest.mark.parametrize("name,run,launch,S", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_random_operands_within_the_summation_bound(dev, name, run, launch, S, form):
    """Normal deviates rounded to bf16, R = 64 * 23, S = 5 (stream-K: 5 workgroups over 3 tiles
    of 23 steps, at most 3 partial sums per tile): |got - fp64| <= (R + S) * 2^-24 *
    (|dz|^T |x|) in every element (tests/_wgrad_oracle.random_bound)."""
    case = _case(RB_R, RB_N, RB_K, random=True)
    if name == "stream-k":
        assert wo.streamk_geometry(RB_N, RB_K, RB_R, RB_S)["straddle"]
        a, b, layout = wo.operands(case, form, dev)
        buf, out = wo.out_slabs(1, RB_N, RB_K, dev)
        _streamk_native(a, b, out, layout, RB_N, RB_K, RB_R, RB_S)
        wo.assert_outside_untouched(buf, 1, RB_N, RB_K, "random stream-K")
        got = out[0]
    else:
        got = wo.reduced_gradient(case, form, S, dev, run=run, **launch)
    ratio = wo.random_ratio(got, case, RB_S, f"{name} {form}")
    print(f"\nWGRADSTAT {name} {form} R={RB_R} S={RB_S} worst |err|/bound {ratio:.5f}")
    assert ratio <= 1.0
