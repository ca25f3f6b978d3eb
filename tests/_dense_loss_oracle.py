"""fp64 oracle of the dense-target losses (ops.dense_loss: mse | bce), shared by the CPU and GPU
tests.

Method (as tests/_loss_oracle.py): what reaches the loss is EXACT in fp32 -- pre-activations z
are multiples of 1/4 with |z| <= 200, targets t multiples of 1/8 in [0, 1] (exact in bf16) -- and
the oracle is evaluated in fp64 from the same numbers, so a stored value can differ from it only
by the loss arithmetic itself. Buffers are padded views: NaN around z and t, in their columns
>= n_out and in the z rows of padding rows; a sentinel around every output.

Derivation of the bounds (u = 2^-24, fp32 unit roundoff; n = n_out; coef = (2 | 1) * scale / n):
  * coef: scale is rounded to fp32 when passed (u), the quotient is rounded once more (u):
    <= 2 u relative. inv_n = fl(1 / n): u relative.
  * linear / relu: d = y - t is exact (multiples of 1/8 below 2^8), g = coef * d is one
    rounding: g is within 4 u |g| of the exact value.
  * sigmoid, from e = __expf(-|z|), s = 1 + e, p = 1 / s, q = e * p (y = p or q, y (1 - y) = p q):
    the exponent argument -|z| log2(e) is rounded to fp32, an error of |z| u relative in e, plus
    2 ulps (4 u) of the hardware exponential: e is off by e (|z| + 4) u <= 5 u absolutely
    (|z| e^-|z| <= 1/e, e <= 1). s adds one rounding (u, s in [1, 2]): 6 u relative; the
    hardware reciprocal 1 ulp (2 u): p within 8 u relative and absolute (p <= 1); q = e p within
    (|z| + 13) u relative, so within (0.37 + 13) u < 14 u absolutely (q <= e). Hence y is within
    14 u absolutely, d = y - t (one rounding, |d| <= 1) within 15 u.
      - bce: g = coef * d, <= coef * (15 u + 3 u |d|) <= 18 u coef from the exact one.
      - mse: p q carries (|z| + 22) u relative, <= 6 u absolute (p q <= min(e, 1/4)); d * (p q)
        is within 15 u / 4 + 6 u + u / 4 = 10 u, and g = coef * that within 11 u coef.
    Both are covered by 24 u coef.
  * dz is g rounded ONCE to bf16: the fp32 value lies far inside half a bf16 ulp (2^-9
    relative) of the exact one unless y - t cancels, so the stored value is one of the two bf16
    neighbours of the exact one, or within the fp32 term of it:
        |got - want| <= 1 * bf16_ulp(want) + 4 u |want| + [sigmoid] 24 u coef.
    Columns n_out..width and padding rows are exactly 0.
  * loss term of one element (before the 1 / n), all terms >= 0:
      - mse linear / relu: d exact, term = fl(d^2): u relative, no absolute part (C = 0);
      - mse sigmoid: d within 15 u, |d| <= 1: d^2 within 30 u + u + (15 u)^2 < 32 u (C = 32);
      - bce: a = max(z, 0) - t z is exact (multiples of 1/32 below 2^8, contracted to an fma or
        not); L = __logf(s): s within 6 u relative = 6 u absolute in the logarithm, the hardware
        log2 1 ulp at values <= 1 (2 u) times ln 2 (two roundings at L <= 0.7: 1.4 u), < 10 u;
        the final addition rounds relative to the term: C = 12 covers it, plus u relative.
    A partial (64 rows x 256 columns) adds 64 terms serially per lane, then 6 butterfly levels
    and 2 LDS levels: 72 additions, each relative to a running sum <= the total; the product
    with inv_n adds 2 u:
        |got - want| <= 76 u want + valid_elements * C u / n,     want = sum(term) / n
    over the valid rows and columns < n_out of THAT partial. A partial without a valid element
    holds the exact sum 0.
  * colsum partial = fp32 sum of at most 64 stored bf16 values per (row block, column) -- 16
    serial additions per lane and 2 LDS levels -- compared with the fp64 sum of the kernel's own
    stored dz: 64 u sum|dz| (+ 1e-30), as tests/_loss_oracle.py.
"""
from __future__ import annotations

import functools

import torch

import _loss_oracle as lo
from _act_oracle import CPU, PAD, SENTINEL, bf16_ulp
from docker_dist_nn_amd import ops

U = 2.0 ** -24
NAN = float("nan")
BLOCK_ROWS = 64   # rows per partial (ops.dense_loss_row_blocks = ops.xent_blocks)
CHUNK_COLS = 256  # columns per partial (ops.dense_loss_col_chunks)
SHAPES = [(64, 1), (64, 10), (64, 64), (128, 65), (256, 256), (320, 257), (832, 784)]
ROWS = [1, 63, 64, 65, 300]
PAIRS = [("mse", "linear"), ("mse", "relu"), ("mse", "sigmoid"), ("bce", "sigmoid")]
TERM_C = {("mse", "linear"): 0.0, ("mse", "relu"): 0.0, ("mse", "sigmoid"): 32.0,
          ("bce", "sigmoid"): 12.0}


# ---- cases ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def dense_case(rows: int, n_out: int, seed: int) -> dict:
    """z [rows][n_out] multiples of 1/4, |z| <= 200; t multiples of 1/8 in [0, 1]; row_ok (0 =
    valid, -1 = padding). Edge rows, as far as there are rows: 0: z = +200, t alternating 0 / 1;
    1: z = -200, t alternating 1 / 0; 2: z = 0 (the relu kink), t = 1/2; 3: z = +-(50..200) mixed,
    t exactly 0 or 1. Padding: every 7th row from row 8 on, the whole second 64-row block and
    the last row (where the edge rows leave it free)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randint(-40, 41, (rows, n_out), generator=g).double() / 4
    t = torch.randint(0, 9, (rows, n_out), generator=g).double() / 8
    alt = (torch.arange(n_out) % 2).double()
    z[0], t[0] = 200.0, alt
    if rows > 1:
        z[1], t[1] = -200.0, 1.0 - alt
    if rows > 2:
        z[2], t[2] = 0.0, 0.5
    if rows > 3:
        sign = torch.randint(0, 2, (n_out,), generator=g).double() * 2 - 1
        z[3] = sign * torch.randint(200, 801, (n_out,), generator=g).double() / 4
        t[3] = torch.randint(0, 2, (n_out,), generator=g).double()
    ok = torch.zeros(rows, dtype=torch.int32)
    ok[8::7] = -1
    if rows > BLOCK_ROWS:
        ok[BLOCK_ROWS:2 * BLOCK_ROWS] = -1
    if rows > 4:
        ok[rows - 1] = -1
    assert float(z.abs().max()) <= 200.0 and torch.equal((z * 4).round(), z * 4)
    assert torch.equal(z.float().double(), z) and torch.equal(t.to(torch.bfloat16).double(), t)
    assert float(t.min()) >= 0.0 and float(t.max()) <= 1.0
    return dict(rows=rows, n_out=n_out, z=z, t=t, ok=ok)


def dense_ref(case: dict, loss: str, act: str, scale: float, use_ok: bool) -> dict:
    """fp64 dz [rows][n_out], per-element loss terms already divided by n, validity."""
    z, t, n = case["z"], case["t"], case["n_out"]
    valid = case["ok"] >= 0 if use_ok else torch.ones(case["rows"], dtype=torch.bool)
    e = torch.exp(-z.abs())
    p, q = 1.0 / (1.0 + e), e / (1.0 + e)
    sig = torch.where(z >= 0, p, q)
    if loss == "bce":
        assert act == "sigmoid"
        term = z.clamp_min(0.0) - t * z + torch.log1p(e)
        coef = float(scale) / n
        g = coef * (sig - t)
    else:
        coef = 2.0 * float(scale) / n
        if act == "sigmoid":
            d = sig - t
            g = coef * d * (p * q)
        elif act == "relu":
            d = z.clamp_min(0.0) - t
            g = torch.where(z > 0, coef * d, torch.zeros_like(d))
        else:
            assert act == "linear", act
            d = z - t
            g = coef * d
        term = d * d
    g = torch.where(valid[:, None], g, torch.zeros_like(g))
    term = torch.where(valid[:, None], term, torch.zeros_like(term)) / n
    return dict(dz=g, term=term, valid=valid, coef=abs(coef), n=n, sigmoid=act == "sigmoid",
                C=TERM_C[(loss, act)])


# ---- padded views ---------------------------------------------------------------------------

def view(rows, cols, dtype, fill, dev, data=None, shift=0):
    """(buffer, view): a [rows][cols] view at (PAD, PAD + shift) of a wider, taller buffer filled
    with ``fill``. shift = 0: every row 16-byte aligned; shift = 1: no row is."""
    buf = torch.full((rows + 2 * PAD, cols + 3 * PAD), fill, dtype=dtype)
    c0 = PAD + shift
    if data is not None:
        buf[PAD:PAD + rows, c0:c0 + cols] = data.to(dtype)
    buf = buf.to(dev)
    return buf, buf[PAD:PAD + rows, c0:c0 + cols]


def assert_untouched(buf, rows, cols, shift, what):
    outside = torch.ones(buf.shape, dtype=torch.bool)
    outside[PAD:PAD + rows, PAD + shift:PAD + shift + cols] = False
    assert bool((buf.to(CPU)[outside] == SENTINEL).all()), f"{what}: wrote outside [rows][width]"


# ---- comparators ----------------------------------------------------------------------------

def new_stats() -> dict:
    return dict(dz=0.0, loss=0.0, colsum=0.0)


def statline(name: str, stats: dict) -> str:
    return "STAT dense_loss " + name + " worst/bound " + " ".join(
        f"{k} {v:.3f}" for k, v in stats.items())


def assert_dz(got, ref, width, stats, what):
    got = got.detach().to(CPU).double()
    n = ref["n"]
    assert not torch.isnan(got).any(), f"{what}: NaN in dz"
    assert not torch.isinf(got).any(), f"{what}: inf in dz"
    want = ref["dz"]
    bound = bf16_ulp(want) + 4 * U * want.abs() + (24 * U * ref["coef"] if ref["sigmoid"] else 0)
    err = (got[:, :n] - want).abs()
    ratio = float((err / bound).max())
    stats["dz"] = max(stats["dz"], ratio)
    assert ratio <= 1.0, (f"{what}: dz off by {ratio:.2f} x the bound at "
                          f"{(err > bound).nonzero()[:4].tolist()}")
    assert bool((got[:, n:width] == 0).all()), f"{what}: dz padding columns not zero"
    assert bool((got[~ref["valid"]] == 0).all()), f"{what}: dz of a padding row not zero"


def assert_loss_partials(got, ref, rows, width, stats, what):
    nb, nc = -(-rows // BLOCK_ROWS), -(-width // CHUNK_COLS)
    got = got.detach().to(CPU).double()[:nb * nc].view(nb, nc)
    assert torch.isfinite(got).all(), f"{what}: non-finite loss partial"
    n = ref["n"]
    term = torch.zeros(nb * BLOCK_ROWS, nc * CHUNK_COLS, dtype=torch.float64)
    term[:rows, :n] = ref["term"]
    cnt = torch.zeros_like(term)
    cnt[:rows, :n] = ref["valid"].double()[:, None]
    want = term.view(nb, BLOCK_ROWS, nc, CHUNK_COLS).sum((1, 3))
    count = cnt.view(nb, BLOCK_ROWS, nc, CHUNK_COLS).sum((1, 3))
    bound = 76 * U * want + count * ref["C"] * U / n
    empty = count == 0
    assert bool((got[empty] == 0).all()), f"{what}: a partial without valid elements is not 0"
    if bool((~empty).any()):
        ratio = float(((got - want).abs()[~empty] / bound[~empty]).max())
        stats["loss"] = max(stats["loss"], ratio)
        assert ratio <= 1.0, (f"{what}: loss partial off by {ratio:.2f} x the bound: got "
                              f"{got.flatten().tolist()[:6]} want {want.flatten().tolist()[:6]}")


# ---- the check ------------------------------------------------------------------------------

def check_dense_loss(case, width, scale, loss, act, dev, use_ok=True, want_loss=True,
                     want_colsum=True, shift=0, stats=None):
    """ops.dense_loss on padded views against the fp64 oracle. ``shift`` = 1 moves z, t and dz
    off every vector alignment (the kernel's element-wise form)."""
    rows, n = case["rows"], case["n_out"]
    stats = new_stats() if stats is None else stats
    what = (f"dense_loss {loss}/{act} {rows}x{width} n={n} scale={scale:.3g} ok={use_ok} "
            f"shift={shift}")
    zd = torch.full((rows, width), NAN)
    zd[:, :n] = case["z"].float()
    if use_ok:
        zd[case["ok"] < 0] = NAN  # a padding row's pre-activations may be anything
    td = torch.full((rows, width), NAN)
    td[:, :n] = case["t"].float()
    _, z = view(rows, width, torch.float32, NAN, dev, zd, shift)
    _, t = view(rows, width, torch.bfloat16, NAN, dev, td, shift)
    buf, dz = view(rows, width, torch.bfloat16, SENTINEL, dev, None, shift)
    nb, nc = ops.dense_loss_row_blocks(rows), ops.dense_loss_col_chunks(width)
    assert (nb, nc) == (-(-rows // BLOCK_ROWS), -(-width // CHUNK_COLS))
    lp = torch.full((nb * nc + 1,), SENTINEL, dtype=torch.float32, device=dev) \
        if want_loss else None
    cs = torch.full((nb + 1, width + PAD), SENTINEL, dtype=torch.float32, device=dev) \
        if want_colsum else None
    ops.dense_loss(z, t, dz, n, scale, loss, act, row_ok=case["ok"].to(dev) if use_ok else None,
                   loss_part=lp, colsum=cs)
    ref = dense_ref(case, loss, act, scale, use_ok)
    assert_dz(dz, ref, width, stats, what)
    assert_untouched(buf, rows, width, shift, what)
    if want_loss:
        assert_loss_partials(lp, ref, rows, width, stats, what)
        assert float(lp[nb * nc]) == SENTINEL, f"{what}: loss_part written past the last partial"
    if want_colsum:
        lo.assert_colsum_partials(cs[:, :width], dz, lo.owners(rows, BLOCK_ROWS), nb, stats, what)
        outside = cs.detach().to(CPU)
        assert bool((outside[nb:] == SENTINEL).all()) and \
            bool((outside[:, width:] == SENTINEL).all()), f"{what}: colsum wrote outside"
    return stats


def check_shape(width, n_out, dev, stats):
    """Every allowed loss/activation pair over every row count of one (width, n_out); the
    optional arguments and the unaligned form on the row counts that cover them."""
    for rows in ROWS:
        case = dense_case(rows, n_out, 1000 * width + n_out + rows)
        for loss, act in PAIRS:
            check_dense_loss(case, width, 1.0 / rows, loss, act, dev, stats=stats)
            if rows in (65, 300):
                check_dense_loss(case, width, 1.0, loss, act, dev, use_ok=False,
                                 want_colsum=False, stats=stats)
                check_dense_loss(case, width, 0.37, loss, act, dev, want_loss=False, shift=1,
                                 stats=stats)
