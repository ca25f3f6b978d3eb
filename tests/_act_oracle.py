"""fp64 oracle of the activation epilogues, shared by the activation tests (CPU and GPU).

Method: operands are small integers (or dyadic fractions), so every product and partial sum of
the GEMM is exact in fp32 AND in fp64. What the kernel stores can then differ from the fp64
reference only by the activation arithmetic (a few fp32 ulps, 2^-24 relative each) and ONE
rounding to bf16 (2^-9 relative): the fp32 value lies within ~2^-20 of the exact one, far inside
half a bf16 ulp, so it rounds to one of the two bf16 neighbours of the exact value. Hence the
bound of :func:`assert_bf16_close`: at most 1 bf16 ulp from RN_bf16(fp64 reference), and bit
equality for linear / ReLU (no arithmetic at all between the exact sum and the rounding).
"""
from __future__ import annotations

import torch

from docker_dist_nn_amd import ops
from docker_dist_nn_amd.ops import KMAJ, MNMAJ

ACTS = ("linear", "relu", "sigmoid")
LAYOUTS = [(KMAJ, KMAJ), (KMAJ, MNMAJ), (MNMAJ, MNMAJ), (MNMAJ, KMAJ)]
PAD = 8  # rows / columns of padding in front of every padded view (16-byte aligned)
SENTINEL = 5.0
CPU = torch.device("cpu")


# ---- fp64 activations -----------------------------------------------------------------------

def act_fwd(z: torch.Tensor, act: str) -> torch.Tensor:
    z = z.double()
    if act == "relu":
        return z.clamp_min(0.0)
    if act == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-z))
    assert act == "linear", act
    return z


def act_bwd(g: torch.Tensor, y: torch.Tensor, act: str) -> torch.Tensor:
    """g * act'(z), the derivative expressed through the stored activation output y."""
    g, y = g.double(), y.double()
    if act == "relu":
        return torch.where(y > 0, g, torch.zeros_like(g))
    if act == "sigmoid":
        return g * y * (1.0 - y)
    assert act == "linear", act
    return g


# ---- bf16 comparison ------------------------------------------------------------------------

def _ordered(t: torch.Tensor) -> torch.Tensor:
    """bf16 -> integers in value order (sign-magnitude int16 view unfolded; +0 == -0 == 0)."""
    assert t.dtype == torch.bfloat16
    bits = t.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
    mag = bits & 0x7FFF
    return torch.where(bits >= 0x8000, -mag, mag)


def bf16_ulp_distance(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Number of bf16 values between a and b (0 = same value); NaN on either side = 2^16."""
    d = (_ordered(a) - _ordered(b)).abs()
    nan = torch.isnan(a.float()) | torch.isnan(b.float())
    return torch.where(nan, torch.full_like(d, 1 << 16), d)


def rn_bf16(x: torch.Tensor) -> torch.Tensor:
    """fp64 -> bf16, round to nearest (even) in ONE rounding. torch converts double -> float ->
    bf16; where the two roundings disagree with the single one, the nearer bf16 neighbour of
    the double is taken instead (an exact tie survives both conversions unchanged)."""
    x = x.double()
    c = x.float().to(torch.bfloat16)
    bits = c.view(torch.int16).to(torch.int32) & 0xFFFF
    best = c
    err = (c.double() - x).abs()
    for step in (-1, 1):  # the bf16 values next to c (same sign: c != 0 wherever this matters)
        nb = (bits + step).clamp(0, 0xFFFF)
        nb = torch.where(nb >= 0x8000, nb - 0x10000, nb).to(torch.int16).view(torch.bfloat16)
        e = (nb.double() - x).abs()
        take = torch.isfinite(nb.float()) & (e < err) & (c != 0)
        best = torch.where(take, nb, best)
        err = torch.where(take, e, err)
    return best


def assert_bf16_close(got: torch.Tensor, ref64: torch.Tensor, max_ulp: int, what="") -> float:
    """Every element of ``got`` (bf16) within ``max_ulp`` bf16 values of RN_bf16(ref64); no NaN.
    Returns the share of elements that are not identical (a figure to report, not a check)."""
    got = got.detach().to(CPU)
    assert not torch.isnan(got.float()).any(), f"{what}: NaN in the stored output"
    d = bf16_ulp_distance(got, rn_bf16(ref64))
    worst = int(d.max())
    assert worst <= max_ulp, (f"{what}: {int((d > max_ulp).sum())} of {d.numel()} elements differ "
                              f"by more than {max_ulp} bf16 ulp (worst {worst}) at "
                              f"{(d > max_ulp).nonzero()[:4].tolist()}")
    return float((d > 0).double().mean())


def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 (8 significand bits) at |x| (fp64), never below the smallest normal's."""
    e = torch.floor(torch.log2(x.double().abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7)


# ---- padded views ---------------------------------------------------------------------------

def padded(rows, cols, dtype, fill, dev, data=None):
    """(buffer, view): a [rows][cols] view at (PAD, PAD) of a wider, taller buffer filled with
    ``fill``; the view holds ``data`` when given. Row stride = cols + 3 * PAD > cols."""
    buf = torch.full((rows + 2 * PAD, cols + 3 * PAD), fill, dtype=dtype)
    if data is not None:
        buf[PAD:PAD + rows, PAD:PAD + cols] = data.to(dtype)
    buf = buf.to(dev)
    return buf, buf[PAD:PAD + rows, PAD:PAD + cols]


def assert_padding_untouched(buf, rows, cols, fill=SENTINEL, what=""):
    outside = torch.ones(buf.shape, dtype=torch.bool)
    outside[PAD:PAD + rows, PAD:PAD + cols] = False
    assert bool((buf.to(CPU)[outside] == fill).all()), f"{what}: wrote outside [M][N]"


# ---- case generators ------------------------------------------------------------------------

def _store(logical: torch.Tensor, layout: int) -> torch.Tensor:
    """[mn][k] logical matrix -> bf16 storage of the layout (KMAJ: as is, MNMAJ: [k][mn])."""
    t = logical if layout == KMAJ else logical.t()
    return t.contiguous().to(torch.bfloat16)


def fwd_case(M, N, K, la, lb, seed):
    """Forward GEMM + bias: A, B in {-1, 0, 1}, bias a multiple of 0.25. Returns the storage
    tensors, the bias and z = A.B^T + bias in fp64 (exact)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-1, 2, (M, K), generator=g).double()
    b = torch.randint(-1, 2, (N, K), generator=g).double()
    bias = torch.randint(-16, 17, (N,), generator=g).double() * 0.25
    z = a @ b.t() + bias
    return dict(M=M, N=N, K=K, la=la, lb=lb, a=_store(a, la), b=_store(b, lb),
                bias=bias.float(), z=z)


def sigmoid_aux(rows, cols, g):
    """Stored output of a sigmoid layer: sigmoid(randn) rounded to bf16 -- asymmetric, different
    in every row and column -- with about 1/8 of the entries forced to exactly 0 and 1/16 to
    exactly 1 (saturated units, and the zeros a ReLU derivative masks)."""
    y = torch.sigmoid(torch.randn(rows, cols, generator=g)).to(torch.bfloat16)
    r = torch.rand(rows, cols, generator=g)
    y[r < 0.125] = 0.0
    y[r > 0.9375] = 1.0
    y[0, 0], y[rows - 1, cols - 1] = 0.0, 1.0
    return y


def bwd_case(M, N, K, lb, seed):
    """dgrad GEMM: dx[M][N] = dz[M][K] . w[K][N] (dz in {-2..2}, w in {-1, 0, 1}), times the
    derivative from ``aux``. ``lb`` = MNMAJ: B is w as stored ([K][N]); KMAJ: the transposed
    weight shadow ([N][K])."""
    g = torch.Generator().manual_seed(seed)
    dz = torch.randint(-2, 3, (M, K), generator=g).double()
    w = torch.randint(-1, 2, (K, N), generator=g).double()
    aux = sigmoid_aux(M, N, g)
    return dict(M=M, N=N, K=K, la=KMAJ, lb=lb, a=_store(dz, KMAJ), b=_store(w.t(), lb),
                aux=aux, prod=dz @ w)


def colsum_ref(stored: torch.Tensor, rows_per: int) -> torch.Tensor:
    """fp64 column sums of the stored bf16 output per block of ``rows_per`` rows (last block
    partial): what a ``colsum`` / ``part`` output must hold."""
    s = stored.detach().to(CPU).double()
    return torch.stack([s[r:r + rows_per].sum(0) for r in range(0, s.shape[0], rows_per)])


def assert_colsum(cs, stored, rows_per, what=""):
    want = colsum_ref(stored, rows_per)
    got = cs.detach().to(CPU)[:want.shape[0], :want.shape[1]].double()
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-3, msg=lambda m: f"{what}: {m}")


# ---- runners (public ops entry points; device of the case decides CPU reference / kernel) ---

def run_fwd(case, act, dev, out_dtype=torch.bfloat16, **form):
    """ops.gemm forward into a padded view. Returns (buffer, view)."""
    M, N, K = case["M"], case["N"], case["K"]
    buf, out = padded(M, N, out_dtype, SENTINEL, dev)
    ops.gemm(case["a"].to(dev), case["b"].to(dev), out, layout_a=case["la"], layout_b=case["lb"],
             M=M, N=N, K=K, bias=case["bias"].to(dev), act=act, **form)
    return buf, out


def run_bwd(case, act, dev, tiles, **form):
    """ops.gemm dgrad (aux from a NaN-padded view, colsum requested) into a padded view.
    Returns (buffer, view, colsum)."""
    M, N, K = case["M"], case["N"], case["K"]
    buf, out = padded(M, N, torch.bfloat16, SENTINEL, dev)
    _, aux = padded(M, N, torch.bfloat16, float("nan"), dev, case["aux"])
    cs = torch.full((-(-M // tiles[0]), N + PAD), SENTINEL, dtype=torch.float32, device=dev)
    ops.gemm(case["a"].to(dev), case["b"].to(dev), out, layout_a=case["la"], layout_b=case["lb"],
             M=M, N=N, K=K, aux=aux, act=act, tiles=tiles, colsum=cs, **form)
    return buf, out, cs


def check_fwd(case, dev, stats=None, **form):
    """linear / relu bit-exact, sigmoid <= 1 bf16 ulp (bf16 output); sigmoid with fp32 output
    within (|z| + 8) * 2^-23 relative of fp64: the argument of the base-2 exponential,
    z * log2(e), is rounded to fp32 (an absolute error of |z| * 2^-24 in the exponent = the same
    RELATIVE error in e^-z, which the sigmoid passes on at most undiminished), plus a few ulps
    for the exponential, the add and the reciprocal."""
    M, N, z = case["M"], case["N"], case["z"]
    assert float(z.abs().max()) <= 80.0  # nothing overflows or goes denormal
    what = f"fwd {M}x{N}x{case['K']} {form}"
    for act in ACTS:
        buf, out = run_fwd(case, act, dev, **form)
        share = assert_bf16_close(out, act_fwd(z, act), 1 if act == "sigmoid" else 0,
                                  f"{what} {act}")
        assert_padding_untouched(buf, M, N, what=f"{what} {act}")
        if stats is not None and act == "sigmoid":
            stats["fwd_elems"] += out.numel()
            stats["fwd_diff"] += share * out.numel()
    buf, out = run_fwd(case, "sigmoid", dev, out_dtype=torch.float32, **form)
    ref = act_fwd(z, "sigmoid")
    got = out.detach().to(CPU)
    assert not torch.isnan(got).any()
    ratio = ((got.double() - ref).abs() / ref) / ((z.abs() + 8.0) * 2.0 ** -23)
    rel = float(((got.double() - ref).abs() / ref).max())
    if stats is not None:
        stats["f32_ratio"] = max(stats["f32_ratio"], float(ratio.max()))
        stats["f32_rel"] = max(stats["f32_rel"], rel)
    assert float(ratio.max()) <= 1.0, (f"{what} sigmoid fp32: relative error {rel:.3e} is "
                                       f"{float(ratio.max()):.2f} x the bound")
    assert_padding_untouched(buf, M, N, what=f"{what} sigmoid fp32")


def check_bwd(case, dev, tiles, stats=None, **form):
    """sigmoid <= 1 bf16 ulp; linear (aux present) and relu bit-exact; colsum partials = column
    sums of the stored output per row tile; NaN padding of aux never reaches [M][N]."""
    M, N = case["M"], case["N"]
    what = f"bwd {M}x{N}x{case['K']} lb={case['lb']} {tiles} {form}"
    for act in ACTS:
        buf, out, cs = run_bwd(case, act, dev, tiles, **form)
        ref = act_bwd(case["prod"], case["aux"], act)
        share = assert_bf16_close(out, ref, 1 if act == "sigmoid" else 0, f"{what} {act}")
        assert_padding_untouched(buf, M, N, what=f"{what} {act}")
        assert_colsum(cs[:, :N], out, tiles[0], f"{what} {act} colsum")
        assert bool((cs[:, N:] == SENTINEL).all()), f"{what} {act}: colsum wrote past N"
        if stats is not None and act == "sigmoid":
            stats["bwd_elems"] += out.numel()
            stats["bwd_diff"] += share * out.numel()


def new_stats():
    return dict(fwd_elems=0, fwd_diff=0.0, bwd_elems=0, bwd_diff=0.0, f32_ratio=0.0, f32_rel=0.0)


# ---- elementwise epilogues of tensor parallelism --------------------------------------------

def dact_case(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g).to(torch.bfloat16)
    return dict(rows=rows, cols=cols, x=x, aux=sigmoid_aux(rows, cols, g))


def check_dact_colsum(case, act, dev, n_part, with_part=True):
    """ops.dact_colsum on padded views (ld > cols). The product g * y is exact in fp32 (8 x 8
    significand bits) and 1 - y is exact for y >= 2^-16, so sigmoid is one fp32 rounding and
    one bf16 rounding away from fp64: 1 bf16 ulp; relu / linear copy or zero: bit-exact."""
    rows, cols = case["rows"], case["cols"]
    buf, x = padded(rows, cols, torch.bfloat16, SENTINEL, dev, case["x"])
    _, aux = padded(rows, cols, torch.bfloat16, float("nan"), dev, case["aux"])
    part = torch.full((n_part, cols), SENTINEL, dtype=torch.float32, device=dev) \
        if with_part else None
    ops.dact_colsum(x, aux, act, part, n_part)
    what = f"dact_colsum {rows}x{cols} {act} n_part={n_part}"
    share = assert_bf16_close(x, act_bwd(case["x"], case["aux"], act),
                              1 if act == "sigmoid" else 0, what)
    assert_padding_untouched(buf, rows, cols, what=what)
    if with_part:
        assert_colsum(part, x, -(-rows // n_part), what)
    return share


def bias_case(rows, cols, seed):
    """fp32 inputs that are no bf16 values but whose sum x + bias is exact in fp32 (multiples of
    2^-10 below 2^6), so the fp64 reference of linear / relu is a single rounding too."""
    g = torch.Generator().manual_seed(seed)
    x = torch.round(torch.randn(rows, cols, generator=g) * 4.0 * 1024.0) / 1024.0
    bias = torch.round(torch.randn(cols, generator=g) * 1024.0) / 1024.0
    return dict(rows=rows, cols=cols, x=x, bias=bias)


def check_bias_act_cast(case, act, dev, with_bias=True):
    rows, cols = case["rows"], case["cols"]
    _, x = padded(rows, cols, torch.float32, float("nan"), dev, case["x"])
    buf, y = padded(rows, cols, torch.bfloat16, SENTINEL, dev)
    bias = case["bias"].to(dev) if with_bias else None
    ops.bias_act_cast(x, bias, y, act)
    z = case["x"].double() + (case["bias"].double() if with_bias else 0.0)
    assert float(z.abs().max()) <= 80.0
    what = f"bias_act_cast {rows}x{cols} {act} bias={with_bias}"
    share = assert_bf16_close(y, act_fwd(z, act), 1 if act == "sigmoid" else 0, what)
    assert_padding_untouched(buf, rows, cols, what=what)
    return share
