"""fp64 oracle of softmax cross-entropy, shared by the loss tests (CPU and GPU).

Method (as tests/_act_oracle.py): what reaches the softmax is EXACT in fp32 -- logits generated
as multiples of 1/4, or GEMM operands whose every product and partial sum is a dyadic fraction
inside 24 bits -- and the oracle is evaluated in fp64 from the same numbers. Every generator
asserts that on the CPU (fp32 matmul == fp64 matmul bit for bit). What a kernel stores can then
differ from the oracle only by the softmax arithmetic itself.

Derivation of the bounds (u = 2^-24, fp32 unit roundoff; t = mx - x_c >= 0 exact):
  * e_c = __expf(-t): the argument of the base-2 exponential, -t * log2(e), is rounded to fp32,
    an absolute error of t * u in the exponent, so e_c is off by e^-t * t * u <= 0.37 u
    absolutely (t * e^-t <= 1/e), plus about 2 ulps of the hardware exponential: <= 3 u.
  * se = sum of n_cls such terms, each <= 1, summed serially or as a tree: relative error
    <= (n_cls - 1) u from the additions on top of the terms' own; inv = 1 / se and the product
    e_c * inv add 3 more roundings. The probability p_c = e_c / se therefore carries
    <= (n_cls + 5) u relative and <= 3 u absolute error: <= (n_cls + 8) u absolutely (p <= 1).
  * dz = (p - onehot) * scale, rounded ONCE to bf16 (2^-9 relative). The fp32 value lies within
    |scale| * (n_cls + 8) u of the exact one -- far inside half a bf16 ulp unless p_label - 1
    cancels or the entry underflows -- so the stored value is one of the two bf16 neighbours of
    the exact one, or within the absolute term of it:
        |got - want| <= 1 * bf16_ulp(want) + |scale| * (n_cls + 8) * 2^-24.
    An absolute-excess check, not an ordered-integer distance (which blows up near zero).
  * softmax_rows output (fp32, no bf16 rounding): |got - p| <= (n_cls + 8) * 2^-24.
  * loss_r = log(se) - (x_label - mx): the difference is exact, log(se) inherits se's relative
    error as an ABSOLUTE one ((n_cls + 5) u, plus 3 u for __logf and the final subtraction at
    log-sized values), and the subtraction rounds relative to loss_r. A partial sums at most 64
    rows per wave-sized group in fp32, each addition relative to the running sum <= sum(loss):
        |got - want| <= 2^-18 * sum(loss_r) + valid_rows * (n_cls + 8) * 2^-24
    over the rows of THAT partial (64 additions * 2^-24 = 2^-18). A partial without valid rows
    is exactly 0.
  * colsum partial = fp32 sum of at most 64 stored bf16 values per (block, column), compared
    with the fp64 sum of the kernel's own stored dz: 64 * 2^-24 * sum|dz| (+ 1e-30).
  * correct counts and argmax are integers: exact.
"""
from __future__ import annotations

import torch

from _act_oracle import (CPU, PAD, SENTINEL, act_fwd, assert_padding_untouched, bf16_ulp, padded,
                         rn_bf16)
from docker_dist_nn_amd import ops

U = 2.0 ** -24
XENT_BLOCK_ROWS = 64  # rows per loss partial of the stand-alone kernel (ops.xent_blocks)
XENT_SHAPES = [(64, 1), (64, 2), (64, 10), (64, 64), (128, 65), (128, 100), (256, 256),
               (192, 130)]  # (width, n_cls): both instantiations of softmax_xent_kernel
XENT_ROWS = [1, 63, 64, 65, 300]
GEMM_SHAPES = [(64, 64, 64, 10), (192, 64, 128, 64), (128, 128, 64, 1), (256, 128, 128, 100),
               (128, 128, 128, 128)]  # (M, Np, K, n_cls)
TAIL_GEOS = [(144, 64, 64, 64, 10), (144, 128, 128, 128, 16), (144, 256, 128, 64, 1),
             (144, 64, 64, 64, 2), (4096 + 48, 256, 128, 64, 10)]  # (rows, k3, n3, n4, n_cls)
ROWS_CLS = [1, 10, 64, 65, 256]
ROWS_ROWS = [1, 5, 257]
ISENT = 1000  # prefill of int32 count buffers
NAN = float("nan")


# ---- fp64 reference -------------------------------------------------------------------------

def xent_ref(logits: torch.Tensor, labels: torch.Tensor, scale: float) -> dict:
    """logits fp64 [rows][n_cls], labels int (-1 = padding row). dz [rows][n_cls], per-row loss
    (0 for padding rows), p, argmax (lowest index on ties, as np.argmax), correct."""
    x = logits.double()
    rows, n_cls = x.shape
    lab = labels[:rows].long()
    valid = lab >= 0
    safe = lab.clamp_min(0)
    mx = x.max(1, keepdim=True).values
    e = torch.exp(x - mx)
    se = e.sum(1, keepdim=True)
    p = e / se
    onehot = torch.zeros_like(x)
    onehot[torch.arange(rows), safe] = 1.0
    dz = (p - onehot) * float(scale)
    dz[~valid] = 0.0
    loss = (mx + torch.log(se))[:, 0] - x[torch.arange(rows), safe]
    loss = torch.where(valid, loss, torch.zeros_like(loss))
    idx = torch.arange(n_cls).expand(rows, n_cls)
    argmax = torch.where(x == mx, idx, torch.full_like(idx, n_cls)).min(1).values
    return dict(dz=dz, loss=loss, p=p, argmax=argmax, correct=valid & (argmax == lab),
                valid=valid, n_cls=n_cls, scale=float(scale))


# ---- comparators ----------------------------------------------------------------------------

def new_stats() -> dict:
    return dict(dz=0.0, p=0.0, loss=0.0, colsum=0.0)


def _note(stats, key, ratio):
    if stats is not None:
        stats[key] = max(stats[key], float(ratio))


def statline(name: str, stats: dict) -> str:
    return "LOSSSTAT " + name + " worst/bound " + " ".join(
        f"{k} {v:.3f}" for k, v in stats.items() if v > 0.0 or k == "dz")


def assert_dz(got, ref, width=None, stats=None, what=""):
    """Stored bf16 dz [rows][width]: the first n_cls columns within the derived bound of the
    oracle, the padding columns n_cls..width exactly zero, no NaN."""
    got = got.detach().to(CPU).double()
    n_cls = ref["n_cls"]
    assert not torch.isnan(got).any(), f"{what}: NaN in dz"
    want = ref["dz"]
    bound = bf16_ulp(want) + abs(ref["scale"]) * (n_cls + 8) * U
    ratio = ((got[:, :n_cls] - want).abs() / bound).max() if want.numel() else 0.0
    _note(stats, "dz", ratio)
    assert float(ratio) <= 1.0, (f"{what}: dz off by {float(ratio):.2f} x the bound at "
                                 f"{((got[:, :n_cls] - want).abs() > bound).nonzero()[:4].tolist()}")
    if width is not None:
        assert got.shape[1] >= width
    assert bool((got[:, n_cls:width] == 0).all()), f"{what}: dz padding columns not zero"


def assert_probs(got, ref, stats=None, what=""):
    got = got.detach().to(CPU).double()
    assert not torch.isnan(got).any(), f"{what}: NaN in the probabilities"
    ratio = ((got - ref["p"]).abs() / ((ref["n_cls"] + 8) * U)).max()
    _note(stats, "p", ratio)
    assert float(ratio) <= 1.0, f"{what}: softmax off by {float(ratio):.2f} x the bound"


def owners(rows: int, rows_per: int, n_part: int = 0) -> torch.Tensor:
    """Partial index of every row: block of ``rows_per`` rows, dealt round-robin over
    ``n_part`` partials when given (the tail), else one partial per block."""
    blk = torch.arange(rows) // rows_per
    return blk % n_part if n_part else blk


def assert_loss_partials(got, ref, owner, n_part, stats=None, what=""):
    got = got.detach().to(CPU).double()[:n_part]
    assert not torch.isnan(got).any(), f"{what}: NaN loss (saturated row?)"
    want = torch.zeros(n_part, dtype=torch.float64).index_add_(0, owner, ref["loss"])
    nval = torch.zeros(n_part, dtype=torch.float64).index_add_(0, owner, ref["valid"].double())
    bound = 2.0 ** -18 * want + nval * (ref["n_cls"] + 8) * U
    err = (got - want).abs()
    empty = nval == 0
    assert bool((got[empty] == 0).all()), f"{what}: an all-padding partial is not exactly 0"
    if bool((~empty).any()):
        ratio = (err[~empty] / bound[~empty]).max()
        _note(stats, "loss", ratio)
        assert float(ratio) <= 1.0, (f"{what}: loss partial off by {float(ratio):.2f} x the "
                                     f"bound: got {got.tolist()[:6]} want {want.tolist()[:6]}")


def assert_correct_partials(got, ref, owner, n_part, base=0, what=""):
    want = torch.zeros(n_part, dtype=torch.int64).index_add_(0, owner, ref["correct"].long())
    got = got.detach().to(CPU).long()[:n_part]
    assert torch.equal(got, want + base), f"{what}: correct {got.tolist()[:8]} != " \
                                          f"{(want + base).tolist()[:8]}"


def assert_colsum_partials(cs, stored, owner, n_part, stats=None, what=""):
    """fp32 partial column sums against fp64 sums of the kernel's OWN stored dz."""
    s = stored.detach().to(CPU).double()
    cols = s.shape[1]
    want = torch.zeros(n_part, cols, dtype=torch.float64).index_add_(0, owner, s)
    mag = torch.zeros(n_part, cols, dtype=torch.float64).index_add_(0, owner, s.abs())
    got = cs.detach().to(CPU).double()[:n_part, :cols]
    assert not torch.isnan(got).any(), f"{what}: NaN colsum"
    ratio = ((got - want).abs() / (64 * U * mag + 1e-30)).max()
    _note(stats, "colsum", ratio)
    assert float(ratio) <= 1.0, f"{what}: colsum off by {float(ratio):.2f} x the bound"


# ---- edge rows ------------------------------------------------------------------------------

def _labels(rows: int, n_cls: int, g, blk: int) -> torch.Tensor:
    """Random labels; (e): every 7th row from row 8 on, the whole second ``blk``-row block
    (where there is one) and the last row (where the edge rows leave it free) are padding."""
    lab = torch.randint(0, n_cls, (rows,), generator=g, dtype=torch.int32)
    lab[8::7] = -1
    if rows > blk:
        lab[blk:2 * blk] = -1
    if rows > 4:
        lab[rows - 1] = -1
    return lab


def _pair(n_cls: int) -> tuple[int, int]:
    """Columns of the shared maximum of edge row (b): c1 < c2, in different 64-column chunks
    once n_cls > 64."""
    return n_cls // 3, n_cls - 1


# ---- stand-alone kernel / softmax_rows ------------------------------------------------------

def logits_case(rows: int, n_cls: int, seed: int, blk: int = 64) -> dict:
    """fp32 logits, all multiples of 1/4 with |x| <= 200. Rows 0..3 (as far as there are rows):
    (a) all equal, label = last column; (b) the maximum shared by two columns, label = the
    higher one; (c) the label 320 below the maximum; (d) the label 130..140 above the rest."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-40, 41, (rows, n_cls), generator=g).double() / 4
    lab = _labels(rows, n_cls, g, blk)
    c1, c2 = _pair(n_cls)
    x[0], lab[0] = 2.5, n_cls - 1
    if rows > 1 and n_cls > 1:
        x[1, c1], x[1, c2], lab[1] = 12.0, 12.0, c2
    if rows > 2 and n_cls > 1:
        x[2, 0], x[2, c2], lab[2] = 150.0, -170.0, c2
    if rows > 3 and n_cls > 1:
        x[3, n_cls // 2], lab[3] = 140.0, n_cls // 2
    assert float(x.abs().max()) <= 200.0 and torch.equal(x.float().double(), x)
    assert torch.equal((x * 4).round(), x * 4)
    return dict(rows=rows, n_cls=n_cls, x=x, labels=lab)


def check_softmax_xent(case, width, scale, dev, colsum=True, loss=True, correct=True,
                       stats=None):
    """ops.softmax_xent on padded views: NaN around the logits and in their columns >= n_cls,
    sentinel around dz; loss / correct / colsum per 64-row block."""
    rows, n_cls = case["rows"], case["n_cls"]
    what = f"softmax_xent {rows}x{width} cls={n_cls} scale={scale:.3g}"
    data = torch.full((rows, width), NAN)
    data[:, :n_cls] = case["x"].float()
    _, lg = padded(rows, width, torch.float32, NAN, dev, data)
    buf, dz = padded(rows, width, torch.bfloat16, SENTINEL, dev)
    nb = ops.xent_blocks(rows)
    lp = torch.full((nb + 1,), SENTINEL, dtype=torch.float32, device=dev) if loss else None
    co = torch.full((nb + 1,), ISENT, dtype=torch.int32, device=dev) if correct else None
    cs = torch.full((nb + 1, width + PAD), SENTINEL, dtype=torch.float32, device=dev) \
        if colsum else None
    ops.softmax_xent(lg, case["labels"].to(dev), dz, n_cls, scale, lp, co, colsum=cs)
    ref = xent_ref(case["x"], case["labels"], scale)
    assert_dz(dz, ref, width, stats, what)
    assert_padding_untouched(buf, rows, width, what=what)
    own = owners(rows, XENT_BLOCK_ROWS)
    if loss:
        assert_loss_partials(lp, ref, own, nb, stats, what)
        assert float(lp[nb]) == SENTINEL, f"{what}: loss_part written past the last block"
    if correct:
        assert_correct_partials(co, ref, own, nb, what=what)
        assert int(co[nb]) == ISENT, f"{what}: correct written past the last block"
    if colsum:
        assert_colsum_partials(cs[:, :width], dz, own, nb, stats, what)
        outside = cs.detach().to(CPU)
        assert bool((outside[nb:] == SENTINEL).all()) and \
            bool((outside[:, width:] == SENTINEL).all()), f"{what}: colsum wrote outside"
    return ref


def check_softmax_rows(case, dev, out=True, labels=True, pred=True, stats=None):
    """ops.softmax_rows from a NaN-padded view (ld_in > n_cls): probabilities, argmax with the
    lowest-index tie rule, and the correct counter ACCUMULATED onto its previous value."""
    rows, n_cls = case["rows"], case["n_cls"]
    what = f"softmax_rows {rows} cls={n_cls}"
    _, lg = padded(rows, n_cls, torch.float32, NAN, dev, case["x"].float())
    obuf, o = padded(rows, n_cls, torch.float32, SENTINEL, dev) if out else (None, None)
    lab = case["labels"].to(dev) if labels else None
    pr = torch.full((rows + 1,), ISENT, dtype=torch.int32, device=dev) if pred else None
    co = torch.full((1,), ISENT, dtype=torch.int32, device=dev)
    ops.softmax_rows(lg, o, n_cls, lab, pr, co)
    ref = xent_ref(case["x"], case["labels"], 1.0)
    if out:
        assert_probs(o, ref, stats, what)
        assert_padding_untouched(obuf, rows, n_cls, what=what)
    if pred:
        assert torch.equal(pr.to(CPU).long()[:rows], ref["argmax"]), f"{what}: argmax"
        assert int(pr[rows]) == ISENT
    assert int(co[0]) == ISENT + (int(ref["correct"].sum()) if labels else 0), f"{what}: correct"


# ---- fused GEMM -----------------------------------------------------------------------------

_BIAS = (0.5, 0.75, 0.0, -1.0, -3.0, 1.0, 1.25, 1.5, 2.0, 3.0, 5.0)  # 1 - b is 0 or +-2^s


def _pow2(shape, g, lo, hi, zeros=True):
    sign = torch.randint(-1 if zeros else 0, 2, shape, generator=g).double()
    if not zeros:
        sign = sign * 2 - 1
    return sign * torch.pow(torch.tensor(2.0, dtype=torch.float64),
                            torch.randint(lo, hi + 1, shape, generator=g).double())


def gemm_case(M, Np, K, n_cls, seed, blk=64, pad_weights=True) -> dict:
    """x[M][K] (multiples of 1/16 in [-1, 1]), w[Np][K] in {-1, 0, 1} * 2^s, bias multiples of
    1/4; K <= 128. Feature 0 cancels the bias (w[c][0] = 1 - bias[c]), features 1..3 carry the
    edge patterns, so the edge rows 0..3 are one-hot sums: (a) e0 -> every logit 1; (b) e0 + e1
    -> 1 + 4 in two columns; (c) e0 + e2 -> 129 in column 0, the label at 1; (d) e0 + e3 -> the
    label at 129. Rows n_cls..Np of w and bias are non-zero padding (``pad_weights``) that must
    not reach any output."""
    assert K <= 128 and M > 4
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-16, 17, (M, K), generator=g).double() / 16
    x[:, :4] = 0.0
    x[:4] = 0.0
    w = _pow2((Np, K), g, -2, 2)
    bias = torch.tensor(_BIAS, dtype=torch.float64)[torch.randint(0, len(_BIAS), (Np,),
                                                                  generator=g)]
    lab = _labels(M, n_cls, g, blk)
    c1, c2 = _pair(n_cls)
    w[:n_cls, :4] = 0.0
    w[:n_cls, 0] = 1.0 - bias[:n_cls]
    x[0, 0], lab[0] = 1.0, n_cls - 1
    if n_cls > 1:
        w[c1, 1] = w[c2, 1] = 4.0
        x[1, 0] = x[1, 1] = 1.0
        lab[1] = c2
        w[:n_cls, 2] = torch.randint(-1, 2, (n_cls,), generator=g).double()
        w[0, 2], w[c2, 2] = 128.0, 0.0
        x[2, 0] = x[2, 2] = 1.0
        lab[2] = c2
        w[:n_cls, 3] = torch.randint(-1, 2, (n_cls,), generator=g).double()
        w[n_cls // 2, 3] = 128.0
        x[3, 0] = x[3, 3] = 1.0
        lab[3] = n_cls // 2
    if pad_weights:
        w[n_cls:] = _pow2((Np - n_cls, K), g, -2, 7, zeros=False)
        bias[n_cls:] = 3.25
    else:
        w[n_cls:], bias[n_cls:] = 0.0, 0.0
    z = x @ w[:n_cls].t() + bias[:n_cls]
    z32 = x.float() @ w[:n_cls].float().t() + bias[:n_cls].float()
    assert torch.equal(z32.double(), z), "gemm_case: logits not exact in fp32 (test bug)"
    assert torch.equal(x.to(torch.bfloat16).double(), x)
    assert torch.equal(w.to(torch.bfloat16).double(), w)
    if n_cls > 1:
        assert float(z[2].max() - z[2, c2]) >= 120 and float(z[3, n_cls // 2] - 120) >= \
            float(z[3][torch.arange(n_cls) != n_cls // 2].max())
        assert float(z[1, c1]) == float(z[1, c2]) == float(z[1].max())
    assert bool((z[0] == z[0, 0]).all())
    return dict(M=M, Np=Np, K=K, n_cls=n_cls, x=x.to(torch.bfloat16), w=w.to(torch.bfloat16),
                bias=bias.float(), labels=lab, z=z)


def run_linear_fwd_xent(case, scale, dev, colsum=True):
    M, Np, n_cls = case["M"], case["Np"], case["n_cls"]
    bm = ops.xent_tiles(M, Np)[0]
    nt = M // bm
    buf, dz = padded(M, Np, torch.bfloat16, SENTINEL, dev)
    dz.fill_(SENTINEL)
    lp = torch.full((nt + 1,), SENTINEL, dtype=torch.float32, device=dev)
    co = torch.full((nt + 1,), ISENT, dtype=torch.int32, device=dev)
    cs = torch.full((nt + 1, Np + PAD), SENTINEL, dtype=torch.float32, device=dev) \
        if colsum else None
    ops.linear_fwd_xent(case["x"].to(dev), case["w"].to(dev), case["bias"].to(dev), dz,
                        case["labels"].to(dev), n_cls, scale, lp, co, colsum=cs)
    return dict(buf=buf, dz=dz, loss=lp, corr=co, cs=cs, bm=bm, nt=nt)


def check_linear_fwd_xent(case, scale, dev, stats=None):
    M, Np, n_cls = case["M"], case["Np"], case["n_cls"]
    what = f"linear_fwd_xent {M}x{Np}x{case['K']} cls={n_cls}"
    out = run_linear_fwd_xent(case, scale, dev)
    ref = xent_ref(case["z"], case["labels"], scale)
    assert_dz(out["dz"], ref, Np, stats, what)
    assert_padding_untouched(out["buf"], M, Np, what=what)
    own, nt = owners(M, out["bm"]), out["nt"]
    assert_loss_partials(out["loss"], ref, own, nt, stats, what)
    assert_correct_partials(out["corr"], ref, own, nt, what=what)
    assert float(out["loss"][nt]) == SENTINEL and int(out["corr"][nt]) == ISENT
    assert_colsum_partials(out["cs"][:, :Np], out["dz"], own, nt, stats, what)
    cs = out["cs"].to(CPU)
    assert bool((cs[nt:] == SENTINEL).all()) and bool((cs[:, Np:] == SENTINEL).all())
    return out


# ---- fused classifier tail ------------------------------------------------------------------

def tail_case(rows, k3, n3, n4, n_cls, act3, act2, seed) -> dict:
    """Operands of ops.mlp_tail as tests/test_mlp_tail_gpu.py::_exact_case makes them (x a
    multiple of 1/8, w3 of 1/8 in {-1, 0, 1}/8, b3 of 1/4), w4 in {-1, 0, 1}/8 and b4 chosen so
    that an all-zero input row gives every class the logit 1: edge rows (a) = rows 0 and 2
    (labels last / first class). Feature 0 drives hidden unit 0 alone, and unit 0 feeds only two
    classes, so row 1 (x = e0) is (b): the maximum shared by two columns, the label the higher
    one. Rows n_cls..15 of w4 and those entries of b4 are non-zero padding."""
    g = torch.Generator().manual_seed(seed)
    if act2 == "sigmoid":
        x = torch.randint(1, 16, (rows, k3), generator=g).double() / 16
    else:
        x = torch.randint(-8, 9, (rows, k3), generator=g).double() / 8
        if act2 == "relu":
            x = x.clamp_min(0)
    w3 = torch.randint(-1, 2, (n3, k3), generator=g).double() / 8
    b3 = torch.randint(-8, 9, (n3,), generator=g).double() * 0.25
    w3[0, :], w3[:, 0], w3[0, 0], b3[0] = 0.0, 0.0, 0.125, 0.25
    w4 = torch.zeros(n4, n3, dtype=torch.float64)
    w4[:n_cls] = torch.randint(-1, 2, (n_cls, n3), generator=g).double() / 8
    c1, c2 = _pair(n_cls)
    w4[:n_cls, 0] = 0.0
    w4[c1, 0] = w4[c2, 0] = 0.125
    w4[n_cls:16] = (torch.randint(0, 2, (16 - n_cls, n3), generator=g).double() * 2 - 1) / 8
    hb = rn_bf16(act_fwd(b3, act3)).double()  # h3 of an all-zero input row
    b4 = torch.full((n4,), 0.75, dtype=torch.float64)
    b4[:n_cls] = 1.0 - w4[:n_cls] @ hb
    b4[16:] = 0.0
    assert torch.equal(b4.float().double(), b4)
    lab = _labels(rows, n_cls, g, 16)
    x[0], lab[0] = 0.0, n_cls - 1
    x[1], lab[1] = 0.0, c2
    x[1, 0] = 0.5 if act2 == "sigmoid" else 1.0
    x[2], lab[2] = 0.0, 0
    bf = torch.bfloat16
    return dict(rows=rows, k3=k3, n3=n3, n4=n4, n_cls=n_cls, act3=act3, act2=act2,
                x=x.to(bf), w3=w3.to(bf), b3=b3.float(), w4=w4.to(bf), b4=b4.float(),
                labels=lab)


def tail_logits(h3, w4, b4, n_cls, strict=True):
    """fp64 logits from the kernel's OWN stored h3; exact in fp32 or (strict) a test bug.
    Returns (logits, exact)."""
    h3, w4, b4 = h3.detach().to(CPU), w4.detach().to(CPU), b4.detach().to(CPU)
    z = h3.double() @ w4[:n_cls].double().t() + b4[:n_cls].double()
    z32 = h3.float() @ w4[:n_cls].float().t() + b4[:n_cls].float()
    exact = torch.equal(z32.double(), z)
    assert exact or not strict, "tail logits not exact in fp32 (test bug)"
    return z, exact


def run_tail(case, scale, dev):
    rows, k3, n3, n4 = case["rows"], case["k3"], case["n3"], case["n4"]
    nb = ops.tail_blocks(rows)
    bf, f32 = torch.bfloat16, torch.float32
    dz4 = torch.zeros(rows, n4, dtype=bf)
    dz4[:, :16] = SENTINEL  # columns >= 16 stay the caller's zeros
    out = dict(h3=torch.full((rows, n3), SENTINEL, dtype=bf, device=dev), dz4=dz4.to(dev),
               dz3=torch.full((rows, n3), SENTINEL, dtype=bf, device=dev),
               dz2=torch.full((rows, k3), SENTINEL, dtype=bf, device=dev),
               loss=torch.full((nb + 1,), SENTINEL, dtype=f32, device=dev),
               corr=torch.full((nb + 1,), ISENT, dtype=torch.int32, device=dev),
               cs4=torch.full((nb, n4), SENTINEL, dtype=f32, device=dev),
               cs3=torch.full((nb, n3), SENTINEL, dtype=f32, device=dev),
               cs2=torch.full((nb, k3), SENTINEL, dtype=f32, device=dev), nb=nb)
    t = [case[k].to(dev) for k in ("x", "w3", "b3", "w4", "b4", "labels")]
    ops.mlp_tail(*t, out["h3"], out["dz4"], out["dz3"], out["dz2"], case["n_cls"], scale,
                 act3=case["act3"], act2=case["act2"], loss_part=out["loss"],
                 correct=out["corr"], cs4=out["cs4"], cs3=out["cs3"], cs2=out["cs2"])
    return out


def check_tail(case, scale, dev, stats=None):
    rows, n_cls, n4 = case["rows"], case["n_cls"], case["n4"]
    what = f"mlp_tail {rows}x{case['k3']}x{case['n3']}x{n4} cls={n_cls} {case['act3']}"
    out = run_tail(case, scale, dev)
    z, _ = tail_logits(out["h3"], case["w4"], case["b4"], n_cls)
    if case["act3"] != "sigmoid":  # rows (a) and (b) are exact ties of the stored h3
        c1, c2 = _pair(n_cls)
        assert bool((z[0] == 1.0).all()) and bool((z[2] == 1.0).all())
        assert float(z[1, c1]) == float(z[1, c2]) == float(z[1].max()) > 1.0
    ref = xent_ref(z, case["labels"], scale)
    assert_dz(out["dz4"], ref, n4, stats, what)
    nb = out["nb"]
    own = owners(rows, 16, nb)
    assert_loss_partials(out["loss"], ref, own, nb, stats, what)
    assert_correct_partials(out["corr"], ref, own, nb, what=what)
    assert float(out["loss"][nb]) == SENTINEL and int(out["corr"][nb]) == ISENT
    assert_colsum_partials(out["cs4"], out["dz4"], own, nb, stats, what)
    return out
