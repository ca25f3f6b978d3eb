"""Tight bounds for the wide softmax kernels (csrc/kernels/softmax_wide.hip), on top of the fp64
oracle of tests/_loss_oracle.py (``lo``: its reference, case generator and comparators are used
as they are).

Why tighter ones: lo's bounds carry the absolute term (n_cls + 8) * 2^-24, which assumes the row
sum is ONE serial chain of n_cls - 1 additions. At 1000 classes that is 6e-5 -- the size of the
change from losing a whole 64-column chunk of an all-equal row (1/936 - 1/1000 = 6.8e-5). The
wide kernels do not sum serially, so the bounds here are derived from their actual longest
addition chain.

The chain. A row is swept by one wave; lane l adds the terms of columns 256 j + 4 l + e
(j = 0, 1, ..; e = 0 .. 3) serially in column order into one register that starts at 0, and the
64 lane sums then go through the 6-level xor butterfly. There is no cross-wave step. Lane 0
has the most terms, T = 4 floor(n_cls / 256) + min(n_cls mod 256, 4); its first addition
(0 + e) is exact; columns past n_cls contribute exp(-inf) = 0, an exact no-op. So the longest
chain of roundings in se is
    D(n_cls) = (T - 1) + 6 = 4 floor(n_cls / 256) + min(n_cls mod 256, 4) + 5   (kernel_depth)
e.g. 10 at 257 classes, 13 at 290 and 320, 21 at 1000, 22 at 1025, 41 at 2101 -- against
n_cls - 1.
An implementation with another summation order states its own depth (``depth=``); any order of
n_cls terms has depth <= n_cls - 1, which is what the CPU reference path is held to.

The bounds (u = 2^-24; t_c = mx - x_c >= 0 is exact: the logits are multiples of 1/4):
  * e_c = __expf(-t_c) = exp2(-t_c * log2e): the product is rounded (u relative in the
    argument = t_c * u relative in the result), the fp32 constant log2e is off by 0.22 u
    relative (another 0.22 t_c u) and the hardware exponential by one ulp (2 u): relative
    error <= (1.25 t_c + 2) u, absolute <= e^-t (1.25 t + 2) u <= 3 u.
  * se = sum e_c: the additions add <= D u relative; the terms' own errors add
    sum_c e_c (1.25 t_c + 2) u / se = (1.25 sum_c p_c t_c + 2) u, and sum_c p_c t_c =
    H(p) - ln(se) <= ln(n_cls) (H = entropy of the softmax). So
        rel(se) <= (D + 1.25 ln(n_cls) + 2) u.
  * p_c = e_c * (1 / se): the division and the product round once each, the division counted
    as 2 u (a reciprocal-based sequence): |p_c - exact| <= 3 u (from e_c; 1 / se <= 1)
    + p_c (rel(se) + 3 u), and with p_c <= 1
        |p_c - exact| <= (D + 1.25 ln(n_cls) + 8) u.
  * dz = (p - onehot) * scale: two more roundings of a value <= 1 in magnitude, then ONE
    rounding to bf16 (lo's argument: one of the two bf16 neighbours of the exact value, or
    within the absolute term of it):
        |dz - exact| <= 1 * bf16_ulp(exact) + |scale| (D + 1.25 ln(n_cls) + 10) u.
    p_terms() returns D + 1.25 ln(n_cls) + 10 and is used for p as well (2 u of slack there).
  * loss_r = -((x_l - mx) - __logf(se)): x_l - mx is exact; __logf(se) = log2(se) * ln2 with
    the hardware logarithm one ulp off (2 u), the constant 0.5 u and the product u, all
    relative to log(se) <= ln(n_cls): <= 4 ln(n_cls) u absolute; se's relative error arrives
    as an absolute one; the final subtraction rounds relative to loss_r:
        |loss_r - exact| <= (D + 5.25 ln(n_cls) + 2) u + u * loss_r.      (loss_terms: + 3)
    A partial is summed by lane 0 of each wave over its 16 rows (15 roundings), then
    (s0 + s1) + (s2 + s3): with the row's own last rounding a chain of 18, each relative to a
    running sum <= sum(loss_r):
        |partial - exact| <= 18 u * sum(loss_r) + valid_rows * loss_terms * u.
    A partial without valid rows is exactly 0.
  * colsum: 64 stored bf16 values added serially per (block, column) in row order: lo's bound
    64 u * sum|dz| against the fp64 sum of the kernel's own stored dz is already this chain.
  * argmax, correct: integers, exact.

Cases: lo.logits_case unmodified -- its edge rows (a)-(d) put the tied maxima at n_cls // 3 and
n_cls - 1 (different sweeps of a wide row) and labels on the last column -- plus two rows that
only a wide row has (wide_case): (e) the unique maximum, 120 above everything else, in the LAST
column, which is also the label; (f) the unique maximum in column 256, the first one a
register-resident 256-column kernel would not see.
"""
from __future__ import annotations

import math

import torch

import _loss_oracle as lo
from _act_oracle import CPU, PAD, SENTINEL, assert_padding_untouched, bf16_ulp, padded, rn_bf16
from docker_dist_nn_amd import ops

U = lo.U
WIDE_SHAPES = [(320, 257), (320, 320), (1024, 1000), (1088, 1025), (2112, 2101), (300, 290)]
NARROW_SHAPES = [(256, 256), (192, 130)]  # (width, n_cls) that must stay on the narrow kernels
ROWS_CLS = [257, 1000, 1025, 2101]
LAYOUTS = ("plain", "padded", "shifted")


def kernel_depth(n_cls: int) -> int:
    """Longest addition chain of a row sum in softmax_wide.hip (module docstring)."""
    return 4 * (n_cls // 256) + min(n_cls % 256, 4) + 5


def _depth(n_cls, depth):
    return kernel_depth(n_cls) if depth is None else depth


def p_terms(n_cls: int, depth=None) -> float:
    return _depth(n_cls, depth) + 1.25 * math.log(n_cls) + 10


def loss_terms(n_cls: int, depth=None) -> float:
    return _depth(n_cls, depth) + 5.25 * math.log(n_cls) + 3


# ---- comparators ----------------------------------------------------------------------------

def assert_dz_tight(got, ref, width=None, stats=None, what="", depth=None):
    got = got.detach().to(CPU).double()
    n_cls = ref["n_cls"]
    assert not torch.isnan(got).any(), f"{what}: NaN in dz"
    want = ref["dz"]
    bound = bf16_ulp(want) + abs(ref["scale"]) * p_terms(n_cls, depth) * U
    err = (got[:, :n_cls] - want).abs()
    ratio = (err / bound).max()
    lo._note(stats, "dz", ratio)
    assert float(ratio) <= 1.0, (f"{what}: dz off by {float(ratio):.2f} x the tight bound at "
                                 f"{(err > bound).nonzero()[:4].tolist()}")
    assert bool((got[:, n_cls:width] == 0).all()), f"{what}: dz padding columns not zero"


def assert_probs_tight(got, ref, stats=None, what="", depth=None):
    got = got.detach().to(CPU).double()
    assert not torch.isnan(got).any(), f"{what}: NaN in the probabilities"
    ratio = ((got - ref["p"]).abs() / (p_terms(ref["n_cls"], depth) * U)).max()
    lo._note(stats, "p", ratio)
    assert float(ratio) <= 1.0, f"{what}: softmax off by {float(ratio):.2f} x the tight bound"


def assert_loss_partials_tight(got, ref, owner, n_part, stats=None, what="", depth=None):
    got = got.detach().to(CPU).double()[:n_part]
    assert not torch.isnan(got).any(), f"{what}: NaN loss"
    want = torch.zeros(n_part, dtype=torch.float64).index_add_(0, owner, ref["loss"])
    nval = torch.zeros(n_part, dtype=torch.float64).index_add_(0, owner, ref["valid"].double())
    bound = 18 * U * want + nval * loss_terms(ref["n_cls"], depth) * U
    empty = nval == 0
    assert bool((got[empty] == 0).all()), f"{what}: an all-padding partial is not exactly 0"
    if bool((~empty).any()):
        ratio = ((got - want).abs()[~empty] / bound[~empty]).max()
        lo._note(stats, "loss", ratio)
        assert float(ratio) <= 1.0, (f"{what}: loss partial off by {float(ratio):.2f} x the "
                                     f"tight bound: got {got.tolist()[:6]} want "
                                     f"{want.tolist()[:6]}")


# ---- cases ----------------------------------------------------------------------------------

def wide_case(rows: int, n_cls: int, seed: int) -> dict:
    """lo.logits_case plus the edge rows (e) and (f) of the module docstring (rows 4 and 5,
    where there are more than 6 rows: lo keeps the last row of a short case as padding)."""
    case = lo.logits_case(rows, n_cls, seed)
    if rows > 6 and n_cls > 256:
        x, lab = case["x"], case["labels"]
        x[4, n_cls - 1], lab[4] = 130.0, n_cls - 1
        x[5, 256], lab[5] = 30.0, 0
        assert float(x[4, :n_cls - 1].max()) <= 10.0 and float(x[5].max()) == 30.0
    return case


# ---- runners --------------------------------------------------------------------------------

def _view(rows, cols, dtype, fill, dev, layout, data=None):
    """(buffer, [rows][cols] view): ``plain`` contiguous (16-byte aligned rows where cols % 4
    == 0), ``padded`` lo's view at (PAD, PAD) of a larger buffer, ``shifted`` columns 1.. of a
    [rows][cols + 1] buffer -- base and rows off every 8- and 16-byte boundary."""
    if layout == "padded":
        return padded(rows, cols, dtype, fill, dev, data)
    off = 1 if layout == "shifted" else 0
    buf = torch.full((rows, cols + off), fill, dtype=dtype)
    if data is not None:
        buf[:, off:] = data.to(dtype)
    buf = buf.to(dev)
    return buf, buf[:, off:]


def run_softmax_xent(case, width, scale, dev, layout="padded", colsum=True, loss=True,
                     correct=True):
    """ops.softmax_xent on the given layout: NaN in the logit columns >= n_cls and around the
    view, sentinels around every output. Returns the outputs on the CPU after checking that
    nothing outside the views was written."""
    rows, n_cls = case["rows"], case["n_cls"]
    what = f"softmax_xent {rows}x{width} cls={n_cls} {layout}"
    data = torch.full((rows, width), lo.NAN)
    data[:, :n_cls] = case["x"].float()
    _, lg = _view(rows, width, torch.float32, lo.NAN, dev, layout, data)
    buf, dz = _view(rows, width, torch.bfloat16, SENTINEL, dev, layout)
    nb = ops.xent_blocks(rows)
    lp = torch.full((nb + 1,), SENTINEL, dtype=torch.float32, device=dev) if loss else None
    co = torch.full((nb + 1,), lo.ISENT, dtype=torch.int32, device=dev) if correct else None
    cs = torch.full((nb + 1, width + PAD), SENTINEL, dtype=torch.float32, device=dev) \
        if colsum else None
    ops.softmax_xent(lg, case["labels"].to(dev), dz, n_cls, scale, lp, co, colsum=cs)
    out = dict(dz=dz.detach().to(CPU).clone(), nb=nb, what=what)
    if layout == "padded":
        assert_padding_untouched(buf, rows, width, what=what)
    elif layout == "shifted":
        assert bool((buf.to(CPU)[:, 0] == SENTINEL).all()), f"{what}: wrote in front of dz"
    if loss:
        out["loss"] = lp.to(CPU)
        assert float(out["loss"][nb]) == SENTINEL, f"{what}: loss_part written past the end"
    if correct:
        out["corr"] = co.to(CPU)
        assert int(out["corr"][nb]) == lo.ISENT, f"{what}: correct written past the end"
    if colsum:
        out["cs"] = cs.to(CPU)
        assert bool((out["cs"][nb:] == SENTINEL).all()) and \
            bool((out["cs"][:, width:] == SENTINEL).all()), f"{what}: colsum wrote outside"
    return out


def judge_softmax_xent(out, case, width, scale, stats=None, depth=None):
    """The tight comparators (and lo's for colsum / correct) on the outputs of one launch."""
    ref = lo.xent_ref(case["x"], case["labels"], scale)
    nb, what = out["nb"], out["what"]
    own = lo.owners(case["rows"], lo.XENT_BLOCK_ROWS)
    assert_dz_tight(out["dz"], ref, width, stats, what, depth)
    if "loss" in out:
        assert_loss_partials_tight(out["loss"], ref, own, nb, stats, what, depth)
    if "corr" in out:
        lo.assert_correct_partials(out["corr"], ref, own, nb, what=what)
    if "cs" in out:
        lo.assert_colsum_partials(out["cs"][:, :width], out["dz"], own, nb, stats, what)
    return ref


def check_softmax_xent(case, width, scale, dev, stats=None, depth=None, lo_stats=None, **outs):
    """One case through lo's comparators (lo.check_softmax_xent, unmodified, with its sentinel
    checks; worst ratios into ``lo_stats``) and through the tight ones (``stats``)."""
    lo.check_softmax_xent(case, width, scale, dev, stats=lo_stats, **outs)
    out = run_softmax_xent(case, width, scale, dev, "padded", **outs)
    judge_softmax_xent(out, case, width, scale, stats, depth)
    return out


def run_softmax_rows(case, dev, out=True, labels=True, pred=True, inplace=False, base=lo.ISENT):
    """ops.softmax_rows from a NaN-padded view; ``inplace``: out is the logits view itself.
    Returns (probabilities or None, pred or None, correct counter) on the CPU."""
    rows, n_cls = case["rows"], case["n_cls"]
    what = f"softmax_rows {rows} cls={n_cls} inplace={inplace}"
    lbuf, lg = padded(rows, n_cls, torch.float32, lo.NAN, dev, case["x"].float())
    if inplace:
        obuf, o = lbuf, lg
    else:
        obuf, o = padded(rows, n_cls, torch.float32, SENTINEL, dev) if out else (None, None)
    lab = case["labels"].to(dev) if labels else None
    pr = torch.full((rows + 1,), lo.ISENT, dtype=torch.int32, device=dev) if pred else None
    co = torch.full((1,), base, dtype=torch.int32, device=dev)
    ops.softmax_rows(lg, o, n_cls, lab, pr, co)
    if o is not None:  # NaN != NaN: the in-place buffer is compared through nan_to_num
        fill = -7.0 if inplace else SENTINEL
        b = torch.nan_to_num(obuf.to(CPU), nan=-7.0) if inplace else obuf
        assert_padding_untouched(b, rows, n_cls, fill=fill, what=what)
    if pred:
        assert int(pr[rows]) == lo.ISENT, f"{what}: pred written past the last row"
    return (o.detach().to(CPU).clone() if o is not None else None,
            pr.to(CPU)[:rows].long() if pred else None, int(co[0]))


def check_softmax_rows(case, dev, stats=None, depth=None, **kw):
    """lo.check_softmax_rows (where its signature covers the variant) and the tight bound."""
    if not kw.get("inplace"):
        lo.check_softmax_rows(case, dev, **{k: v for k, v in kw.items()
                                            if k in ("out", "labels", "pred")})
    ref = lo.xent_ref(case["x"], case["labels"], 1.0)
    base = kw.get("base", lo.ISENT)
    p, pr, co = run_softmax_rows(case, dev, **kw)
    what = f"softmax_rows {case['rows']} cls={case['n_cls']} {kw}"
    if p is not None:
        assert_probs_tight(p, ref, stats, what, depth)
    if pr is not None:
        assert torch.equal(pr, ref["argmax"]), f"{what}: argmax"
    hits = int((ref["argmax"] == case["labels"].long()).sum()) if kw.get("labels", True) else 0
    assert co == base + hits, f"{what}: correct {co} != {base} + {hits}"


# ---- mutants of the oracle ------------------------------------------------------------------

MUTANTS = ("drop_chunk", "max_first_256", "last_tie", "no_onehot_beyond_256", "pad_col_nonzero",
           "colsum_unrounded")


def oracle_outputs(case, width, scale, mutant=None):
    """The outputs of softmax_xent computed in fp64 from the oracle's own formulae (dz rounded
    once to bf16), with one deliberate mistake when ``mutant`` names it:
      drop_chunk            the row sum misses columns 256..319 (one 64-column chunk)
      max_first_256         maximum and argmax taken over the first 256 columns only
      last_tie              argmax by the HIGHEST column holding the maximum
      no_onehot_beyond_256  the label's one-hot dropped when label >= 256
      pad_col_nonzero       dz column n_cls (a padding column) holds a stray value
      colsum_unrounded      column sums of the fp64 dz instead of the stored bf16 dz"""
    assert mutant is None or mutant in MUTANTS, mutant
    rows, n_cls = case["rows"], case["n_cls"]
    x = case["x"].double()
    lab = case["labels"].long()
    valid, safe = lab >= 0, lab.clamp_min(0)
    idx = torch.arange(n_cls).expand(rows, n_cls)
    seen = x[:, :256] if mutant == "max_first_256" else x
    mx = seen.max(1, keepdim=True).values
    hit = seen == mx
    ids = idx[:, :seen.shape[1]]
    if mutant == "last_tie":
        argmax = torch.where(hit, ids, torch.full_like(ids, -1)).max(1).values
    else:
        argmax = torch.where(hit, ids, torch.full_like(ids, n_cls)).min(1).values
    e = torch.exp(x - mx)
    summed = e.clone()
    if mutant == "drop_chunk":
        summed[:, 256:320] = 0.0
    se = summed.sum(1, keepdim=True)
    onehot = torch.zeros_like(x)
    onehot[torch.arange(rows), safe] = 1.0
    if mutant == "no_onehot_beyond_256":
        onehot[:, 256:] = 0.0
    g = (e / se - onehot) * float(scale)
    g[~valid] = 0.0
    dz64 = torch.zeros(rows, width, dtype=torch.float64)
    dz64[:, :n_cls] = g
    if mutant == "pad_col_nonzero" and width > n_cls:
        dz64[rows // 2, n_cls] = 2.0 ** -20
    dz = rn_bf16(dz64)
    nll = (mx + torch.log(se))[:, 0] - x[torch.arange(rows), safe]
    nll = torch.where(valid, nll, torch.zeros_like(nll))
    own = lo.owners(rows, lo.XENT_BLOCK_ROWS)
    nb = int(own.max()) + 1
    loss = torch.zeros(nb, dtype=torch.float64).index_add_(0, own, nll)
    corr = torch.zeros(nb, dtype=torch.int64).index_add_(0, own,
                                                         ((argmax == lab) & valid).long())
    src = dz64 if mutant == "colsum_unrounded" else dz.double()
    cs = torch.zeros(nb, width, dtype=torch.float64).index_add_(0, own, src)
    return dict(dz=dz, loss=loss, corr=corr, cs=cs, nb=nb,
                what=f"oracle {rows}x{width} cls={n_cls} mutant={mutant}")
