"""The fp64 softmax cross-entropy oracle (tests/_loss_oracle.py) checked without a GPU: its
reference on hand-made values, its case generators and comparators run through the CPU path of
the same public ops the GPU tests call (ops.softmax_xent / ops.linear_fwd_xent / ops.mlp_tail /
ops.softmax_rows), and a set of deliberately wrong implementations it must reject."""
import math

import pytest
import torch

import _loss_oracle as lo

CPU = torch.device("cpu")


def test_reference_on_hand_values():
    x = torch.tensor([[0.0, 0.0], [3.0, 3.0], [200.0, -200.0], [-200.0, 200.0], [1.0, 2.0]],
                     dtype=torch.float64)
    lab = torch.tensor([0, 1, 1, 1, -1], dtype=torch.int32)
    r = lo.xent_ref(x, lab, 0.5)
    assert r["argmax"].tolist() == [0, 0, 0, 1, 1]
    assert r["correct"].tolist() == [True, False, False, True, False]
    assert r["loss"].tolist() == pytest.approx([math.log(2.0), math.log(2.0), 400.0, 0.0, 0.0],
                                               rel=1e-15, abs=1e-300)
    assert r["dz"].flatten().tolist() == pytest.approx(
        [-0.25, 0.25, 0.25, -0.25, 0.5, -0.5, 0.0, 0.0, 0.0, 0.0], rel=1e-15, abs=1e-100)
    assert lo.owners(40, 16, 2).tolist() == [0] * 16 + [1] * 16 + [0] * 8


@pytest.mark.parametrize("width,n_cls", lo.XENT_SHAPES)
def test_softmax_xent_cases_on_cpu_path(width, n_cls):
    stats = lo.new_stats()
    for rows in lo.XENT_ROWS:
        case = lo.logits_case(rows, n_cls, seed=rows + n_cls)
        for scale in (1.0, 1.0 / rows):
            lo.check_softmax_xent(case, width, scale, CPU, stats=stats)
        lo.check_softmax_xent(case, width, 1.0 / rows, CPU, colsum=False, stats=stats)
        lo.check_softmax_xent(case, width, 1.0, CPU, loss=False, correct=False, stats=stats)
    print("\n" + lo.statline(f"cpu softmax_xent {width}/{n_cls}", stats))


@pytest.mark.parametrize("M,Np,K,n_cls", lo.GEMM_SHAPES + [(16384, 64, 64, 10)])
def test_linear_fwd_xent_cases_on_cpu_path(M, Np, K, n_cls):
    stats = lo.new_stats()
    blk = lo.ops.xent_tiles(M, Np)[0]
    case = lo.gemm_case(M, Np, K, n_cls, seed=M + K + n_cls, blk=blk)
    out = lo.check_linear_fwd_xent(case, 1.0 / M, CPU, stats)
    bare = lo.gemm_case(M, Np, K, n_cls, seed=M + K + n_cls, blk=blk, pad_weights=False)
    assert torch.equal(bare["z"], case["z"])
    ref = lo.run_linear_fwd_xent(bare, 1.0 / M, CPU)
    for k in ("dz", "loss", "corr", "cs"):  # the padding weights reach nothing
        assert torch.equal(out[k], ref[k]), k
    print("\n" + lo.statline(f"cpu linear_fwd_xent {M}x{Np}x{K}/{n_cls}", stats))


@pytest.mark.parametrize("rows,k3,n3,n4,n_cls", lo.TAIL_GEOS)
def test_tail_cases_on_cpu_path(rows, k3, n3, n4, n_cls):
    stats = lo.new_stats()
    acts = ("relu", "linear", "sigmoid") if (rows, n_cls) == (144, 10) else ("relu", "linear")
    for act3 in acts:
        act2 = "relu" if act3 == "sigmoid" else act3
        case = lo.tail_case(rows, k3, n3, n4, n_cls, act3, act2, seed=rows + k3 + n_cls)
        lo.check_tail(case, 1.0 / rows, CPU, stats)
    print("\n" + lo.statline(f"cpu mlp_tail {rows}x{k3}x{n3}x{n4}/{n_cls}", stats))


@pytest.mark.parametrize("n_cls", lo.ROWS_CLS)
def test_softmax_rows_cases_on_cpu_path(n_cls):
    stats = lo.new_stats()
    for rows in lo.ROWS_ROWS:
        case = lo.logits_case(rows, n_cls, seed=3 * rows + n_cls)
        lo.check_softmax_rows(case, CPU, stats=stats)
    lo.check_softmax_rows(case, CPU, out=False)
    lo.check_softmax_rows(case, CPU, labels=False)
    lo.check_softmax_rows(case, CPU, pred=False)
    print("\n" + lo.statline(f"cpu softmax_rows /{n_cls}", stats))


# ---- the mistakes the oracle is for ---------------------------------------------------------

def _plain(case, width, scale, *, no_max=False, last_tie=False, pad_cols=False, no_onehot=False,
           keep_padding_rows=False, log2=False, swap=None):
    """Plain fp32 torch softmax-CE with the comparators' output contract; each flag is one
    wrong implementation."""
    rows, n_cls = case["rows"], case["n_cls"]
    x = torch.zeros(rows, width)  # zero logits in the padding columns (a GEMM's zero weights)
    x[:, :n_cls] = case["x"].float()
    lab = case["labels"].long()
    valid, safe = lab >= 0, lab.clamp_min(0)
    xs = x if pad_cols else x[:, :n_cls]
    sh = xs if no_max else xs - xs.max(1, keepdim=True).values
    e = torch.exp(sh)
    se = e.sum(1, keepdim=True)
    g = (e / se)[:, :n_cls].clone()
    if not no_onehot:
        g[torch.arange(rows), safe] -= 1.0
    g *= scale
    if not keep_padding_rows:
        g[~valid] = 0.0
    dz = torch.zeros(rows, width, dtype=torch.bfloat16)
    dz[:, :n_cls] = g.to(torch.bfloat16)
    lse = (torch.log2(se) if log2 else torch.log(se))[:, 0]
    nll = torch.where(valid, lse - sh[torch.arange(rows), safe], torch.zeros(rows))
    xc = x[:, :n_cls]
    am = (n_cls - 1 - torch.argmax(xc.flip(1), 1)) if last_tie else \
        lo.xent_ref(xc, lab, 1.0)["argmax"]
    own = lo.owners(rows, 64)
    nb = int(own.max()) + 1
    loss = torch.zeros(nb).index_add_(0, own, nll)
    corr = torch.zeros(nb, dtype=torch.int64).index_add_(0, own, ((am == lab) & valid).long())
    if swap:
        loss[list(swap)] = loss[list(reversed(swap))]
    return dz, loss, corr, own, nb


def _judge(case, width, scale, **mut):
    dz, loss, corr, own, nb = _plain(case, width, scale, **mut)
    ref = lo.xent_ref(case["x"], case["labels"], scale)
    lo.assert_dz(dz, ref, width)
    lo.assert_loss_partials(loss, ref, own, nb)
    lo.assert_correct_partials(corr, ref, own, nb)


def test_oracle_catches_the_mistakes_it_is_for():
    """Each wrong softmax-CE must fail the comparators on the standard cases; the right one
    passes them."""
    cases = [(lo.logits_case(300, 10, seed=1), 64), (lo.logits_case(300, 100, seed=2), 128)]
    mutants = [dict(no_max=True), dict(last_tie=True), dict(pad_cols=True),
               dict(no_onehot=True), dict(keep_padding_rows=True), dict(log2=True),
               dict(swap=(0, 2))]
    for case, width in cases:
        for scale in (1.0, 1.0 / 300):
            _judge(case, width, scale)
            for mut in mutants:
                with pytest.raises(AssertionError):
                    _judge(case, width, scale, **mut)
    # the tie rule alone: rows (a) and (b) are the first it changes
    case = lo.logits_case(300, 10, seed=1)
    ref = lo.xent_ref(case["x"], case["labels"], 1.0)
    last = 9 - torch.argmax(case["x"].flip(1), 1)
    assert (last != ref["argmax"]).nonzero().flatten().tolist()[:2] == [0, 1]
