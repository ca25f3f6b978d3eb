"""The four softmax cross-entropy implementations -- softmax_xent_kernel<1|4>, the xent_rows
epilogue of ops.linear_fwd_xent (64- and 128-row tiles), the softmax block of the fused
classifier tail, softmax_rows_kernel<1|4> -- each against the fp64 oracle of
tests/_loss_oracle.py: exact logits, saturated and tied rows, padding rows / columns / weights
that must reach nothing, and loss / correct / colsum compared PER PARTIAL."""
import pytest
import torch

import _loss_oracle as lo
from docker_dist_nn_amd import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("width,n_cls", lo.XENT_SHAPES)
def test_softmax_xent_fp64(dev, width, n_cls):
    stats = lo.new_stats()
    for rows in lo.XENT_ROWS:  # 300: a partial last block behind an all-padding one
        case = lo.logits_case(rows, n_cls, seed=rows + n_cls)
        for scale in (1.0, 1.0 / rows):
            lo.check_softmax_xent(case, width, scale, dev, stats=stats)
        lo.check_softmax_xent(case, width, 1.0 / rows, dev, colsum=False, stats=stats)
        lo.check_softmax_xent(case, width, 1.0, dev, loss=False, correct=False, stats=stats)
    print("\n" + lo.statline(f"gpu softmax_xent {width}/{n_cls}", stats))


@pytest.mark.parametrize("M,Np,K,n_cls", lo.GEMM_SHAPES + [(16384, 64, 64, 10)])
def test_linear_fwd_xent_fp64(dev, M, Np, K, n_cls):
    """Rows n_cls..Np of w (and of the bias) hold non-zero values: the padding columns of dz
    come back zero, and every output is bitwise what it is with zero padding weights."""
    stats = lo.new_stats()
    bm = ops.xent_tiles(M, Np)[0]
    assert bm == (128 if M == 16384 else 64)  # the large case selects the 128-row tile
    case = lo.gemm_case(M, Np, K, n_cls, seed=M + K + n_cls, blk=bm)
    out = lo.check_linear_fwd_xent(case, 1.0 / M, dev, stats)
    bare = lo.gemm_case(M, Np, K, n_cls, seed=M + K + n_cls, blk=bm, pad_weights=False)
    assert torch.equal(bare["z"], case["z"])
    ref = lo.run_linear_fwd_xent(bare, 1.0 / M, dev)
    for k in ("dz", "loss", "corr", "cs"):
        assert torch.equal(out[k], ref[k]), k
    print("\n" + lo.statline(f"gpu linear_fwd_xent {M}x{Np}x{K}/{n_cls}", stats))


@pytest.mark.parametrize("rows,k3,n3,n4,n_cls", lo.TAIL_GEOS)
def test_tail_softmax_fp64(dev, rows, k3, n3, n4, n_cls):
    """dz4, loss, correct and cs4 of ops.mlp_tail against the oracle evaluated from the
    kernel's own stored h3; relu/relu is the 16-wave instantiation, the others the 8-wave one."""
    stats = lo.new_stats()
    acts = ("relu", "linear", "sigmoid") if (rows, n_cls) == (144, 10) else ("relu", "linear")
    for act3 in acts:
        act2 = "relu" if act3 == "sigmoid" else act3
        case = lo.tail_case(rows, k3, n3, n4, n_cls, act3, act2, seed=rows + k3 + n_cls)
        lo.check_tail(case, 1.0 / rows, dev, stats)
    print("\n" + lo.statline(f"gpu mlp_tail {rows}x{k3}x{n3}x{n4}/{n_cls}", stats))


@pytest.mark.parametrize("n_cls", lo.ROWS_CLS)
def test_softmax_rows_fp64(dev, n_cls):
    stats = lo.new_stats()
    for rows in lo.ROWS_ROWS:
        case = lo.logits_case(rows, n_cls, seed=3 * rows + n_cls)
        lo.check_softmax_rows(case, dev, stats=stats)
    lo.check_softmax_rows(case, dev, out=False)
    lo.check_softmax_rows(case, dev, labels=False)
    lo.check_softmax_rows(case, dev, pred=False)
    print("\n" + lo.statline(f"gpu softmax_rows /{n_cls}", stats))
