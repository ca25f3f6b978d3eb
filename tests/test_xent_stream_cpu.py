"""CPU side of the logits-free wide cross-entropy: the reference path of
ops.linear_xent_stream against the fp64 oracle, and when LossHead.choose takes StreamXentHead."""
import pytest
import torch

import _loss_oracle as lo
from docker_dist_nn_amd import MLPSpec, ops, switches
from docker_dist_nn_amd.engine import Trainer
from docker_dist_nn_amd.engine.loss_head import FusedXentHead, StreamXentHead, XentHead

CPU = torch.device("cpu")


@pytest.mark.parametrize("M,Np,n_cls,K", [(192, 192, 130, 128), (128, 1088, 1025, 64)])
def test_cpu_path_matches_the_oracle(M, Np, n_cls, K):
    case, scale, nb = lo.gemm_case(M, Np, K, n_cls, 7), 1.0 / M, M // 64
    dz = torch.full((M, Np), lo.SENTINEL, dtype=torch.bfloat16)
    lp, co, cs = torch.zeros(nb), torch.zeros(nb, dtype=torch.int32), torch.zeros(nb, Np)
    ops.linear_xent_stream(case["x"], case["w"], case["bias"], dz, case["labels"], n_cls, scale,
                           lp, co, colsum=cs)
    ref, own = lo.xent_ref(case["z"], case["labels"], scale), lo.owners(M, 64)
    lo.assert_dz(dz, ref, Np, what="cpu")
    lo.assert_loss_partials(lp, ref, own, nb, what="cpu")
    lo.assert_correct_partials(co, ref, own, nb, what="cpu")
    lo.assert_colsum_partials(cs, dz, own, nb, what="cpu")


@pytest.mark.parametrize("widths,stream,head", [
    ([128, 64, 300], "0", XentHead), ([128, 64, 300], "1", StreamXentHead),
    ([128, 64, 10], "1", FusedXentHead), ([128, 64, 100], "1", FusedXentHead),
    ([128, ops.XENT_STREAM_MAX_K + 64, 300], "1", XentHead)])
def test_head_choice(monkeypatch, widths, stream, head):
    monkeypatch.setenv("DNN_XENT_STREAM", stream)
    tr = Trainer(MLPSpec.from_widths(widths), device=CPU, micro_batch=64, num_micro=1)
    assert type(tr.last.head) is head
    assert tr.last.acts[-1].shape[0] == (64 if head is XentHead else 0)


def test_switch_defaults_to_off(monkeypatch):
    monkeypatch.delenv("DNN_XENT_STREAM", raising=False)
    assert switches.get("DNN_XENT_STREAM") == "0" == switches.SWITCHES["DNN_XENT_STREAM"][0]
    assert not ops.xent_stream_supported(ops.XENT_STREAM_MAX_K + 64, 320)
    assert ops.xent_stream_supported(ops.XENT_STREAM_MAX_K, 320) and ops.XENT_STREAM_MAX_K >= 1024
