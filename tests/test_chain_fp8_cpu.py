"""fp8 rank chains on the device-side chain, the parts that need no GPU: the stage's weight
operand accessor (what serve/fastpath.py hands to the chain kernels) and the benchmark's
``--weights`` option."""
import os
import subprocess
import sys

import numpy as np
import torch

import _fp8_oracle as fo
from docker_dist_nn_amd.config import LayerWeights
from docker_dist_nn_amd.engine.inference import InferenceStage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def _layers():
    rng = np.random.default_rng(8)
    dims = [40, 24, 10]
    return [LayerWeights(rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i]),
                         rng.standard_normal(dims[i + 1]) * 0.1, "relu") for i in range(2)]


def test_weight_operand_bf16_is_the_padded_weight():
    st = InferenceStage(_layers(), CPU, expected_input=40)
    for i in range(2):
        w, ld, shape, scale = st.weight_operand(i)
        assert w is st.w[i] and w.dtype == torch.bfloat16 and scale is None
        assert shape == (64, 64) and ld == w.stride(0) == 64


def test_weight_operand_fp8_is_codes_and_scales():
    """The codes and row scales of the oracle's quantisation of the padded bf16 weight, the row
    stride in bytes; no bf16 copy is kept."""
    L = _layers()
    st = InferenceStage(L, CPU, expected_input=40, weights="fp8")
    assert not st.w
    for i in range(2):
        q, ld, shape, scale = st.weight_operand(i)
        assert q is st.q[i] and scale is st.s[i]
        assert q.dtype == torch.uint8 and scale.dtype == torch.float32
        assert shape == (64, 64) and ld == 64 and tuple(scale.shape) == (64,)
        w = torch.zeros(64, 64)
        w[:L[i].out_dim, :L[i].in_dim] = torch.as_tensor(np.asarray(L[i].weight, np.float32))
        qr, sr, _ = fo.quant_ref(w.to(torch.bfloat16))
        assert np.array_equal(q.numpy(), qr) and np.array_equal(fo.bits32(scale), fo.bits32(sr))


def test_chain_latency_lists_the_weights_option():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench", "chain_latency.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--weights" in r.stdout and "fp8" in r.stdout
