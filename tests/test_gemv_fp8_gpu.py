"""The fp8-weight serving GEMV (csrc/kernels/gemv_fp8.hip, ops.gemv_fp8) and the engine's
``weights="fp8"`` on the GPU, against the exact oracles of _fp8_oracle.py (the format) and
_act_oracle.py (the activations): operands and method in _gemv_fp8_cases.py."""
import numpy as np
import pytest
import torch

import _act_oracle as ao
import _fp8_oracle as fo
import _gemv_fp8_cases as gc
from test_gemv_gpu import SIGMOID_F32_MAX_ULP
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.config import LayerWeights
from docker_dist_nn_amd.engine.inference import InferenceEngine

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,K", gc.NK)
def test_gemv_fp8_equals_fp64_oracle(dev, N, K):
    """M = 1..8, every activation, fp32 and bf16 output, bias (longer than N) and None. fp32:
    linear / relu bit-equal to fp64, sigmoid within SIGMOID_F32_MAX_ULP of test_gemv_gpu.py
    (the same act_fwd runs on an exact z, so that measured bound carries over). bf16: linear /
    relu bit-equal to RN_bf16(fp64), sigmoid within 1 bf16 ulp. Nothing outside [M][N] is
    written; NaN padding of x, q, scale and bias is never read."""
    worst = gc.check_exact_shape(ops.gemv_fp8, N, K, dev, SIGMOID_F32_MAX_ULP)
    print(f"\ngemv_fp8 N={N} K={K}: sigmoid fp32 worst {worst:.2f} ulp (bound "
          f"{SIGMOID_F32_MAX_ULP:g})")


def test_gemv_fp8_decodes_every_code(dev):
    """q[n][0] = n, x = e_0, scale 1: y[0][n] is the kernel's decode of code n. It must equal
    the oracle's table bit for bit for the 254 finite codes (code 0x80, -0, arrives as the sum
    0 + (-0) = +0 of IEEE addition) and be NaN for 0x7F and 0xFF."""
    q = torch.zeros(256, 16, dtype=torch.uint8)
    q[:, 0] = torch.arange(256, dtype=torch.uint8)
    x = torch.zeros(1, 16, dtype=torch.bfloat16)
    x[0, 0] = 1.0
    y = torch.full((1, 256), ao.SENTINEL, dtype=torch.float32, device=dev)
    ops.gemv_fp8(x.to(dev), q.to(dev), torch.ones(256, device=dev), None, y, "linear")
    got = y.cpu().numpy()[0]
    want = fo.DEC.astype(np.float32) + np.float32(0.0)
    finite = np.isfinite(fo.DEC)
    assert finite.sum() == 254 and not finite[0x7F] and not finite[0xFF]
    assert np.array_equal(fo.bits32(got[finite]), fo.bits32(want[finite]))
    assert np.isnan(got[0x7F]) and np.isnan(got[0xFF])


def test_gemv_fp8_random_operands_within_derived_bound(dev):
    """Random bf16 x and quantised random weights at 8 x 300 x 4112 against s * (x . dec(q)^T)
    + bias in fp64. dec * x is exact in fp32 (4 x 8 significant bits), so the error is that of
    the additions and the epilogue only: a lane accumulates T = 16 * ceil(K / 1024) = 80
    products (16 codes per 1024-column chunk, 5 chunks, the last on lane 0 alone), then come 6
    shuffle levels, the scale multiply, the bias add and a spare unit, each at most 2^-24 of the
    running magnitude <= s * sum_k |x_k dec_k| + |bias|:
    |y - ref| <= (T + 6 + 3) * 2^-24 * (s * sum_k |x_k dec_k| + |bias|) per output."""
    M, N, K = 8, 300, 4112
    g = torch.Generator().manual_seed(4112)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    bias = torch.randn(N, generator=g)
    q, s, _ = fo.quant_ref(w)
    deq = s.astype(np.float64)[:, None] * fo.DEC[q]
    x64, b64 = x.double().numpy(), bias.double().numpy()
    ref = x64 @ deq.T + b64
    assert gc.lane_terms(K) == 80
    bound = gc.summation_bound(K, np.abs(x64) @ np.abs(deq).T, b64)
    _, xv = ao.padded(M, K, torch.bfloat16, float("nan"), dev, x)
    ybuf, yv = ao.padded(M, N, torch.float32, ao.SENTINEL, dev)
    ops.gemv_fp8(xv, gc.padded_codes(torch.from_numpy(q), dev), torch.from_numpy(s).to(dev),
                 bias.to(dev), yv, "linear")
    ratio = float((np.abs(yv.cpu().double().numpy() - ref) / bound).max())
    print(f"\ngemv_fp8 random 8x300x4112: error at {ratio:.3f} x the derived bound")
    assert ratio <= 1.0
    ao.assert_padding_untouched(ybuf, M, N, what="gemv_fp8 random")


def test_gemv_fp8_rejects_bad_operands(dev):
    x = torch.zeros(9, 32, dtype=torch.bfloat16, device=dev)
    q = torch.zeros(4, 32, dtype=torch.uint8, device=dev)
    s = torch.ones(4, device=dev)
    y = torch.zeros(9, 4, device=dev)
    with pytest.raises(ValueError):
        ops.gemv_fp8(x, q, s, None, y)  # 9 rows
    with pytest.raises(ValueError):
        ops.gemv_fp8(x[:2, :24], q, s, None, y)  # K % 16
    with pytest.raises(ValueError):
        ops.gemv_fp8(x[:2], q, s[:3], None, y)  # scale shorter than N
    with pytest.raises(TypeError):
        ops.gemv_fp8(x[:2], q.to(torch.int8), s, None, y)
    with pytest.raises(ValueError):  # rows of codes not 16-byte aligned: the launcher's -2
        ops.gemv_fp8(x[:2, :16], torch.zeros(4, 24, dtype=torch.uint8, device=dev)[:, :16], s,
                     None, y)


# ---- engine ---------------------------------------------------------------------------------

DIMS = [40, 24, 10]
MODELS = {"relu": ("relu", "linear"), "sigmoid": ("sigmoid", "sigmoid")}


def _layers(acts):
    rng = np.random.default_rng(len(acts[0]))
    return [LayerWeights(rng.standard_normal((DIMS[i + 1], DIMS[i])) / np.sqrt(DIMS[i]),
                         rng.standard_normal(DIMS[i + 1]) * 0.1, acts[i]) for i in range(2)]


def _padded_bf16(L):
    w = torch.zeros(64, 64)
    w[:L.out_dim, :L.in_dim] = torch.as_tensor(np.asarray(L.weight, np.float32))
    return w.to(torch.bfloat16)


def _engine(acts, dev, split=False, **kw):
    L = _layers(acts)
    return InferenceEngine([L[:1], L[1:]] if split else [L], dev, expected_input=40,
                           weights="fp8", **kw)


def _all_layers(eng):
    return [(st.q[i], st.s[i], st.b[i], st.acts[i]) for st in eng.stages
            for i in range(len(st.layers))]


@pytest.mark.parametrize("model", sorted(MODELS))
def test_engine_fp8_weights_are_the_oracle_quantisation(dev, model):
    """stage.q / stage.s equal quant_ref(padded bf16 weight) bit for bit; the bf16 weight list
    is empty (one byte per weight resident)."""
    L = _layers(MODELS[model])
    eng = _engine(MODELS[model], dev)
    st = eng.stages[0]
    assert not getattr(st, "w", None)
    for i in range(2):
        q, s, _ = fo.quant_ref(_padded_bf16(L[i]))
        assert st.q[i].dtype == torch.uint8 and tuple(st.q[i].shape) == (64, 64)
        assert np.array_equal(st.q[i].cpu().numpy(), q)
        assert np.array_equal(fo.bits32(st.s[i]), fo.bits32(s))


@pytest.mark.parametrize("mode", ["eager", "graph", "native"])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_engine_fp8_serving_sizes_chain_gemv_fp8(dev, monkeypatch, model, mode):
    """predict at 1, 5 and 8 rows is bit-equal to ops.gemv_fp8 chained by hand over the stage's
    codes -- eagerly, under HIP-graph replay and under native Program replay; the sigmoid
    model as two stages (a bf16 hand-off between them)."""
    monkeypatch.setenv("DNN_SERVE_REPLAY", "native" if mode == "native" else "graph")
    eng = _engine(MODELS[model], dev, split=model == "sigmoid", use_graphs=mode != "eager")
    (q0, s0, b0, a0), (q1, s1, b1, a1) = _all_layers(eng)
    for rows in (1, 5, 8):
        x = np.random.default_rng(rows).standard_normal((rows, 40))
        xb = torch.zeros(rows, 64, dtype=torch.bfloat16, device=dev)
        ops.pack_bf16(torch.from_numpy(x).float().to(dev), xb)
        h = torch.zeros(rows, 64, dtype=torch.bfloat16, device=dev)
        f = torch.zeros(rows, 64, dtype=torch.float32, device=dev)
        ops.gemv_fp8(xb, q0, s0, b0, h, a0)
        ops.gemv_fp8(h, q1, s1, b1, f, a1)
        want = f[:, :10].double().cpu().numpy()
        for _ in range(2):  # capture / record, then replay
            assert np.array_equal(eng.predict(x), want), f"{model} {mode} rows={rows}"


@pytest.mark.parametrize("model", sorted(MODELS))
def test_engine_fp8_large_buckets_equal_bf16_engine_on_dequantised_weights(dev, model):
    """predict at 9 and 64 rows (dequantise into the scratch + the bf16 GEMM) is bit-equal to a
    bf16 engine built from dequant_ref(q, s)."""
    eng = _engine(MODELS[model], dev)
    L = _layers(MODELS[model])
    deq = []
    for i, (q, s, _, act) in enumerate(_all_layers(eng)):
        w = fo.dequant_ref(q.cpu().numpy(), s.cpu().numpy()).float().numpy()
        deq.append(LayerWeights(w[:DIMS[i + 1], :DIMS[i]], L[i].bias, act))
    ref = InferenceEngine([deq], dev, expected_input=40)
    for rows in (9, 64):
        x = np.random.default_rng(rows).standard_normal((rows, 40))
        for _ in range(2):
            assert np.array_equal(eng.predict(x), ref.predict(x)), f"{model} rows={rows}"


def test_engine_rejects_unknown_weight_format(dev):
    with pytest.raises(ValueError):
        InferenceEngine([_layers(MODELS["relu"])], dev, expected_input=40, weights="int4")


def test_engine_fp8_one_layer_within_format_bound(dev):
    """One linear layer at 1 row (the gemv_fp8 path) against the fp64 product with the ORIGINAL
    bf16 weights: within the format's per-weight bound summed against |x| plus the summation
    bound."""
    w, b, x = gc.one_layer_case()
    eng = InferenceEngine([[LayerWeights(w.float().numpy(), b.numpy(), "linear")]], dev,
                          expected_input=64, weights="fp8")
    ratio = gc.check_one_layer(eng.predict(x.float().numpy()), w, b, x)
    print(f"\nfp8 one-layer predict: error at {ratio:.3f} x the bound")
