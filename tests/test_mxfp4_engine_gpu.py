"""``InferenceEngine(weights="mxfp4")`` on the GPU: a 64-128-24 model at buckets of 1, 8, 9 and
100 rows, eager and under HIP-graph replay, against the exact oracle of the format
(_mxfp4_oracle.py) and the bounds of _gemv_mxfp4_cases.py."""
import numpy as np
import pytest
import torch

import _gemv_mxfp4_cases as gc
import _mxfp4_oracle as mo
from docker_dist_nn_amd.config import LayerWeights
from docker_dist_nn_amd.engine.inference import InferenceEngine

pytestmark = pytest.mark.gpu

DIMS = [64, 128, 24]
ACTS = ("relu", "linear")
BUCKETS = (1, 8, 9, 100)


def _layers():
    rng = np.random.default_rng(64128)
    return [LayerWeights(rng.standard_normal((DIMS[i + 1], DIMS[i])) / np.sqrt(DIMS[i]),
                         rng.standard_normal(DIMS[i + 1]) * 0.1, ACTS[i]) for i in range(2)]


def _inputs(rows):
    return np.random.default_rng(rows).standard_normal((rows, 64))


@pytest.fixture(scope="module")
def engines(dev):
    """(eager mxfp4 engine, graph mxfp4 engine, bf16 engine on the dequantised weights, the
    dequantised fp64 weights and biases), built once."""
    L = _layers()
    eager = InferenceEngine([L], dev, expected_input=64, weights="mxfp4", use_graphs=False)
    graph = InferenceEngine([L], dev, expected_input=64, weights="mxfp4", use_graphs=True)
    st = eager.stages[0]
    deq, w64 = [], []
    for i in range(2):
        d = mo.dequant_ref(st.q4[i].cpu().numpy(), st.e4[i].cpu().numpy())
        w64.append(d.double().numpy()[:DIMS[i + 1], :DIMS[i]])
        deq.append(LayerWeights(d.float().numpy()[:DIMS[i + 1], :DIMS[i]], L[i].bias, ACTS[i]))
    bf = InferenceEngine([deq], dev, expected_input=64, use_graphs=False)
    return eager, graph, bf, w64, [np.asarray(l.bias, np.float32).astype(np.float64) for l in L]


def test_stage_holds_the_oracle_quantisation_and_no_bf16_weight(dev, engines):
    eager, _, _, _, _ = engines
    st, L = eager.stages[0], _layers()
    assert not st.w and not st.q and not st.s
    for i in range(2):
        w = torch.zeros(st.pads[i + 1], st.pads[i])
        w[:DIMS[i + 1], :DIMS[i]] = torch.as_tensor(np.asarray(L[i].weight, np.float32))
        q, e, _ = mo.quant_ref(w.to(torch.bfloat16))
        assert np.array_equal(st.q4[i].cpu().numpy(), q)
        assert np.array_equal(st.e4[i].cpu().numpy(), e)
    n = sum(a * b for a, b in zip(st.pads, st.pads[1:]))
    assert eager.resident_weight_bytes() == n // 2 + n // 32


@pytest.mark.parametrize("rows", BUCKETS)
def test_eager_and_graph_replay_give_the_same_bits(engines, rows):
    eager, graph, _, _, _ = engines
    x = _inputs(rows)
    want = eager.predict(x)
    assert want.shape == (rows, 24) and np.isfinite(want).all()
    for _ in range(3):  # warm-up run, capture, replay
        assert np.array_equal(graph.predict(x), want), f"rows={rows}"


@pytest.mark.parametrize("rows", (9, 100))
def test_large_buckets_equal_bf16_engine_on_dequantised_weights(engines, rows):
    """Dequantisation into the scratch is exact, so the bucket answers bit for bit as a bf16
    engine loaded with dequant_ref(q, e)."""
    eager, graph, bf, _, _ = engines
    x = _inputs(rows)
    want = bf.predict(x)
    assert np.array_equal(eager.predict(x), want) and np.array_equal(graph.predict(x), want)


@pytest.mark.parametrize("rows", (1, 8))
def test_serving_sizes_within_the_propagated_summation_bound(engines, rows):
    """Against the fp64 forward on the DEQUANTISED weights (what the codes mean): layer 1 is
    off by its summation bound and one rounding to bf16 (2^-8 relative, spare included), ReLU
    does not widen that, and layer 2 carries it through |W2| and adds its own summation bound
    (gc.summation_bound: T = 16 products per lane, half a block, at K = 64 and at K = 128)."""
    eager, _, _, (w1, w2), (b1, b2) = engines
    x = _inputs(rows)
    xb = torch.from_numpy(x).float().to(torch.bfloat16).double().numpy()  # pack_bf16 of fp32(x)
    z1 = xb @ w1.T + b1
    e1 = gc.summation_bound(64, rows, np.abs(xb) @ np.abs(w1).T, b1)
    h1 = np.maximum(z1, 0.0)
    e1 = e1 + 2.0 ** -8 * (h1 + e1)
    z2 = h1 @ w2.T + b2
    e2 = e1 @ np.abs(w2).T + gc.summation_bound(128, rows, (h1 + e1) @ np.abs(w2).T, b2)
    ratio = float((np.abs(eager.predict(x) - z2) / e2).max())
    print(f"\nmxfp4 engine rows={rows}: error at {ratio:.3f} x the propagated bound")
    assert ratio <= 1.0


@pytest.mark.parametrize("N,K,M", gc.LAYERS)
def test_one_layer_within_format_bound(dev, N, K, M):
    """One linear layer at a serving size against the fp64 product with the ORIGINAL bf16
    weights: within the format's per-weight bound summed against |x| plus the summation bound."""
    w, b, x = gc.layer_case(N, K, M)
    eng = InferenceEngine([[LayerWeights(w.float().numpy(), b.numpy(), "linear")]], dev,
                          expected_input=K, weights="mxfp4")
    ratio = gc.check_layer(eng.predict(x.float().numpy()), w, b, x)
    print(f"\nmxfp4 one-layer predict {M}x{N}x{K}: error at {ratio:.3f} x the bound")


def test_weight_operand_raises(engines):
    with pytest.raises(ValueError, match="mxfp4"):
        engines[0].stages[0].weight_operand(0)
