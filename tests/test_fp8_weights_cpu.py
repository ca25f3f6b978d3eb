"""fp8 serving weights without a GPU: the accuracy of the format on weights, the CPU reference
of ops.gemv_fp8 against the exact oracle, ``InferenceEngine(weights="fp8")`` on the CPU device
and the command-line flag. Operands and bounds in _gemv_fp8_cases.py."""
import numpy as np
import pytest
import torch

import _fp8_oracle as fo
import _gemv_fp8_cases as gc
from test_gemv_gpu import SIGMOID_F32_MAX_ULP
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.config import LayerWeights, load_model_config
from docker_dist_nn_amd.engine.inference import InferenceEngine, InferenceStage
from docker_dist_nn_amd.ops import reference as ref

CPU = torch.device("cpu")
DIMS = [40, 24, 10]
MODELS = {"relu": ("relu", "linear"), "sigmoid": ("sigmoid", "sigmoid")}


def test_reference_decode_table_is_the_oracles():
    got, want = ref.e4m3_table().numpy(), fo.DEC
    assert np.array_equal(np.isnan(got), np.isnan(want))
    finite = np.isfinite(want)
    assert np.array_equal(got[finite].view(np.int64), want[finite].view(np.int64))


def test_format_accuracy_on_weights():
    """|s * dec(q) - w| within the per-element bound of the format for a 24 x 64 random bf16
    matrix (gc.format_bound)."""
    w, _, _ = gc.one_layer_case()
    q, s, _ = fo.quant_ref(w)
    err = np.abs(s.astype(np.float64)[:, None] * fo.DEC[q] - w.double().numpy())
    ratio = float((err / gc.format_bound(w.double().numpy())).max())
    print(f"\nfp8 weight format: worst error at {ratio:.3f} x the bound")
    assert 0.5 < ratio <= 1.0  # the bound is met and is not slack


def test_one_layer_stage_within_format_bound():
    """The stage's serving-size path (ops.gemv_fp8's CPU reference) at 1 row against the fp64
    product with the original bf16 weights."""
    w, b, x = gc.one_layer_case()
    st = InferenceStage([LayerWeights(w.float().numpy(), b.numpy(), "linear")], CPU,
                        expected_input=64, weights="fp8")
    st.buffers(1)["x"].copy_(x)
    y = st.forward(1)[:, :24].double().numpy()
    gc.check_one_layer(y, w, b, x)


@pytest.mark.parametrize("N,K", gc.NK)
def test_gemv_fp8_cpu_reference_equals_oracle(N, K):
    """ops.gemv_fp8 on CPU tensors: linear / relu exact, sigmoid (torch's fp32 sigmoid) within
    the GPU kernel's bounds."""
    gc.check_exact_shape(ops.gemv_fp8, N, K, CPU, SIGMOID_F32_MAX_ULP)


def _layers(acts):
    rng = np.random.default_rng(len(acts[0]))
    return [LayerWeights(rng.standard_normal((DIMS[i + 1], DIMS[i])) / np.sqrt(DIMS[i]),
                         rng.standard_normal(DIMS[i + 1]) * 0.1, acts[i]) for i in range(2)]


@pytest.mark.parametrize("model", sorted(MODELS))
def test_cpu_engine_fp8(model):
    """On the CPU device: codes and scales equal the oracle's, no bf16 weight is kept, and
    predict at 9 and 64 rows equals a bf16 engine on dequant_ref(q, s) bit for bit."""
    L = _layers(MODELS[model])
    eng = InferenceEngine([L], CPU, expected_input=40, weights="fp8")
    st = eng.stages[0]
    assert not getattr(st, "w", None)
    deq = []
    for i in range(2):
        w = torch.zeros(64, 64)
        w[:L[i].out_dim, :L[i].in_dim] = torch.as_tensor(np.asarray(L[i].weight, np.float32))
        q, s, _ = fo.quant_ref(w.to(torch.bfloat16))
        assert np.array_equal(st.q[i].numpy(), q)
        assert np.array_equal(fo.bits32(st.s[i]), fo.bits32(s))
        d = fo.dequant_ref(q, s).float().numpy()
        deq.append(LayerWeights(d[:DIMS[i + 1], :DIMS[i]], L[i].bias, L[i].activation))
    bf = InferenceEngine([deq], CPU, expected_input=40)
    for rows in (9, 64):
        x = np.random.default_rng(rows).standard_normal((rows, 40))
        assert np.array_equal(eng.predict(x), bf.predict(x)), f"{model} rows={rows}"


def test_unknown_weight_format_raises():
    with pytest.raises(ValueError):
        InferenceEngine([_layers(MODELS["relu"])], CPU, expected_input=40, weights="int4")
    with pytest.raises(ValueError):
        InferenceStage(_layers(MODELS["relu"]), CPU, expected_input=40, weights="int4")


def test_command_line_takes_weights(tmp_path):
    """run_grpc_fcnn.py --mode local --device cpu --weights fp8 --no-serve sets up; an engine
    built as local mode builds it answers a request; run_grpc_inference.py takes the flag."""
    from docker_dist_nn_amd.cli import fcnn, inference
    from docker_dist_nn_amd.data import write_examples
    from docker_dist_nn_amd.weights_io import export_model_json

    rng = np.random.default_rng(0)
    dims = [48, 32, 10]
    ws = [rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i]) for i in range(2)]
    bs = [rng.standard_normal(dims[i + 1]) * 0.1 for i in range(2)]
    cfg, inp = tmp_path / "model.json", tmp_path / "inputs.json"
    export_model_json(str(cfg), ws, bs, ["relu", "softmax"], layer_distribution=[1, 1])
    x = rng.random((4, 48))
    write_examples(str(inp), x, np.zeros(4, dtype=np.int64))
    argv = ["--config", str(cfg), "--inputs", str(inp), "--mode", "local", "--device", "cpu",
            "--cache-dir", str(tmp_path / "cache"), "--no-serve"]
    assert fcnn.build_parser(str(tmp_path)).parse_args(argv).weights == "bf16"
    assert fcnn.build_parser(str(tmp_path)).parse_args(argv + ["--weights", "fp8"]).weights == "fp8"
    with pytest.raises(SystemExit):
        fcnn.build_parser(str(tmp_path)).parse_args(argv + ["--weights", "int4"])
    assert fcnn.main(argv + ["--weights", "fp8"], script_dir=str(tmp_path)) == 0
    a = inference.build_parser(str(tmp_path)).parse_args(["--local", str(cfg), "--weights", "fp8"])
    assert a.weights == "fp8"
    mc = load_model_config(str(cfg))
    eng = InferenceEngine([mc.layers[:1], mc.layers[1:]], CPU, expected_input=48,
                          names=["layer_container_0", "layer_container_1"], weights=a.weights)
    out = eng.predict(x)
    assert out.shape == (4, 10) and np.isfinite(out).all()
    np.testing.assert_allclose(out.sum(1), 1.0, atol=1e-5)  # a softmax row
