"""fp8 activations x fp8 weights without a GPU: ops.linear_w8a8 on CPU tensors (the reference in
ops/reference.py) against the exact oracle, ``InferenceEngine(weights="fp8", fp8_gemm="w8a8")``
on the CPU device and the command-line flag. Operands in _linear_w8a8_cases.py."""
import numpy as np
import pytest
import torch

import _linear_w8a8_cases as wc
from test_gemv_gpu import SIGMOID_F32_MAX_ULP
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.config import LayerWeights
from docker_dist_nn_amd.engine.inference import FP8_GEMMS, InferenceEngine, InferenceStage

CPU = torch.device("cpu")
DIMS = [40, 24, 10]
MODELS = {"relu": ("relu", "linear"), "sigmoid": ("sigmoid", "sigmoid")}


@pytest.mark.parametrize("M,N,K", [(9, 17, 48), (65, 33, 144)])
def test_linear_w8a8_cpu_reference_equals_oracle(M, N, K):
    """ops.linear_w8a8 on CPU tensors: linear / relu exact on the exact-sum operands (both scale
    multiplies included), sigmoid (torch's fp32 sigmoid) within the GPU kernel's bound."""
    wc.check_exact(ops.linear_w8a8, M, N, K, CPU, SIGMOID_F32_MAX_ULP)


def test_linear_w8a8_cpu_rejects_bad_operands():
    xq = torch.zeros(9, 32, dtype=torch.uint8)
    q = torch.zeros(4, 32, dtype=torch.uint8)
    sx, s = torch.ones(9), torch.ones(4)
    y = torch.zeros(9, 4)
    ops.linear_w8a8(xq, sx, q, s, None, y)
    with pytest.raises(ValueError):
        ops.linear_w8a8(xq[:, :24], sx, q, s, None, y)  # K % 16
    with pytest.raises(ValueError):
        ops.linear_w8a8(xq, sx[:8], q, s, None, y)  # sx shorter than M
    with pytest.raises(ValueError):
        ops.linear_w8a8(xq, sx, q, s[:3], None, y)  # sw shorter than N
    with pytest.raises(TypeError):
        ops.linear_w8a8(xq.to(torch.int8), sx, q, s, None, y)
    with pytest.raises(TypeError):
        ops.linear_w8a8(xq, sx, q.to(torch.int8), s, None, y)
    with pytest.raises(TypeError):
        ops.linear_fwd_w8a8(xq, q, s, None, y)  # the composite takes bf16 rows


def _layers(acts):
    rng = np.random.default_rng(len(acts[0]))
    return [LayerWeights(rng.standard_normal((DIMS[i + 1], DIMS[i])) / np.sqrt(DIMS[i]),
                         rng.standard_normal(DIMS[i + 1]) * 0.1, acts[i]) for i in range(2)]


@pytest.mark.parametrize("model", sorted(MODELS))
def test_cpu_engine_w8a8_chains_quantiser_and_op(model):
    """fp8_gemm="w8a8" on the CPU device: predict at 9 and 64 rows (one 64-row bucket) equals
    quant_rows_fp8 -> linear_w8a8 -> quant_rows_fp8 -> linear_w8a8 by hand on bucket-padded rows
    (the quantiser over the padded width, as the buffer stands); no scratch is allocated. The
    sigmoid model runs as two stages."""
    L = _layers(MODELS[model])
    split = model == "sigmoid"
    eng = InferenceEngine([L[:1], L[1:]] if split else [L], CPU, expected_input=40,
                          weights="fp8", fp8_gemm="w8a8")
    (q0, s0, b0, a0), (q1, s1, b1, a1) = [(st.q[i], st.s[i], st.b[i], st.acts[i])
                                          for st in eng.stages for i in range(len(st.layers))]
    for rows in (9, 64):
        x = np.random.default_rng(rows).standard_normal((rows, 40))
        xb = torch.zeros(64, 64, dtype=torch.bfloat16)
        ops.pack_bf16(torch.from_numpy(x).float(), xb[:rows])
        h = torch.zeros(64, 64, dtype=torch.bfloat16)
        f = torch.zeros(64, 64, dtype=torch.float32)
        c = torch.zeros(64, 64, dtype=torch.uint8)
        sc = torch.zeros(64)
        ops.quant_rows_fp8(xb, c, sc)
        ops.linear_w8a8(c, sc, q0, s0, b0, h, a0)
        ops.quant_rows_fp8(h, c, sc)
        ops.linear_w8a8(c, sc, q1, s1, b1, f, a1)
        assert np.array_equal(eng.predict(x), f[:rows, :10].double().numpy()), f"rows={rows}"
    assert all(st._wscratch is None for st in eng.stages)


def test_w8a8_argument():
    """"w8a8" is a value of fp8_gemm and not the default; an unknown value still raises; bf16
    weights ignore the option bit for bit."""
    L = _layers(MODELS["relu"])
    assert FP8_GEMMS == ("scratch", "direct", "w8a8")
    with pytest.raises(ValueError):
        InferenceEngine([L], CPU, expected_input=40, weights="fp8", fp8_gemm="w4a8")
    with pytest.raises(ValueError):
        InferenceStage(L, CPU, expected_input=40, weights="fp8", fp8_gemm="w4a8")
    assert InferenceEngine([L], CPU, expected_input=40, weights="fp8").stages[0].fp8_gemm == \
        "scratch"
    bf = InferenceEngine([L], CPU, expected_input=40)
    bf_w8a8 = InferenceEngine([L], CPU, expected_input=40, fp8_gemm="w8a8")
    for rows in (9, 64):
        x = np.random.default_rng(rows).standard_normal((rows, 40))
        assert np.array_equal(bf.predict(x), bf_w8a8.predict(x))
    assert not bf_w8a8.stages[0].buffers(64)["xq"]  # no code buffers either


def test_command_line_takes_w8a8(tmp_path):
    """Both parsers take --fp8-gemm w8a8 and still default to scratch; run_grpc_fcnn.py --mode
    local --device cpu --weights fp8 --fp8-gemm w8a8 --no-serve sets up."""
    from docker_dist_nn_amd.cli import fcnn, inference
    from docker_dist_nn_amd.data import write_examples
    from docker_dist_nn_amd.weights_io import export_model_json

    rng = np.random.default_rng(0)
    dims = [48, 32, 10]
    ws = [rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i]) for i in range(2)]
    bs = [rng.standard_normal(dims[i + 1]) * 0.1 for i in range(2)]
    cfg, inp = tmp_path / "model.json", tmp_path / "inputs.json"
    export_model_json(str(cfg), ws, bs, ["relu", "softmax"], layer_distribution=[1, 1])
    write_examples(str(inp), rng.random((4, 48)), np.zeros(4, dtype=np.int64))
    argv = ["--config", str(cfg), "--inputs", str(inp), "--mode", "local", "--device", "cpu",
            "--cache-dir", str(tmp_path / "cache"), "--no-serve"]
    parse = fcnn.build_parser(str(tmp_path)).parse_args
    assert parse(argv).fp8_gemm == "scratch"
    assert parse(argv + ["--fp8-gemm", "w8a8"]).fp8_gemm == "w8a8"
    assert "quantises the activations" in " ".join(fcnn.build_parser(str(tmp_path)).format_help()
                                                   .split())
    assert fcnn.main(argv + ["--weights", "fp8", "--fp8-gemm", "w8a8"],
                     script_dir=str(tmp_path)) == 0
    parse = inference.build_parser(str(tmp_path)).parse_args
    assert parse(["--local", str(cfg)]).fp8_gemm == "scratch"
    a = parse(["--local", str(cfg), "--weights", "fp8", "--fp8-gemm", "w8a8"])
    assert a.weights == "fp8" and a.fp8_gemm == "w8a8"
    assert "quantises the activations" in " ".join(inference.build_parser(str(tmp_path))
                                                   .format_help().split())
