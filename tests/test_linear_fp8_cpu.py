"""The fp8-weight GEMM without a GPU: ops.linear_fwd_fp8 on CPU tensors against the exact
oracle, its validation, ``InferenceEngine(weights="fp8", fp8_gemm=...)`` on the CPU device and
the command-line flag. Operands in _linear_fp8_cases.py."""
import numpy as np
import pytest
import torch

import _linear_fp8_cases as lc
from test_gemv_gpu import SIGMOID_F32_MAX_ULP
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.config import LayerWeights
from docker_dist_nn_amd.engine.inference import InferenceEngine, InferenceStage

CPU = torch.device("cpu")
DIMS = [40, 24, 10]
MODELS = {"relu": ("relu", "linear"), "sigmoid": ("sigmoid", "sigmoid")}


@pytest.mark.parametrize("M,N,K", [(9, 17, 80), (70, 65, 528)])
def test_linear_fwd_fp8_cpu_reference_equals_oracle(M, N, K):
    """ops.linear_fwd_fp8 on CPU tensors at M = 9 and 70 (no row cap): linear / relu exact,
    sigmoid (torch's fp32 sigmoid) within the GPU kernel's bound."""
    lc.check_exact(ops.linear_fwd_fp8, M, N, K, CPU, SIGMOID_F32_MAX_ULP)


def test_linear_fwd_fp8_rejects_bad_operands():
    x = torch.zeros(9, 32, dtype=torch.bfloat16)
    q = torch.zeros(4, 32, dtype=torch.uint8)
    s = torch.ones(4)
    y = torch.zeros(9, 4)
    ops.linear_fwd_fp8(x, q, s, None, y)  # 9 rows are fine here
    with pytest.raises(ValueError):
        ops.linear_fwd_fp8(x[:, :24], q, s, None, y)  # K % 16
    with pytest.raises(ValueError):
        ops.linear_fwd_fp8(x, q, s[:3], None, y)  # scale shorter than N
    with pytest.raises(ValueError):
        ops.linear_fwd_fp8(x, q, s, torch.zeros(3), y)  # bias shorter than N
    with pytest.raises(ValueError):
        ops.linear_fwd_fp8(x, q, s, None, y[:8])  # y shorter than M
    with pytest.raises(TypeError):
        ops.linear_fwd_fp8(x, q.to(torch.int8), s, None, y)
    with pytest.raises(TypeError):
        ops.linear_fwd_fp8(x.float(), q, s, None, y)
    with pytest.raises(TypeError):
        ops.linear_fwd_fp8(x, q, s, None, y.double())
    assert ops.GEMV_MAX_ROWS < 64 <= ops.FP8_DIRECT_MAX_ROWS
    assert ops.FP8_DIRECT_MAX_ROWS & (ops.FP8_DIRECT_MAX_ROWS - 1) == 0  # a power-of-two bucket


def _layers(acts):
    rng = np.random.default_rng(len(acts[0]))
    return [LayerWeights(rng.standard_normal((DIMS[i + 1], DIMS[i])) / np.sqrt(DIMS[i]),
                         rng.standard_normal(DIMS[i + 1]) * 0.1, acts[i]) for i in range(2)]


@pytest.mark.parametrize("model", sorted(MODELS))
def test_cpu_engine_fp8_gemm_direct_chains_the_op(model):
    """fp8_gemm="direct" on the CPU device: predict at 9 and 64 rows (one 64-row bucket) equals
    ops.linear_fwd_fp8 chained by hand over the stages' codes; no scratch is allocated. The
    sigmoid model runs as two stages."""
    L = _layers(MODELS[model])
    split = model == "sigmoid"
    eng = InferenceEngine([L[:1], L[1:]] if split else [L], CPU, expected_input=40,
                          weights="fp8", fp8_gemm="direct")
    (q0, s0, b0, a0), (q1, s1, b1, a1) = [(st.q[i], st.s[i], st.b[i], st.acts[i])
                                          for st in eng.stages for i in range(len(st.layers))]
    for rows in (9, 64):
        x = np.random.default_rng(rows).standard_normal((rows, 40))
        xb = torch.zeros(64, 64, dtype=torch.bfloat16)
        ops.pack_bf16(torch.from_numpy(x).float(), xb[:rows])
        h = torch.zeros(64, 64, dtype=torch.bfloat16)
        f = torch.zeros(64, 64, dtype=torch.float32)
        ops.linear_fwd_fp8(xb, q0, s0, b0, h, a0)
        ops.linear_fwd_fp8(h, q1, s1, b1, f, a1)
        assert np.array_equal(eng.predict(x), f[:rows, :10].double().numpy()), f"rows={rows}"
    assert all(st._wscratch is None for st in eng.stages)


def test_fp8_gemm_argument():
    """An unknown value raises; "scratch" is the default, bit for bit; bf16 weights ignore it."""
    L = _layers(MODELS["relu"])
    with pytest.raises(ValueError):
        InferenceEngine([L], CPU, expected_input=40, weights="fp8", fp8_gemm="int4")
    with pytest.raises(ValueError):
        InferenceStage(L, CPU, expected_input=40, weights="fp8", fp8_gemm="int4")
    default = InferenceEngine([L], CPU, expected_input=40, weights="fp8")
    scratch = InferenceEngine([L], CPU, expected_input=40, weights="fp8", fp8_gemm="scratch")
    assert default.stages[0].fp8_gemm == "scratch"
    bf = InferenceEngine([L], CPU, expected_input=40)
    bf_direct = InferenceEngine([L], CPU, expected_input=40, fp8_gemm="direct")
    for rows in (9, 64):
        x = np.random.default_rng(rows).standard_normal((rows, 40))
        assert np.array_equal(default.predict(x), scratch.predict(x))
        assert np.array_equal(bf.predict(x), bf_direct.predict(x))
    assert scratch.stages[0]._wscratch is not None


def test_command_line_takes_fp8_gemm(tmp_path):
    """Both parsers take --fp8-gemm and default to scratch; run_grpc_fcnn.py --mode local
    --device cpu --weights fp8 --fp8-gemm direct --no-serve sets up."""
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
    assert parse(argv + ["--fp8-gemm", "direct"]).fp8_gemm == "direct"
    with pytest.raises(SystemExit):
        parse(argv + ["--fp8-gemm", "int4"])
    assert fcnn.main(argv + ["--weights", "fp8", "--fp8-gemm", "direct"],
                     script_dir=str(tmp_path)) == 0
    parse = inference.build_parser(str(tmp_path)).parse_args
    assert parse(["--local", str(cfg)]).fp8_gemm == "scratch"
    a = parse(["--local", str(cfg), "--weights", "fp8", "--fp8-gemm", "direct"])
    assert a.weights == "fp8" and a.fp8_gemm == "direct"
