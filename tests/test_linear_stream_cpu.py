"""The weight-streaming bf16 GEMM without a GPU: ops.linear_fwd_stream on CPU tensors, the
``bf16_gemm`` option of the engine, and its way from the command line to the plan and worker."""
import json
import signal

import numpy as np
import pytest
import torch

import _act_oracle as ao
import _linear_fp8_cases as lc
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.engine.inference import BF16_GEMMS, InferenceEngine, InferenceStage
from test_linear_fp8_cpu import MODELS, _layers

CPU = torch.device("cpu")


@pytest.mark.parametrize("act", ao.ACTS)
def test_cpu_op_is_the_reference_layer(act):
    """CPU tensors take the torch reference: x . w^T + b through the reference activation (the
    exact-sum operands: linear / relu equal fp64)."""
    M, N, K = 9, 17, 96
    x, xs, w, _, _, bias = lc.operands(M, N, K)
    x = xs if act == "sigmoid" else x
    y = torch.full((M, N), ao.SENTINEL)
    ops.linear_fwd_stream(x.to(torch.bfloat16), w.to(torch.bfloat16), bias.float(), y, act)
    z = x.float() @ w.float().t() + bias[:N].float()
    want = {"linear": z, "relu": torch.relu(z), "sigmoid": torch.sigmoid(z)}[act]
    torch.testing.assert_close(y, want, rtol=2.0 ** -22, atol=0.0)
    assert ops.GEMV_MAX_ROWS < 64 <= ops.BF16_STREAM_MAX_ROWS and ops.LINEAR_STREAM_TILES >= 4


@pytest.mark.parametrize("model", sorted(MODELS))
def test_cpu_engine_option(model):
    """An unknown value raises; "tiled" is the default; on the CPU device "stream" answers as
    the default does (both are the reference), and fp8 stages take and ignore it."""
    L = _layers(MODELS[model])
    assert BF16_GEMMS == ("tiled", "stream")
    with pytest.raises(ValueError):
        InferenceEngine([L], CPU, expected_input=40, bf16_gemm="direct")
    with pytest.raises(ValueError):
        InferenceStage(L, CPU, expected_input=40, bf16_gemm="direct")
    default = InferenceEngine([L], CPU, expected_input=40)
    stream = InferenceEngine([L[:1], L[1:]], CPU, expected_input=40, bf16_gemm="stream")
    fp8 = InferenceEngine([L], CPU, expected_input=40, weights="fp8", bf16_gemm="stream")
    assert default.stages[0].bf16_gemm == "tiled" and stream.stages[1].bf16_gemm == "stream"
    for rows in (3, 9, 65):
        x = np.random.default_rng(rows).standard_normal((rows, 40))
        assert np.array_equal(stream.predict(x), default.predict(x))
        assert fp8.predict(x).shape == (rows, 10)


def test_command_line_plan_and_worker_take_bf16_gemm(tmp_path, monkeypatch):
    """Both parsers take --bf16-gemm and reject another word; --mode ranks writes "bf16_gemm"
    into the plan and --mode workers STAGE_BF16_GEMM into every stage's environment (launchers
    stubbed); the worker passes it to its engine."""
    from docker_dist_nn_amd import launch
    from docker_dist_nn_amd.cli import fcnn, inference
    from docker_dist_nn_amd.data import write_examples
    from docker_dist_nn_amd.serve.worker import StageWorker
    from docker_dist_nn_amd.weights_io import export_model_json

    g = np.random.default_rng(0)
    dims = [48, 32, 10]
    ws = [g.standard_normal((n, k)) / 7 for k, n in zip(dims, dims[1:])]
    cfg, inp = tmp_path / "model.json", tmp_path / "inputs.json"
    export_model_json(str(cfg), ws, [np.zeros(n) for n in dims[1:]], ["relu", "softmax"],
                      layer_distribution=[1, 1])
    write_examples(str(inp), g.random((4, 48)), np.zeros(4, dtype=np.int64))
    base = ["--config", str(cfg), "--inputs", str(inp), "--device", "cpu",
            "--cache-dir", str(tmp_path / "cache")]
    for parse, argv in ((fcnn.build_parser(str(tmp_path)).parse_args, base),
                        (inference.build_parser(str(tmp_path)).parse_args, ["--local", str(cfg)])):
        assert parse(argv).bf16_gemm == "tiled"
        assert parse(argv + ["--bf16-gemm", "stream"]).bf16_gemm == "stream"
        with pytest.raises(SystemExit):
            parse(argv + ["--bf16-gemm", "direct"])
    seen = {}

    def stub(module, arg, *a, **kw):  # spawn_workers(envs) / spawn_ranks(["--plan", path, ..])
        seen[module] = arg
        raise RuntimeError("stub")

    monkeypatch.setattr(launch, "spawn_workers", stub)
    monkeypatch.setattr(launch, "spawn_ranks", stub)
    handlers = {s: signal.getsignal(s) for s in (signal.SIGTERM, signal.SIGINT)}
    try:  # the bring-up reports the stub's exception and returns 1
        for mode in ("workers", "ranks"):
            assert fcnn.main(base + ["--mode", mode, "--bf16-gemm", "stream"],
                             script_dir=str(tmp_path)) == 1
    finally:  # main() leaves both signals ignored after its teardown
        for s, h in handlers.items():
            signal.signal(s, h)
    envs = seen["docker_dist_nn_amd.serve.worker"]
    assert [e["STAGE_BF16_GEMM"] for e in envs] == ["stream"] * 2
    args = seen["docker_dist_nn_amd.serve.chain"]
    assert json.load(open(args[args.index("--plan") + 1]))["bf16_gemm"] == "stream"
    for value in ("stream", "tiled"):  # the last stage's environment: no next hop
        w = StageWorker(dict(envs[-1], DNN_WORKER_DEVICE="cpu", STAGE_BF16_GEMM=value))
        assert w.engine.stages[0].bf16_gemm == value
