"""Fused stage forward without a GPU: the CPU reference of ops.stage_fwd, the eligibility rule,
and the ``stage_gemm`` option from the engine to the command line, plan and worker."""
import json
import signal

import numpy as np
import pytest
import torch

import _stage_fwd_cases as sc
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.engine.inference import STAGE_GEMMS, InferenceEngine, InferenceStage
from docker_dist_nn_amd.models.mlp import NAMED_MODELS, round_up

CPU = torch.device("cpu")


def test_cpu_stage_fwd_equals_the_per_layer_chain():
    M, widths, acts = 70, [128, 192, 64, 64], ["sigmoid", "relu", "linear"]
    x, ws, bs = sc.random_case(M, widths, seed=1)
    x = torch.as_tensor(x).to(torch.bfloat16)
    ws = [torch.as_tensor(w).to(torch.bfloat16) for w in ws]
    bs = [torch.as_tensor(b).float() for b in bs]
    h = x
    for l, (w, b, a) in enumerate(zip(ws, bs, acts)):
        out = torch.zeros(M, w.shape[0], dtype=torch.float32 if l == 2 else torch.bfloat16)
        h = ops.linear_fwd(h, w, b, out, act=a)
    y = torch.zeros(M, 64)
    assert torch.equal(ops.stage_fwd(x, ws, bs, acts, y), h)


def test_stage_fwd_supported():
    for pads, acts, n_cls, why in sc.REFUSED + [([64, 64], ["relu"], 0, "one layer")]:
        assert not ops.stage_fwd_supported(pads, acts, n_cls), why
    assert ops.stage_fwd_supported([64, 64, 128], ["relu", "linear"], 65)
    assert (ops.STAGE_FWD_MAX_LAYERS, ops.STAGE_FWD_MAX_WIDTH) == (8, 512)
    for name, ok in (("mnist-fcnn", True), ("pytorch-recipe", True), ("notebook", True),
                     ("mlp8", False), ("wide", False)):
        dims = list(NAMED_MODELS[name].widths)
        pads = [round_up(d, 64) for d in dims]
        acts = ["relu"] * (len(dims) - 2) + ["softmax"]
        assert ops.stage_fwd_supported(pads, acts, dims[-1]) is ok, name


def test_engine_option_on_cpu():
    dims, acts = list(NAMED_MODELS["notebook"].widths), ["relu", "sigmoid", "softmax"]
    L = sc.model_layers(dims, acts, seed=2)
    assert STAGE_GEMMS == ("layers", "fused")
    with pytest.raises(ValueError):
        InferenceStage(L, CPU, expected_input=784, stage_gemm="fuse")
    a = InferenceEngine([L], CPU, expected_input=784)
    b = InferenceEngine([L], CPU, expected_input=784, stage_gemm="fused")
    assert a.stages[0].stage_gemm == "layers" and not a.stages[0].buffers(64)["fused"]
    for rows in (3, 65):
        x = np.random.default_rng(rows).standard_normal((rows, 784))
        assert np.array_equal(a.predict(x), b.predict(x))
    bufs = b.stages[0].buffers(64)
    assert bufs["fused"] and bufs["h"][0] is None and bufs["h"][1] is None


def test_command_line_plan_and_worker_take_stage_gemm(tmp_path, monkeypatch):
    """Both parsers take --stage-gemm; --mode ranks writes "stage_gemm" into the plan and
    --mode workers STAGE_GEMM into every stage's environment (launchers stubbed)."""
    from docker_dist_nn_amd import launch
    from docker_dist_nn_amd.cli import fcnn, inference
    from docker_dist_nn_amd.data import write_examples
    from docker_dist_nn_amd.weights_io import export_model_json

    g = np.random.default_rng(0)
    dims = [48, 32, 16, 10]
    ws = [g.standard_normal((n, k)) / 7 for k, n in zip(dims, dims[1:])]
    cfg, inp = tmp_path / "model.json", tmp_path / "inputs.json"
    export_model_json(str(cfg), ws, [np.zeros(n) for n in dims[1:]], ["relu", "relu", "softmax"],
                      layer_distribution=[2, 1])
    write_examples(str(inp), g.random((4, 48)), np.zeros(4, dtype=np.int64))
    base = ["--config", str(cfg), "--inputs", str(inp), "--device", "cpu",
            "--cache-dir", str(tmp_path / "cache")]
    for parse, argv in ((fcnn.build_parser(str(tmp_path)).parse_args, base),
                        (inference.build_parser(str(tmp_path)).parse_args, ["--local", str(cfg)])):
        assert parse(argv).stage_gemm == "layers"
        assert parse(argv + ["--stage-gemm", "fused"]).stage_gemm == "fused"
        with pytest.raises(SystemExit):
            parse(argv + ["--stage-gemm", "w8a8"])
    seen = {}

    def stub(module, arg, *a, **kw):  # spawn_workers(envs) / spawn_ranks(["--plan", path, ..])
        seen[module] = arg
        raise RuntimeError("stub")

    monkeypatch.setattr(launch, "spawn_workers", stub)
    monkeypatch.setattr(launch, "spawn_ranks", stub)
    handlers = {s: signal.getsignal(s) for s in (signal.SIGTERM, signal.SIGINT)}
    try:  # the bring-up reports the stub's exception and returns 1
        for mode in ("workers", "ranks"):
            assert fcnn.main(base + ["--mode", mode, "--stage-gemm", "fused"],
                             script_dir=str(tmp_path)) == 1
    finally:  # main() leaves both signals ignored after its teardown
        for s, h in handlers.items():
            signal.signal(s, h)
    assert [e["STAGE_GEMM"] for e in seen["docker_dist_nn_amd.serve.worker"]] == ["fused"] * 2
    args = seen["docker_dist_nn_amd.serve.chain"]
    assert json.load(open(args[args.index("--plan") + 1]))["stage_gemm"] == "fused"
