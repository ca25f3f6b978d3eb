"""Fused small-batch stage forward without a GPU: the CPU reference of ops.stage_gemv, the
eligibility rule, and the ``stage_gemv`` option from the engine to the command line, plan and
worker."""
import json
import signal

import numpy as np
import pytest
import torch

import _stage_fwd_cases as sc
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.engine.inference import STAGE_GEMVS, InferenceEngine, InferenceStage
from docker_dist_nn_amd.models.mlp import NAMED_MODELS

CPU = torch.device("cpu")


def test_cpu_stage_gemv_equals_the_per_layer_chain():
    M, widths, acts = 5, [128, 192, 64, 64], ["sigmoid", "relu", "softmax"]
    x, ws, bs = sc.random_case(M, widths, seed=1)
    x = torch.as_tensor(x).to(torch.bfloat16)
    ws = [torch.as_tensor(w).to(torch.bfloat16) for w in ws]
    bs = [torch.as_tensor(b).float() for b in bs]
    h = x
    for l, (w, b, a) in enumerate(zip(ws, bs, acts)):
        out = torch.zeros(M, w.shape[0], dtype=torch.float32 if l == 2 else torch.bfloat16)
        h = ops.gemv(h, w, b, out, act="linear" if a == "softmax" else a)
    ops.softmax_rows(h, h, 10)
    y = torch.zeros(M, 64)
    work, counter = torch.zeros(8 * 192, dtype=torch.bfloat16), torch.zeros(1, dtype=torch.int32)
    got = ops.stage_gemv(x, ws, bs, acts, y, work, counter, n_cls=10)
    assert torch.equal(got[:, :10], h[:, :10]) and int(counter) == 0
    with pytest.raises(ValueError):
        ops.stage_gemv(x.repeat(2, 1), ws, bs, acts, torch.zeros(10, 64), work, counter, n_cls=10)


def test_stage_gemv_supported():
    for pads, acts, n_cls, why in sc.REFUSED + [([64, 64], ["relu"], 0, "one layer")]:
        assert not ops.stage_gemv_supported(pads, acts, n_cls), why
    assert ops.stage_gemv_supported(sc.HEADLINE, ["relu"] * 3 + ["softmax"], 10)


def test_engine_option_on_cpu():
    dims, acts = list(NAMED_MODELS["notebook"].widths), ["relu", "sigmoid", "softmax"]
    L = sc.model_layers(dims, acts, seed=2)
    assert STAGE_GEMVS == ("layers", "fused")
    with pytest.raises(ValueError):
        InferenceStage(L, CPU, expected_input=784, stage_gemv="fuse")
    a = InferenceEngine([L], CPU, expected_input=784)
    b = InferenceEngine([L], CPU, expected_input=784, stage_gemv="fused", stage_gemm="fused")
    assert a.stages[0].stage_gemv == "layers" and not a.stages[0].buffers(8)["gemv_fused"]
    x = np.random.default_rng(3).standard_normal((3, 784))
    assert np.array_equal(a.predict(x), b.predict(x))
    st = b.stages[0]
    bufs = st.buffers(8)
    assert bufs["gemv_fused"] and not bufs["fused"] and all(h is not None for h in bufs["h"])
    assert int(bufs["gemv_counter"]) == 0 and bufs["gemv_work"].numel() == 8 * st.pads[1]
    assert st.buffers(64)["fused"] and not st.buffers(64)["gemv_fused"]
    for s in (st, a.stages[0]):  # the 8-row bucket itself: the CPU op against the layers
        s.buffers(8)["x"][:3] = a.stages[0].buffers(64)["x"][:3]
    assert torch.equal(st.forward(8)[:, :10], a.stages[0].forward(8)[:, :10])


def test_command_line_plan_and_worker_take_stage_gemv(tmp_path, monkeypatch):
    """Both parsers take --stage-gemv; --mode ranks writes "stage_gemv" into the plan and
    --mode workers STAGE_GEMV into every stage's environment (launchers stubbed)."""
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
        assert parse(argv).stage_gemv == "layers"
        assert parse(argv + ["--stage-gemv", "fused"]).stage_gemv == "fused"
        with pytest.raises(SystemExit):
            parse(argv + ["--stage-gemv", "fuse"])
    seen = {}

    def stub(module, arg, *a, **kw):  # spawn_workers(envs) / spawn_ranks(["--plan", path, ..])
        seen[module] = arg
        raise RuntimeError("stub")

    monkeypatch.setattr(launch, "spawn_workers", stub)
    monkeypatch.setattr(launch, "spawn_ranks", stub)
    handlers = {s: signal.getsignal(s) for s in (signal.SIGTERM, signal.SIGINT)}
    try:  # the bring-up reports the stub's exception and returns 1
        for mode in ("workers", "ranks"):
            assert fcnn.main(base + ["--mode", mode, "--stage-gemv", "fused"],
                             script_dir=str(tmp_path)) == 1
    finally:  # main() leaves both signals ignored after its teardown
        for s, h in handlers.items():
            signal.signal(s, h)
    envs = seen["docker_dist_nn_amd.serve.worker"]
    assert [(e["STAGE_GEMV"], e["STAGE_GEMM"]) for e in envs] == [("fused", "layers")] * 2
    args = seen["docker_dist_nn_amd.serve.chain"]
    plan = json.load(open(args[args.index("--plan") + 1]))
    assert (plan["stage_gemv"], plan["stage_gemm"]) == ("fused", "layers")
