"""MXFP4 serving weights without a GPU: the CPU reference of ops.gemv_mxfp4 against the exact
oracle, ``InferenceStage`` / ``InferenceEngine(weights="mxfp4")`` on the CPU device, the
command-line flag and its way to the stage processes. Operands and bounds in
_gemv_mxfp4_cases.py."""
import json
import os
import signal

import numpy as np
import pytest
import torch

import _gemv_mxfp4_cases as gc
import _mxfp4_oracle as mo
from test_gemv_gpu import SIGMOID_F32_MAX_ULP
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.config import LayerWeights, load_model_config
from docker_dist_nn_amd.engine import inference as eng_mod
from docker_dist_nn_amd.engine.inference import InferenceEngine, InferenceStage

CPU = torch.device("cpu")
HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLE_CONFIG = os.path.join(HERE, "fixtures", "config_sample.json")
SAMPLE_INPUTS = os.path.join(HERE, "fixtures", "example_inputs_sample.json")
DIMS = [40, 24, 10]
MODELS = {"relu": ("relu", "linear"), "sigmoid": ("sigmoid", "sigmoid")}


@pytest.mark.parametrize("N,K", gc.NK)
def test_gemv_mxfp4_cpu_reference_equals_oracle(N, K):
    """ops.gemv_mxfp4 on CPU tensors: linear / relu exact, sigmoid (torch's fp32 sigmoid) within
    the GPU kernel's bounds."""
    gc.check_exact_shape(ops.gemv_mxfp4, N, K, CPU, SIGMOID_F32_MAX_ULP)


def test_gemv_mxfp4_cpu_zero_blocks_add_nothing():
    gc.check_zero_blocks_add_nothing(ops.gemv_mxfp4, CPU)


def test_gemv_mxfp4_rejects_bad_operands():
    x = torch.zeros(9, 64, dtype=torch.bfloat16)
    q = torch.zeros(4, 32, dtype=torch.uint8)
    e = torch.full((4, 2), 127, dtype=torch.uint8)
    y = torch.zeros(9, 4)
    with pytest.raises(ValueError):
        ops.gemv_mxfp4(x, q, e, None, y)  # 9 rows
    with pytest.raises(ValueError):
        ops.gemv_mxfp4(x[:2, :48], q, e, None, y)  # K % 32
    with pytest.raises(ValueError):
        ops.gemv_mxfp4(x[:2], q, e[:, :1], None, y)  # fewer scale bytes than blocks
    with pytest.raises(ValueError):
        ops.gemv_mxfp4(x[:2], q, e, torch.zeros(3), y)  # bias shorter than N
    with pytest.raises(TypeError):
        ops.gemv_mxfp4(x[:2], q.to(torch.int8), e, None, y)
    with pytest.raises(TypeError):
        ops.gemv_mxfp4(x[:2], q, e, None, y.double())


@pytest.mark.parametrize("N,K,M", gc.LAYERS)
def test_one_layer_stage_within_format_bound(N, K, M):
    """The stage's serving-size path (ops.gemv_mxfp4's CPU reference) against the fp64 product
    with the original bf16 weights: within the format's bound summed against |x| plus the
    summation bound."""
    w, b, x = gc.layer_case(N, K, M)
    st = InferenceStage([LayerWeights(w.float().numpy(), b.numpy(), "linear")], CPU,
                        expected_input=K, weights="mxfp4")
    st.buffers(M)["x"][:, :K].copy_(x)
    y = st.forward(M)[:, :N].double().numpy()
    ratio = gc.check_layer(y, w, b, x)
    print(f"\nmxfp4 one-layer stage {M}x{N}x{K}: error at {ratio:.3f} x the bound")


def _layers(acts):
    rng = np.random.default_rng(len(acts[0]))
    return [LayerWeights(rng.standard_normal((DIMS[i + 1], DIMS[i])) / np.sqrt(DIMS[i]),
                         rng.standard_normal(DIMS[i + 1]) * 0.1, acts[i]) for i in range(2)]


def _padded_bf16(L):
    w = torch.zeros(64, 64)
    w[:L.out_dim, :L.in_dim] = torch.as_tensor(np.asarray(L.weight, np.float32))
    return w.to(torch.bfloat16)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_cpu_engine_mxfp4(model):
    """On the CPU device: codes and scale bytes equal the oracle's, no bf16 weight is kept, and
    predict at 9 and 64 rows equals a bf16 engine on dequant_ref(q, e) bit for bit."""
    L = _layers(MODELS[model])
    eng = InferenceEngine([L], CPU, expected_input=40, weights="mxfp4")
    st = eng.stages[0]
    assert not st.w and not st.q and not st.s
    deq = []
    for i in range(2):
        q, e, _ = mo.quant_ref(_padded_bf16(L[i]))
        assert st.q4[i].dtype == torch.uint8 and tuple(st.q4[i].shape) == (64, 32)
        assert st.e4[i].dtype == torch.uint8 and tuple(st.e4[i].shape) == (64, 2)
        assert np.array_equal(st.q4[i].numpy(), q) and np.array_equal(st.e4[i].numpy(), e)
        d = mo.dequant_ref(q, e).float().numpy()
        deq.append(LayerWeights(d[:DIMS[i + 1], :DIMS[i]], L[i].bias, L[i].activation))
    bf = InferenceEngine([deq], CPU, expected_input=40)
    for rows in (9, 64):
        x = np.random.default_rng(rows).standard_normal((rows, 40))
        assert np.array_equal(eng.predict(x), bf.predict(x)), f"{model} rows={rows}"
    assert not any(t.dtype == torch.bfloat16 and t.numel() for t in (*st.w, *st.q4, *st.e4))


def test_resident_weight_bytes():
    """Per padded layer: bf16 2 Np Kp, fp8 Np Kp + 4 Np, mxfp4 Np Kp / 2 + Np Kp / 32; the
    mxfp4 engine is below the fp8 engine and below a third of the bf16 engine."""
    rng = np.random.default_rng(3)
    dims = [100, 200, 70, 10]  # padded 128, 256, 128, 64
    L = [LayerWeights(rng.standard_normal((dims[i + 1], dims[i])), np.zeros(dims[i + 1]), "relu")
         for i in range(3)]
    pads = [(256, 128), (128, 256), (64, 128)]
    got = {}
    for fmt in eng_mod.WEIGHT_FORMATS:
        eng = InferenceEngine([L[:2], L[2:]], CPU, expected_input=100, weights=fmt)
        got[fmt] = eng.resident_weight_bytes()
        assert got[fmt] == sum(st.resident_weight_bytes() for st in eng.stages)
    assert got["bf16"] == sum(2 * n * k for n, k in pads)
    assert got["fp8"] == sum(n * k + 4 * n for n, k in pads)
    assert got["mxfp4"] == sum(n * k // 2 + n * k // 32 for n, k in pads)
    assert got["mxfp4"] < got["fp8"] and 3 * got["mxfp4"] < got["bf16"]
    eng.predict(rng.standard_normal((9, 100)))  # the scratch of a large bucket is not counted
    assert eng.resident_weight_bytes() == got["mxfp4"]


def test_weight_formats_and_weight_operand():
    assert eng_mod.WEIGHT_FORMATS == ("bf16", "fp8", "mxfp4")
    L = _layers(MODELS["relu"])
    with pytest.raises(ValueError):
        InferenceStage(L, CPU, expected_input=40, weights="int4")
    st = InferenceStage(L, CPU, expected_input=40, weights="mxfp4", fp8_gemm="direct")  # ignored
    with pytest.raises(ValueError, match="mxfp4"):
        st.weight_operand(0)


def test_chain_plan_with_mxfp4_keeps_the_host_chain():
    """serve/chain.py decides from the plan, before any FastChain is built: mxfp4 vetoes the
    device-side chain with a reason to log; bf16, fp8 and plans without the entry do not."""
    from docker_dist_nn_amd.serve import chain

    why = chain.fast_chain_veto({"weights": "mxfp4", "fp8_gemm": "scratch"})
    assert why is not None and "mxfp4" in why and "host chain" in why
    for plan in ({}, {"weights": "bf16"}, {"weights": "fp8", "fp8_gemm": "direct"}):
        assert chain.fast_chain_veto(plan) is None


def _write_model(tmp_path):
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
    return cfg, inp, x


def test_command_line_takes_mxfp4(tmp_path):
    """Both parsers accept --weights mxfp4 and still reject int4; run_grpc_fcnn.py --mode local
    --weights mxfp4 --no-serve sets up on the sample config; run_grpc_inference.py --local
    --weights mxfp4 answers on it end to end."""
    from docker_dist_nn_amd.cli import fcnn, inference

    argv = ["--config", SAMPLE_CONFIG, "--inputs", SAMPLE_INPUTS, "--mode", "local", "--device",
            "cpu", "--cache-dir", str(tmp_path / "cache"), "--no-serve", "--layer-distribution",
            "[2,1]"]  # the sample has 3 layers (2 -> 3 -> 6 -> 2) and names no distribution
    parse = fcnn.build_parser(str(tmp_path)).parse_args
    assert parse(argv).weights == "bf16"
    assert parse(argv + ["--weights", "mxfp4"]).weights == "mxfp4"
    with pytest.raises(SystemExit):
        parse(argv + ["--weights", "int4"])
    assert "mxfp4" in fcnn.build_parser(str(tmp_path)).format_help()
    assert fcnn.main(argv + ["--weights", "mxfp4"], script_dir=str(tmp_path)) == 0
    iparse = inference.build_parser(str(tmp_path)).parse_args
    assert iparse(["--local", SAMPLE_CONFIG, "--weights", "mxfp4"]).weights == "mxfp4"
    with pytest.raises(SystemExit):
        iparse(["--local", SAMPLE_CONFIG, "--weights", "int4"])
    metrics = tmp_path / "metrics.json"
    assert inference.main(["--local", SAMPLE_CONFIG, "--inputs", SAMPLE_INPUTS, "--device", "cpu",
                           "--weights", "mxfp4", "--metrics-json", str(metrics)],
                          script_dir=str(tmp_path)) == 0
    m = json.load(open(metrics))
    assert m["num_examples"] >= 1 and 0 <= m["correct"] <= m["num_examples"]
    # an engine built as the local modes build it answers a softmax model
    cfg, _, x = _write_model(tmp_path)
    mc = load_model_config(str(cfg))
    eng = InferenceEngine([mc.layers[:1], mc.layers[1:]], CPU, expected_input=48,
                          names=["layer_container_0", "layer_container_1"], weights="mxfp4")
    out = eng.predict(x)
    assert out.shape == (4, 10) and np.isfinite(out).all()
    np.testing.assert_allclose(out.sum(1), 1.0, atol=1e-5)  # a softmax row


@pytest.mark.parametrize("mode", ["workers", "ranks"])
def test_weights_reach_the_stage_processes(tmp_path, monkeypatch, mode):
    """--weights mxfp4 arrives as STAGE_WEIGHTS in every worker's environment (workers mode) and
    as "weights" in chain_plan.json (ranks mode). The spawn is intercepted: no process starts."""
    from docker_dist_nn_amd import launch
    from docker_dist_nn_amd.cli import fcnn

    cfg, inp, _ = _write_model(tmp_path)
    seen = {}

    def fake_workers(module, envs, **kw):
        seen["envs"] = envs
        raise KeyboardInterrupt

    def fake_ranks(module, args, n, **kw):
        seen["plan"] = json.load(open(args[args.index("--plan") + 1]))
        raise KeyboardInterrupt

    monkeypatch.setattr(launch, "spawn_workers", fake_workers)
    monkeypatch.setattr(launch, "spawn_ranks", fake_ranks)
    handlers = {s: signal.getsignal(s) for s in (signal.SIGINT, signal.SIGTERM)}
    try:
        rc = fcnn.main(["--config", str(cfg), "--inputs", str(inp), "--mode", mode, "--device",
                        "cpu", "--cache-dir", str(tmp_path / "cache"), "--weights", "mxfp4"],
                       script_dir=str(tmp_path))
    finally:
        for s, h in handlers.items():
            signal.signal(s, h)
    assert rc == 0
    if mode == "workers":
        assert len(seen["envs"]) == 2
        assert all(e["STAGE_WEIGHTS"] == "mxfp4" for e in seen["envs"])
    else:
        assert seen["plan"]["weights"] == "mxfp4" and len(seen["plan"]["stages"]) == 2


def test_stage_worker_builds_an_mxfp4_engine(tmp_path):
    """serve/worker.py passes STAGE_WEIGHTS=mxfp4 to its engine unchanged."""
    from docker_dist_nn_amd.serve.worker import StageWorker
    from docker_dist_nn_amd.weights_io import stage_files_from_model

    cfg, _, x = _write_model(tmp_path)
    mc = load_model_config(str(cfg))
    envs = stage_files_from_model(mc, str(tmp_path / "cache"), 48, [1, 1])
    env = dict(envs[sorted(envs)[-1]])  # the last stage: no next hop
    env.update(STAGE_WEIGHTS="mxfp4", DNN_WORKER_DEVICE="cpu")
    w = StageWorker(env)
    st = w.engine.stages[0]
    assert st.weights == "mxfp4" and st.q4 and not st.w
