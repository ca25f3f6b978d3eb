"""MXFP4 weights x fp8 activations without a GPU: ops.linear_w4a8 on CPU tensors (the reference
in ops/reference.py) against the exact oracles, a demonstration that the checker rejects wrong
implementations, ``InferenceEngine(weights="mxfp4", mxfp4_gemm="w4a8")`` on the CPU device, and
the command-line flag with the plan JSON and the worker environment it travels in. Operands in
_linear_w4a8_cases.py."""
import json
import signal

import numpy as np
import pytest
import torch

import _linear_w4a8_cases as c4
import _mxfp4_oracle as mo
from test_gemv_gpu import SIGMOID_F32_MAX_ULP
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.config import LayerWeights
from docker_dist_nn_amd.engine.inference import (MXFP4_GEMMS, InferenceEngine, InferenceStage)
from docker_dist_nn_amd.ops import reference as ref

CPU = torch.device("cpu")
DIMS = [40, 24, 10]
MODELS = {"relu": ("relu", "linear"), "sigmoid": ("sigmoid", "sigmoid")}


@pytest.mark.parametrize("M,N,K", [(9, 17, 32), (65, 33, 160)])
def test_linear_w4a8_cpu_reference_equals_oracle(M, N, K):
    """ops.linear_w4a8 on CPU tensors: linear / relu exact on the exact-sum operands (block
    scales, E = 0 blocks over junk codes and the row-scale multiply included), sigmoid (torch's
    fp32 sigmoid) within the GPU kernel's bound."""
    c4.check_exact(ops.linear_w4a8, M, N, K, CPU, SIGMOID_F32_MAX_ULP)


def test_linear_w4a8_cpu_reference_decode_and_zero_block():
    c4.check_decode(ops.linear_w4a8, CPU)
    c4.check_zero_block(ops.linear_w4a8, CPU)


def _wrong(kind):
    """An implementation of linear_w4a8 with one defect, in fp64 then the fp32 epilogue."""
    def entry(xq, sx, q, e, bias, y, act):
        M, K = xq.shape
        N = q.shape[0]
        qb, eb = q[:N, :K // 2].numpy().copy(), e[:N, :K // 32].numpy().copy()
        code = mo.unpack(qb)
        if kind == "nibbles swapped":
            code = mo.unpack(((qb & 15) << 4) | (qb >> 4))
        if kind == "scale per 64 columns":
            eb = np.repeat(eb[:, 0::2], 2, axis=1)[:, :eb.shape[1]]
        E = np.repeat(eb.astype(np.int64), 32, axis=1)
        w = np.ldexp(mo.DEC[code], E - 127)
        if kind != "E = 0 as 2^-127":
            w = np.where(E == 0, 0.0, w)
        S = ref._E4M3[xq[:M, :K].long()] @ torch.from_numpy(w).t()
        v = S.float() if kind == "row scale dropped" else sx[:M].float()[:, None] * S.float()
        if bias is not None:
            v = v + bias[:N].float()
        y[:M, :N] = ref.act_fwd(v, ops.kernels.ACT_CODE[act]).to(y.dtype)
    return entry


@pytest.mark.parametrize("kind", ["scale per 64 columns", "nibbles swapped", "E = 0 as 2^-127",
                                  "row scale dropped"])
def test_checker_rejects_wrong_implementations(kind):
    """The checks of _linear_w4a8_cases.py pass on a correct implementation written the same way
    and fail on each defect: a scale byte shared by two blocks, the two codes of a byte swapped,
    an E = 0 block multiplied by 2^-127 instead of dropped, the row scale left out. The
    exact-sum check catches all but the third: 2^-127 times a code vanishes beside any sum or
    bias that fp32 holds, so that defect PASSES the exact-sum check (asserted: this is why the
    zero-block check exists) and only the zero-block check, where nothing larger hides it,
    catches it. The other three do not touch an all-zero-scale block and pass that check."""
    c4.check_exact(_wrong(None), 9, 17, 160, CPU, SIGMOID_F32_MAX_ULP)
    c4.check_zero_block(_wrong(None), CPU)
    if kind == "E = 0 as 2^-127":
        c4.check_exact(_wrong(kind), 9, 17, 160, CPU, SIGMOID_F32_MAX_ULP)
        with pytest.raises(AssertionError, match="E = 0 block contributed"):
            c4.check_zero_block(_wrong(kind), CPU)
    else:
        with pytest.raises(AssertionError, match="not the exact sum"):
            c4.check_exact(_wrong(kind), 9, 17, 160, CPU, SIGMOID_F32_MAX_ULP)
        c4.check_zero_block(_wrong(kind), CPU)


def test_linear_w4a8_cpu_rejects_bad_operands():
    xq = torch.zeros(9, 64, dtype=torch.uint8)
    q = torch.zeros(4, 32, dtype=torch.uint8)
    e = torch.full((4, 2), 127, dtype=torch.uint8)
    sx, b = torch.ones(9), torch.zeros(4)
    y = torch.zeros(9, 4)
    ops.linear_w4a8(xq, sx, q, e, b, y)
    with pytest.raises(ValueError):
        ops.linear_w4a8(xq[:, :48], sx, q, e, None, y)  # K % 32
    with pytest.raises(ValueError):
        ops.linear_w4a8(xq, sx[:8], q, e, None, y)  # sx shorter than M
    with pytest.raises(ValueError):
        ops.linear_w4a8(xq, sx, q, e[:, :1], None, y)  # e narrower than K / 32
    with pytest.raises(ValueError):
        ops.linear_w4a8(xq, sx, q, e[:3], None, y)  # e shorter than N
    with pytest.raises(ValueError):
        ops.linear_w4a8(xq, sx, q, e, b[:3], y)  # bias shorter than N
    with pytest.raises(TypeError):
        ops.linear_w4a8(xq.to(torch.int8), sx, q, e, None, y)
    with pytest.raises(TypeError):
        ops.linear_w4a8(xq, sx, q.to(torch.int8), e, None, y)
    with pytest.raises(TypeError):
        ops.linear_w4a8(xq, sx, q, e.to(torch.int8), None, y)
    with pytest.raises(ValueError):
        ops.linear_w4a8(xq, sx, q, e, None, y, tile=3)
    with pytest.raises(TypeError):
        ops.linear_fwd_w4a8(xq, q, e, None, y)  # the composite takes bf16 rows


def _layers(acts):
    rng = np.random.default_rng(len(acts[0]))
    return [LayerWeights(rng.standard_normal((DIMS[i + 1], DIMS[i])) / np.sqrt(DIMS[i]),
                         rng.standard_normal(DIMS[i + 1]) * 0.1, acts[i]) for i in range(2)]


@pytest.mark.parametrize("model", sorted(MODELS))
def test_cpu_engine_w4a8_chains_quantiser_and_op(model):
    """mxfp4_gemm="w4a8" on the CPU device: predict at 9 and 64 rows (one 64-row bucket) equals
    quant_rows_fp8 -> linear_w4a8 -> quant_rows_fp8 -> linear_w4a8 by hand on bucket-padded rows;
    no scratch is allocated. The sigmoid model runs as two stages."""
    L = _layers(MODELS[model])
    split = model == "sigmoid"
    eng = InferenceEngine([L[:1], L[1:]] if split else [L], CPU, expected_input=40,
                          weights="mxfp4", mxfp4_gemm="w4a8")
    (q0, e0, b0, a0), (q1, e1, b1, a1) = [(st.q4[i], st.e4[i], st.b[i], st.acts[i])
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
        ops.linear_w4a8(c, sc, q0, e0, b0, h, a0)
        ops.quant_rows_fp8(h, c, sc)
        ops.linear_w4a8(c, sc, q1, e1, b1, f, a1)
        assert np.array_equal(eng.predict(x), f[:rows, :10].double().numpy()), f"rows={rows}"
    assert all(st._wscratch is None for st in eng.stages)


def test_mxfp4_gemm_argument():
    """mxfp4_gemm is validated, defaults to "scratch", and is ignored bit for bit by bf16 and
    fp8 engines, which allocate no code buffers for it; weight_operand still raises."""
    L = _layers(MODELS["relu"])
    assert MXFP4_GEMMS == ("scratch", "w4a8")
    with pytest.raises(ValueError):
        InferenceEngine([L], CPU, expected_input=40, weights="mxfp4", mxfp4_gemm="w8a8")
    with pytest.raises(ValueError):
        InferenceStage(L, CPU, expected_input=40, weights="mxfp4", mxfp4_gemm="direct")
    assert InferenceEngine([L], CPU, expected_input=40,
                           weights="mxfp4").stages[0].mxfp4_gemm == "scratch"
    for fmt in ("bf16", "fp8"):
        a = InferenceEngine([L], CPU, expected_input=40, weights=fmt)
        b = InferenceEngine([L], CPU, expected_input=40, weights=fmt, mxfp4_gemm="w4a8")
        for rows in (9, 64):
            x = np.random.default_rng(rows).standard_normal((rows, 40))
            assert np.array_equal(a.predict(x), b.predict(x))
        assert not b.stages[0].buffers(64)["xq"]
    st = InferenceStage(L, CPU, expected_input=40, weights="mxfp4", mxfp4_gemm="w4a8")
    with pytest.raises(ValueError):
        st.weight_operand(0)


def test_fast_chain_still_vetoes_mxfp4():
    from docker_dist_nn_amd.serve.chain import fast_chain_veto

    for mode in MXFP4_GEMMS:
        why = fast_chain_veto({"weights": "mxfp4", "mxfp4_gemm": mode, "stages": []})
        assert why and "mxfp4" in why


def test_command_line_takes_mxfp4_gemm(tmp_path, monkeypatch):
    """Both parsers take --mxfp4-gemm w4a8 and still default to scratch; --mode local sets up;
    --mode ranks writes "mxfp4_gemm" into the plan JSON and --mode workers puts STAGE_MXFP4_GEMM
    into every stage's environment (the launchers are stubbed: nothing is started)."""
    from docker_dist_nn_amd import launch
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
    base = ["--config", str(cfg), "--inputs", str(inp), "--device", "cpu",
            "--cache-dir", str(tmp_path / "cache"), "--no-serve"]
    argv = base + ["--mode", "local"]
    parse = fcnn.build_parser(str(tmp_path)).parse_args
    assert parse(argv).mxfp4_gemm == "scratch"
    assert parse(argv + ["--mxfp4-gemm", "w4a8"]).mxfp4_gemm == "w4a8"
    with pytest.raises(SystemExit):
        parse(argv + ["--mxfp4-gemm", "w8a8"])
    assert "block-scaled MFMA" in " ".join(fcnn.build_parser(str(tmp_path)).format_help().split())
    assert fcnn.main(argv + ["--weights", "mxfp4", "--mxfp4-gemm", "w4a8"],
                     script_dir=str(tmp_path)) == 0
    parse = inference.build_parser(str(tmp_path)).parse_args
    assert parse(["--local", str(cfg)]).mxfp4_gemm == "scratch"
    a = parse(["--local", str(cfg), "--weights", "mxfp4", "--mxfp4-gemm", "w4a8"])
    assert a.weights == "mxfp4" and a.mxfp4_gemm == "w4a8"
    assert "block-scaled MFMA" in " ".join(inference.build_parser(str(tmp_path)).format_help()
                                           .split())

    class Stop(Exception):
        pass

    seen = {}

    def spawn_workers(module, envs, **kw):
        seen["envs"] = envs
        raise Stop

    def spawn_ranks(module, args, n, **kw):
        seen["plan"] = json.load(open(args[args.index("--plan") + 1]))
        raise Stop

    monkeypatch.setattr(launch, "spawn_workers", spawn_workers)
    monkeypatch.setattr(launch, "spawn_ranks", spawn_ranks)
    serve_argv = [v for v in base if v != "--no-serve"]
    handlers = {s: signal.getsignal(s) for s in (signal.SIGTERM, signal.SIGINT)}
    try:  # the bring-up reports the stub's exception and returns 1
        for mode in ("workers", "ranks"):
            assert fcnn.main(serve_argv + ["--mode", mode, "--weights", "mxfp4", "--mxfp4-gemm",
                                           "w4a8"], script_dir=str(tmp_path)) == 1
    finally:  # main() leaves both signals ignored after its teardown
        for s, h in handlers.items():
            signal.signal(s, h)
    assert [e["STAGE_MXFP4_GEMM"] for e in seen["envs"]] == ["w4a8", "w4a8"]
    assert seen["plan"]["mxfp4_gemm"] == "w4a8" and seen["plan"]["weights"] == "mxfp4"


def test_worker_reads_stage_mxfp4_gemm(tmp_path):
    """serve.worker passes STAGE_MXFP4_GEMM to its engine, "scratch" when absent."""
    from docker_dist_nn_amd.serve.worker import StageWorker
    from docker_dist_nn_amd.weights_io import export_model_json, stage_files_from_model
    from docker_dist_nn_amd.config import load_model_config

    rng = np.random.default_rng(1)
    cfg = tmp_path / "model.json"
    export_model_json(str(cfg), [rng.standard_normal((32, 48)) / 7.0], [np.zeros(32)], ["relu"],
                      layer_distribution=[1])
    envs = stage_files_from_model(load_model_config(str(cfg)), str(tmp_path / "cache"), 48, [1])
    env = dict(envs[sorted(envs)[0]])
    env.update(DNN_WORKER_DEVICE="cpu", STAGE_WEIGHTS="mxfp4")
    assert StageWorker(dict(env)).engine.stages[0].mxfp4_gemm == "scratch"
    env["STAGE_MXFP4_GEMM"] = "w4a8"
    assert StageWorker(dict(env)).engine.stages[0].mxfp4_gemm == "w4a8"
