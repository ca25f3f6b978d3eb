"""mxfp4 rank chains on the device-side chain, the parts that need no GPU: the stage's MXFP4
operand accessor (what serve/fastpath.py hands to the chain kernels), the plan's opt-in entry
``"mxfp4_chain"`` as serve/chain.py reads it, and the command line that writes it."""
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

import _mxfp4_oracle as mo
from docker_dist_nn_amd.config import LayerWeights
from docker_dist_nn_amd.engine.inference import InferenceStage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def _layers():
    rng = np.random.default_rng(8)
    dims = [40, 24, 10]
    return [LayerWeights(rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i]),
                         rng.standard_normal(dims[i + 1]) * 0.1, "relu") for i in range(2)]


def test_mxfp4_operand_is_the_stage_own_codes_and_scales():
    """The stage's resident tensors in place -- same data_ptr, strides in bytes, the padded
    shape -- holding the oracle's quantisation of the padded bf16 weight; no bf16 copy is kept;
    weight_operand keeps raising."""
    L = _layers()
    st = InferenceStage(L, CPU, expected_input=40, weights="mxfp4")
    assert not st.w and not st.q
    for i in range(2):
        q, ldq, e, lde, shape = st.mxfp4_operand(i)
        assert q is st.q4[i] and e is st.e4[i]
        assert q.data_ptr() == st.q4[i].data_ptr() and e.data_ptr() == st.e4[i].data_ptr()
        assert q.dtype == torch.uint8 and e.dtype == torch.uint8
        assert shape == (64, 64) and tuple(q.shape) == (64, 32) and tuple(e.shape) == (64, 2)
        assert ldq == q.stride(0) == 32 and lde == e.stride(0) == 2
        w = torch.zeros(64, 64)
        w[:L[i].out_dim, :L[i].in_dim] = torch.as_tensor(np.asarray(L[i].weight, np.float32))
        qr, er, _ = mo.quant_ref(w.to(torch.bfloat16))
        assert np.array_equal(q.numpy(), qr) and np.array_equal(e.numpy(), er)
    with pytest.raises(ValueError, match="mxfp4_operand"):
        st.weight_operand(0)


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_mxfp4_operand_raises_for_other_formats(weights):
    st = InferenceStage(_layers(), CPU, expected_input=40, weights=weights)
    with pytest.raises(ValueError, match=weights):
        st.mxfp4_operand(0)
    assert st.weight_operand(0)[2] == (64, 64)


def test_fast_chain_veto_reads_the_opt_in():
    """"device" lifts the veto of an mxfp4 plan; absent or "host" keeps the reason; anything else
    is an error; bf16 and fp8 plans ignore the entry, whatever it holds."""
    from docker_dist_nn_amd.serve.chain import fast_chain_veto

    for gemm in ("scratch", "w4a8"):
        plan = {"weights": "mxfp4", "mxfp4_gemm": gemm, "stages": []}
        assert fast_chain_veto(dict(plan, mxfp4_chain="device")) is None
        for p in (plan, dict(plan, mxfp4_chain="host")):
            why = fast_chain_veto(p)
            assert why and "mxfp4" in why and "host chain" in why and "--mxfp4-chain" in why
        for bad in ("Device", "", "auto", None, 1):
            with pytest.raises(ValueError, match="mxfp4_chain"):
                fast_chain_veto(dict(plan, mxfp4_chain=bad))
    for weights in ("bf16", "fp8"):
        for mode in ("device", "host", "nonsense"):
            assert fast_chain_veto({"weights": weights, "mxfp4_chain": mode}) is None
    assert fast_chain_veto({"mxfp4_chain": "device"}) is None


def test_command_line_takes_mxfp4_chain(tmp_path, monkeypatch):
    """The fcnn parser takes --mxfp4-chain {host,device} and defaults to host; --mode ranks
    writes "mxfp4_chain" into the plan JSON (the launcher is stubbed: nothing is started);
    --mode local ignores the flag and sets up."""
    from docker_dist_nn_amd import launch
    from docker_dist_nn_amd.cli import fcnn
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
            "--cache-dir", str(tmp_path / "cache")]
    parse = fcnn.build_parser(str(tmp_path)).parse_args
    assert parse(base).mxfp4_chain == "host"
    assert parse(base + ["--mxfp4-chain", "device"]).mxfp4_chain == "device"
    with pytest.raises(SystemExit):
        parse(base + ["--mxfp4-chain", "fast"])
    assert "--mxfp4-chain" in fcnn.build_parser(str(tmp_path)).format_help()
    assert fcnn.main(base + ["--no-serve", "--mode", "local", "--weights", "mxfp4",
                             "--mxfp4-chain", "device"], script_dir=str(tmp_path)) == 0

    class Stop(Exception):
        pass

    plans = []

    def spawn_ranks(module, args, n, **kw):
        plans.append(json.load(open(args[args.index("--plan") + 1])))
        raise Stop

    monkeypatch.setattr(launch, "spawn_ranks", spawn_ranks)
    handlers = {s: signal.getsignal(s) for s in (signal.SIGTERM, signal.SIGINT)}
    try:  # the bring-up reports the stub's exception and returns 1
        for extra in ([], ["--mxfp4-chain", "device"]):
            assert fcnn.main(base + ["--mode", "ranks", "--weights", "mxfp4", *extra],
                             script_dir=str(tmp_path)) == 1
    finally:  # main() leaves both signals ignored after its teardown
        for s, h in handlers.items():
            signal.signal(s, h)
    assert [p["mxfp4_chain"] for p in plans] == ["host", "device"]
    assert all(p["weights"] == "mxfp4" for p in plans)


def test_chain_latency_lists_the_mxfp4_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench", "chain_latency.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--mxfp4-chain" in r.stdout and "mxfp4" in r.stdout


@pytest.mark.parametrize("N,K,rows", [(1024, 832, 8), (64, 2080, 2), (64, 2080, 3),
                                      (1024, 1024, 2), (64, 4096, 2), (64, 4096, 8)])
def test_the_random_layers_tell_the_two_lane_orders_apart(N, K, rows):
    """The GPU tests pin the kernels' lane order by comparing fp32 linear outputs on these
    layers bit for bit with ops.gemv_mxfp4. That only pins anything if the order shows there:
    the CPU emulation of the whole-block and of the half-block order must differ in some fp32
    output of each layer (in bf16 they need not, which is why those comparisons are fp32), and
    both must be the layer, within fp32 summation error of the fp64 product."""
    import _chain_mxfp4_cases as cc

    assert (N, K) in cc.FUSED + [cc.FOLDED, cc.LDS_LIMIT]
    x, q, e, b = cc.random_layer(N, K)
    half = cc.emulate(x[:rows], q, e, b, 16)
    whole = cc.emulate(x[:rows], q, e, b, 32)
    differ = int((half != whole).sum())
    print(f"{rows}x{N}x{K}: the two orders differ in {differ} of {half.size} fp32 outputs, "
          f"{int((torch.from_numpy(half).bfloat16() != torch.from_numpy(whole).bfloat16()).sum())}"
          f" bf16 outputs")
    assert differ > 0
    w64 = mo.values(q.numpy(), e.numpy())
    ref = x[:rows].double().numpy() @ w64.T + b.double().numpy()
    mag = np.abs(x[:rows].double().numpy()) @ np.abs(w64).T + np.abs(b.double().numpy())
    for got in (half, whole):
        assert (np.abs(got - ref) <= (K // 16 + 8) * 2.0 ** -24 * mag).all()
