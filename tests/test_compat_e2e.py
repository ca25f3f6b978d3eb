"""End-to-end compatibility on CPU: run_grpc_fcnn.py brings up the stages (in-process or one
gloo rank per stage), run_grpc_inference.py talks the reference gRPC protocol to it, and the
answers match the fp64 reference forward. Also covers the error paths (INVALID_ARGUMENT for a
width mismatch, a failing middle stage surfacing as "Failed to forward request to ...")."""
import json
import os
import socket
import subprocess
import sys
import time

import grpc
import numpy as np
import pytest

from docker_dist_nn_amd.config import load_model_config
from docker_dist_nn_amd.cpu_ref import model_forward
from docker_dist_nn_amd.data import write_examples
from docker_dist_nn_amd.serve.ingress import LayerClient
from docker_dist_nn_amd.weights_io import export_model_json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module")
def model_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("m")
    rng = np.random.default_rng(0)
    dims = [784, 64, 32, 10]
    ws = [rng.standard_normal((dims[i + 1], dims[i])) * (2.0 / np.sqrt(dims[i])) for i in range(3)]
    bs = [rng.standard_normal(dims[i + 1]) * 0.1 for i in range(3)]
    cfg = d / "model.json"
    export_model_json(str(cfg), ws, bs, ["relu", "relu", "softmax"], layer_distribution=[1, 1, 1])
    x = rng.random((300, 784))
    y = model_forward(load_model_config(str(cfg)).layers, x).argmax(1)  # fp64 labels
    inp = d / "inputs.json"
    write_examples(str(inp), x, y)
    return cfg, inp, x, y


def _start(cfg, inp, port, mode, tmp, extra_env=None, args=()):
    env = dict(os.environ, PYTHONPATH=ROOT, **(extra_env or {}))
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "src", "run_grpc_fcnn.py"),
                          "--config", str(cfg), "--inputs", str(inp), "--port", str(port),
                          "--mode", mode, "--device", "cpu", "--run-for", "120",
                          "--cache-dir", str(tmp / f"cache_{mode}"), *args],
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    t0 = time.time()
    while time.time() - t0 < 90:
        try:
            socket.create_connection(("127.0.0.1", port), timeout=0.5).close()
            return p
        except OSError:
            if p.poll() is not None:
                raise RuntimeError(p.stdout.read())
            time.sleep(0.3)
    p.terminate()
    raise RuntimeError("server did not come up")


def _stop(p):
    p.terminate()
    try:
        out, _ = p.communicate(timeout=30)
    except subprocess.TimeoutExpired:
        p.kill()
        out, _ = p.communicate()
    return out


def _client(inp, port, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "src", "run_grpc_inference.py"),
                        "--inputs", str(inp), "--port", str(port), *args],
                       capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    return r.stdout + r.stderr


@pytest.mark.parametrize("mode", ["local", "ranks", "workers"])
def test_fcnn_chain_serves_reference_protocol(model_files, tmp_path, mode):
    cfg, inp, x, y = model_files
    port = _port()
    p = _start(cfg, inp, port, mode, tmp_path)
    try:
        log = _client(inp, port, "--batch-size", "128")
        assert "Batch 3/3 completed" in log
        assert "Inference process completed." in log
        n = int(log.split("Correct predictions: ")[1].split(" ")[0])
        assert n >= 290, log  # bf16 vs fp64 may flip a near-tie
        c = LayerClient(f"127.0.0.1:{port}", timeout=30)
        out = c.process(x[:5])
        ref = model_forward(load_model_config(str(cfg)).layers, x[:5])
        np.testing.assert_allclose(out, ref, atol=2e-2)
        # width mismatch -> INVALID_ARGUMENT with the reference's dimension message
        with pytest.raises(grpc.RpcError) as ei:
            c.process(np.ones((2, 5)))
        assert ei.value.code() == grpc.StatusCode.INVALID_ARGUMENT
        assert "expected input dim 784, got 5" in ei.value.details()
        # single-index mode counts one example (reference miscounted)
        log1 = _client(inp, port, "7")
        assert "out of 1" in log1
        c.close()
    finally:
        out = _stop(p)
    assert "Distributed FCNN setup completed in" in out
    assert "Shutdown complete." in out


def test_failing_middle_stage_is_reported(model_files, tmp_path):
    cfg, inp, x, y = model_files
    port = _port()
    p = _start(cfg, inp, port, "ranks", tmp_path, {"DNN_FAULT_STAGE": "1"})
    try:
        c = LayerClient(f"127.0.0.1:{port}", timeout=30)
        with pytest.raises(grpc.RpcError) as ei:
            c.process(x[:4])
        assert ei.value.code() == grpc.StatusCode.INTERNAL
        assert "Failed to forward request to layer_container_1" in ei.value.details()
        c.close()
    finally:
        _stop(p)


def test_reference_mapping_errors_are_logged(model_files, tmp_path):
    cfg, inp, *_ = model_files
    r = subprocess.run([sys.executable, os.path.join(ROOT, "src", "run_grpc_fcnn.py"),
                        "--config", str(cfg), "--inputs", str(inp), "--no-serve",
                        "--layer-distribution", "[1,1]", "--cache-dir", str(tmp_path / "c")],
                       capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert "Sum of layer_distribution does not match" in r.stderr + r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "src", "run_grpc_fcnn.py"),
                        "--config", str(tmp_path / "missing.json"), "--inputs", str(inp)],
                       capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert "Configuration file not found" in r.stderr + r.stdout
    # stage files are written in the reference's per-stage format
    r = subprocess.run([sys.executable, os.path.join(ROOT, "src", "run_grpc_fcnn.py"),
                        "--config", str(cfg), "--inputs", str(inp), "--no-serve",
                        "--cache-dir", str(tmp_path / "c2")],
                       capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    f = tmp_path / "c2" / "layer_container_1_neurons_config.json"
    doc = json.load(open(f))
    assert list(doc) == ["layer_1"] and len(doc["layer_1"]) == 32
    assert len(doc["layer_1"][0]["weights"]) == 64


def test_hung_middle_stage_maps_to_deadline_and_ingress_keeps_answering(model_files, tmp_path):
    """A stage that stops responding (after serving one request) must not wedge the chain:
    the caller gets DEADLINE_EXCEEDED "Failed to forward request to layer_container_1" within
    the per-hop deadline (reference: 10 s per hop, grpc_node.py:133-140), later requests are
    answered within their deadline too, stage-0 validation errors still come back at once,
    and teardown completes."""
    cfg, inp, x, y = model_files
    port = _port()
    p = _start(cfg, inp, port, "ranks", tmp_path,
               {"DNN_FAULT_STAGE": "1", "DNN_FAULT_KIND": "hang", "DNN_FAULT_AFTER": "1"},
               args=("--hop-timeout", "1.5"))
    try:
        c = LayerClient(f"127.0.0.1:{port}", timeout=30)
        ref = model_forward(load_model_config(str(cfg)).layers, x[:4])
        np.testing.assert_allclose(c.process(x[:4]), ref, atol=2e-2)  # served before the hang
        for _ in range(2):
            t0 = time.monotonic()
            with pytest.raises(grpc.RpcError) as ei:
                c.process(x[:4])
            dt = time.monotonic() - t0
            assert ei.value.code() == grpc.StatusCode.DEADLINE_EXCEEDED, ei.value
            assert "Failed to forward request to layer_container_1" in ei.value.details()
            assert dt < 2 * 1.5 + 2.0, dt  # 2 hops x 1.5 s, plus slack
        with pytest.raises(grpc.RpcError) as ei:  # the ingress itself is not blocked
            c.process(np.ones((2, 5)))
        assert ei.value.code() == grpc.StatusCode.INVALID_ARGUMENT
        c.close()
    finally:
        t0 = time.monotonic()
        out = _stop(p)
        assert time.monotonic() - t0 < 40
    assert "Shutdown complete." in out


def test_concurrent_requests_through_rank_chain(model_files, tmp_path):
    """Several requests in flight through a 3-rank chain at once (10 ingress workers, the
    reference's pool size): every caller gets its own rows back."""
    from concurrent.futures import ThreadPoolExecutor

    cfg, inp, x, y = model_files
    port = _port()
    p = _start(cfg, inp, port, "ranks", tmp_path)
    try:
        layers = load_model_config(str(cfg)).layers
        c = LayerClient(f"127.0.0.1:{port}", timeout=60)
        chunks = [x[i * 7:(i + 1) * 7 + i] for i in range(24)]  # distinct sizes and rows
        with ThreadPoolExecutor(8) as pool:
            outs = list(pool.map(c.process, chunks))
        for ch, out in zip(chunks, outs):
            np.testing.assert_allclose(out, model_forward(layers, ch), atol=2e-2)
        c.close()
    finally:
        _stop(p)


# One batch request exactly as the ORIGINAL client puts it on the wire: the bytes its generated
# dist_nn_pb2 stubs serialised for Matrix{Row{values}} with 32 rows of 784 values in [0, 1)
# (recorded once from the reference's run_grpc_inference.py stubs; data only).
GOLDEN_REQUEST = os.path.join(ROOT, "tests", "golden", "reference_client_request.bin")


@pytest.mark.parametrize("mode", ["local", "ranks", "workers"])
def test_reference_client_wire_bytes_interop(model_files, tmp_path, mode):
    """The original client's recorded request bytes, sent the way that client sends them (one
    persistent channel with unlimited message sizes, a unary call on
    /grpc_dist_nn.LayerService/Process per batch, no codec of ours on the client side), are
    served by our ingress, and the raw reply parses with the stock protobuf classes of the
    reference's schema -- what its generated stubs do -- into the fp64 forward's answers."""
    from docker_dist_nn_amd.serve import proto

    cfg, inp, _, _ = model_files
    with open(GOLDEN_REQUEST, "rb") as f:
        request = f.read()
    sent = proto.Matrix()
    sent.ParseFromString(request)
    x = np.array([list(r.values) for r in sent.rows])
    assert x.shape == (32, 784)
    ref = model_forward(load_model_config(str(cfg)).layers, x)
    port = _port()
    p = _start(cfg, inp, port, mode, tmp_path)
    try:
        ch = grpc.insecure_channel(f"127.0.0.1:{port}",
                                   options=[("grpc.max_send_message_length", -1),
                                            ("grpc.max_receive_message_length", -1)])
        grpc.channel_ready_future(ch).result(timeout=15)
        call = ch.unary_unary("/grpc_dist_nn.LayerService/Process")  # raw bytes both ways
        # the first stage listens before the later ones do (workers mode); a client process
        # takes longer to start than that, so poll until the chain forwards
        t0 = time.time()
        while True:
            try:
                call(request, timeout=30)
                break
            except grpc.RpcError as e:
                if e.code() != grpc.StatusCode.UNAVAILABLE or time.time() - t0 > 60:
                    raise
                time.sleep(0.2)
        for _ in range(3):  # the client's batches reuse the one channel
            reply = proto.Matrix()
            reply.ParseFromString(call(request, timeout=30))
            out = np.vstack([r.values for r in reply.rows])
            assert out.shape == (32, 10)
            # the client's count of correct predictions; the original asked for 290 of 300
            # (bf16 vs fp64 may flip a near-tie): the same share of 32 rows is 31
            assert int((out.argmax(1) == ref.argmax(1)).sum()) >= 31
            np.testing.assert_allclose(out, ref, atol=2e-2)
        ch.close()
    finally:
        _stop(p)


def test_worker_env_contract_and_forward_failure(model_files, tmp_path):
    """--mode workers: each stage process is configured ONLY by the reference's env contract
    (NEURONS_CONFIG inline for small stages, NEURONS_FILE_CONFIG for > 1000 characters); a dead
    downstream stage surfaces as the reference's "Failed to forward request to <host:port>"
    with the downstream gRPC code (UNAVAILABLE), and the first stage keeps serving errors."""
    from docker_dist_nn_amd.serve.worker import StageWorker
    from docker_dist_nn_amd.weights_io import stage_files_from_model

    cfg, inp, x, y = model_files
    mc = load_model_config(str(cfg))
    envs = stage_files_from_model(mc, str(tmp_path / "c"), 784, [2, 1])
    assert "NEURONS_FILE_CONFIG" in envs[0] and "NEURONS_CONFIG" not in envs[0]
    w0 = StageWorker(dict(envs[0], DNN_WORKER_DEVICE="cpu"))
    assert w0.container_name == "layer_container_0" and len(w0.layers) == 2
    assert w0.next_nodes == [{"host": "layer_container_1", "port": "5201"}]
    tiny = tmp_path / "tiny.json"
    export_model_json(str(tiny), [np.ones((3, 4)), np.ones((2, 3))], [np.zeros(3), np.zeros(2)],
                      ["relu", "softmax"], layer_distribution=[1, 1])
    small = stage_files_from_model(load_model_config(str(tiny)), str(tmp_path / "c2"), 4)
    for env in small.values():  # < 1000 characters: inline, like run_grpc_fcnn.py:126
        assert "NEURONS_CONFIG" in env and json.loads(env["NEURONS_CONFIG"])["layer_1"]
    w1 = StageWorker(dict(small[1], DNN_WORKER_DEVICE="cpu"))
    assert w1.expected_input_dim == 3 and w1.next_nodes == []
    np.testing.assert_allclose(w1.predict(np.ones((1, 3))), [[0.5, 0.5]], atol=1e-6)
    port = _port()
    p = _start(cfg, inp, port, "workers", tmp_path)
    try:
        c = LayerClient(f"127.0.0.1:{port}", timeout=30)
        ref = model_forward(mc.layers, x[:3])
        t0 = time.monotonic()
        while True:  # stage 0 listens first; wait until the whole chain answers
            try:
                got = c.process(x[:3])
                break
            except grpc.RpcError:
                if time.monotonic() - t0 > 60:
                    raise
                time.sleep(0.3)
        np.testing.assert_allclose(got, ref, atol=2e-2)
        ready = tmp_path / "cache_workers" / "chain_ready.json"
        while not ready.exists() and time.monotonic() - t0 < 60:  # setup fully finished
            time.sleep(0.1)
        # kill the last stage: the previous hop reports UNAVAILABLE for it
        last_port = port + 200
        pid = int(open(tmp_path / "cache_workers" / "layer_container_2.pid").read())
        os.kill(pid, 9)
        time.sleep(0.5)
        errs = []
        for _ in range(3):  # the first call may see the dying connection rather than a refusal
            with pytest.raises(grpc.RpcError) as ei:
                c.process(x[:3])
            errs.append((ei.value.code(), ei.value.details()))
            if ei.value.code() == grpc.StatusCode.UNAVAILABLE and \
                    f"Failed to forward request to 127.0.0.1:{last_port}" in ei.value.details():
                break
            time.sleep(0.5)
        else:
            raise AssertionError(errs)
        c.close()
    finally:
        _stop(p)


@pytest.fixture(scope="module")
def model4_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("m4")
    rng = np.random.default_rng(1)
    dims = [784, 64, 48, 32, 10]
    ws = [rng.standard_normal((dims[i + 1], dims[i])) * (2.0 / np.sqrt(dims[i])) for i in range(4)]
    bs = [rng.standard_normal(dims[i + 1]) * 0.1 for i in range(4)]
    cfg = d / "model4.json"
    export_model_json(str(cfg), ws, bs, ["relu", "relu", "relu", "softmax"],
                      layer_distribution=[1, 1, 1, 1])
    x = rng.random((64, 784))
    inp = d / "inputs4.json"
    write_examples(str(inp), x, np.zeros(64, dtype=np.int64))
    return cfg, inp, x


@pytest.mark.parametrize("rows", [1, 40])  # one-packet serving path, packet + payload path
def test_hung_stage_2_of_4_is_the_one_blamed(model4_files, tmp_path, rows):
    """Stage 2 of a 4-rank chain hangs after one request: every later request fails with
    DEADLINE_EXCEEDED "Failed to forward request to layer_container_2" -- the stage that
    stopped, found from the per-rank progress each stage publishes -- not the first hop's
    name (the round-2 chain always blamed names[1])."""
    cfg, inp, x = model4_files
    port = _port()
    p = _start(cfg, inp, port, "ranks", tmp_path,
               {"DNN_FAULT_STAGE": "2", "DNN_FAULT_KIND": "hang", "DNN_FAULT_AFTER": "1"},
               args=("--hop-timeout", "1.0"))
    try:
        c = LayerClient(f"127.0.0.1:{port}", timeout=30)
        ref = model_forward(load_model_config(str(cfg)).layers, x[:rows])
        np.testing.assert_allclose(c.process(x[:rows]), ref, atol=2e-2)  # before the hang
        for _ in range(2):
            with pytest.raises(grpc.RpcError) as ei:
                c.process(x[:rows])
            assert ei.value.code() == grpc.StatusCode.DEADLINE_EXCEEDED, ei.value
            assert "Failed to forward request to layer_container_2" in ei.value.details(), \
                ei.value.details()
        c.close()
    finally:
        _stop(p)


def test_train_one_rank_per_stage_matches_single_process(model4_files, tmp_path):
    """run_grpc_fcnn.py --train with one process per stage (--mode ranks: cli/train.py under
    launch.spawn_ranks, gloo on CPU) trains [1,1,1,1] like the single-process (loopback)
    trainer: the exported neuron-JSON weights agree within bf16 tolerance."""
    cfg, inp, _ = model4_files
    outs = {}
    for mode in ("local", "ranks"):
        out = tmp_path / f"trained_{mode}.json"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "src", "run_grpc_fcnn.py"),
                            "--config", str(cfg), "--inputs", str(inp), "--mode", mode,
                            "--device", "cpu", "--train", "--steps", "4", "--synthetic", "2048",
                            "--micro-batch", "128", "--num-micro-batches", "4", "--lr", "0.05",
                            "--no-serve", "--save", str(out),
                            "--cache-dir", str(tmp_path / f"c_{mode}")],
                           capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, PYTHONPATH=ROOT))
        assert r.returncode == 0, r.stdout + r.stderr
        if mode == "ranks":
            assert "training with 4 ranks" in r.stdout + r.stderr
        outs[mode] = load_model_config(str(out)).layers
    start = load_model_config(str(cfg)).layers
    for a, b, s0 in zip(outs["local"], outs["ranks"], start):
        assert not np.allclose(a.weight, s0.weight)  # it trained
        np.testing.assert_allclose(a.weight, b.weight, rtol=2e-2, atol=2e-3)
        np.testing.assert_allclose(a.bias, b.bias, rtol=2e-2, atol=2e-3)
