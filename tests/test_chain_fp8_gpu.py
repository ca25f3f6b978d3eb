"""The device-side serving chain over fp8 weights (csrc/kernels/chain.hip with ``w_scale``,
serve/fastpath.py): the fused layer-and-send and the persistent stage kernel read e4m3 codes and
their row scales in place and must write, bit for bit, what ops.gemv_fp8 writes -- and on the
exact-sum operands of _gemv_fp8_cases.py the fp64 value itself. Then a 4-rank fp8 chain on one
GPU, persistent stages and host loop, against the fp64 forward over the oracle's dequantised
weights. Every wait is bounded by the kernels' own timeouts."""
import ctypes
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import _act_oracle as ao
import _fp8_oracle as fo
import _gemv_fp8_cases as gc
from test_chain_fast_gpu import _port, _start, _stop
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.config import LayerWeights, load_model_config
from docker_dist_nn_amd.cpu_ref import model_forward
from docker_dist_nn_amd.data import write_examples
from docker_dist_nn_amd.ops.kernels import _act
from docker_dist_nn_amd.serve.ingress import LayerClient
from docker_dist_nn_amd.utils.devmem import uncached_zeros
from docker_dist_nn_amd.utils.native import native
from docker_dist_nn_amd.weights_io import export_model_json

pytestmark = pytest.mark.gpu


class _Hop:
    """One fused layer-and-send hop: the consumer's flag block ([0] flag, [2:4] header), the
    producer's ([8] ack, [9] err), a slot of 8 rows and the arrival counter."""

    def __init__(self, dev, N, f32):
        self.n = native()
        self.N, self.f32 = N, f32
        self.flags_c = uncached_zeros((64,), torch.int32, dev)
        self.flags_p = uncached_zeros((64,), torch.int32, dev)
        self.slot = uncached_zeros((8, N), torch.float32 if f32 else torch.bfloat16, dev)
        self.counter = torch.zeros(4, dtype=torch.int32, device=dev)
        self.s = torch.cuda.Stream(dev)

    def send(self, x, q, scale, bias, act, rows, K, seq, ack_target=0, timeout=2.0, ldw=None,
             w=None):
        fp, fc = self.flags_p.data_ptr(), self.flags_c.data_ptr()
        self.n.chain_gemv_send(
            self.s.cuda_stream, x.data_ptr(), x.stride(0), w or q.data_ptr(),
            ldw or q.stride(0), bias.data_ptr(), _act(act), rows, self.N, K, int(self.f32),
            self.slot.data_ptr(), self.N, fc + 8, 0, fp + 36, 0, 0, fp + 32, ack_target, fc, seq,
            0, self.counter.data_ptr(), timeout, w_scale=scale.data_ptr())


@pytest.mark.parametrize("N,K", [(5, 1040), (10, 832), (3, 2064), (7, 4096)])
def test_fp8_fused_send_equals_fp64_oracle(dev, N, K):
    """chain_gemv_send(w_scale=...) on exact-sum operands, codes on a padded view (ldw > K): the
    slot rows EQUAL act(scale * (x . w^T) + bias) in fp64 for 1, 2, 3, 5 and 8 rows, relu and
    linear, bf16 and fp32 slots -- no tolerance, every partial sum is exact; a row of scale 0
    gives act(bias); rows past the request stay untouched; header, flag and counter end as in
    the bf16 test; a consumer that never acks is blamed and no rows are written."""
    x, _, w, q, scale, bias = gc.operands(N, K)
    qv = gc.padded_codes(q, dev)
    assert qv.stride(0) > K and qv.stride(0) % 16 == 0 and qv.data_ptr() % 16 == 0
    sv, bv = scale.float().to(dev), bias.float().to(dev)
    _, xv = ao.padded(8, K, torch.bfloat16, float("nan"), dev, x)
    seq = 0
    for f32 in (False, True):
        hop = _Hop(dev, N, f32)
        seq = 0
        for rows in (1, 2, 3, 5, 8):
            for act in ("relu", "linear"):
                seq += 1
                hop.slot.zero_()
                torch.cuda.synchronize(dev)
                hop.send(xv, qv, sv, bv, act, rows, K, seq)
                torch.cuda.synchronize(dev)
                ref = ao.act_fwd(gc.oracle_z(x, w, scale, bias, rows, N), act)
                what = f"fused fp8 send {rows}x{N}x{K} {act} f32={f32}"
                got = hop.slot.cpu()
                if f32:
                    assert torch.equal(got[:rows].double(), ref), f"{what}: not the exact sum"
                else:
                    ao.assert_bf16_close(got[:rows], ref, 0, what)
                for n in range(3, N, 4):  # scale 0: the codes do not matter
                    assert torch.equal(got[:rows, n].double(),
                                       ao.act_fwd(bias[n], act).expand(rows)), what
                assert float(got[rows:].float().abs().sum()) == 0.0, f"{what}: wrote past rows"
                assert int(hop.flags_c[0]) == seq and hop.flags_c[2:4].tolist() == [0, rows]
                assert hop.counter.tolist() == [0, 0, 0, 0]
        # the consumer never drained the slot (ack stays 0 < target): blamed (stage 0 + 1)
        seq += 1
        hop.slot.zero_()
        torch.cuda.synchronize(dev)
        hop.send(xv, qv, sv, bv, "relu", 3, K, seq, ack_target=seq, timeout=0.2)
        torch.cuda.synchronize(dev)
        assert int(hop.flags_c[0]) == seq and (int(hop.flags_c[2]) & 0xFF) == 4
        assert (int(hop.flags_c[2]) >> 8) & 0xFF == 1
        assert float(hop.slot.float().abs().sum()) == 0.0
        assert hop.counter.tolist() == [0, 0, 0, 0]


def _random_layer(dev, N, K, seed):
    """bf16 weights randn * 0.05 quantised by ops.quant_rows_fp8, a bias, 8 bf16 input rows."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(8, K, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(dev)
    b = torch.randn(N, generator=g).to(dev)
    q = torch.empty(N, K, dtype=torch.uint8, device=dev)
    s = torch.empty(N, dtype=torch.float32, device=dev)
    ops.quant_rows_fp8(w, q, s)
    return x, q, s, b


@pytest.mark.parametrize("rows", [1, 3, 8])
def test_fp8_fused_send_random_equals_gemv_fp8(dev, rows):
    """Random operands at K = 832, N = 1024 (256 workgroups): the slot is bitwise ops.gemv_fp8."""
    K, N = 832, 1024
    x, q, s, b = _random_layer(dev, N, K, rows)
    ref = torch.empty(rows, N, dtype=torch.bfloat16, device=dev)
    ops.gemv_fp8(x[:rows], q, s, b, ref, act="relu")
    hop = _Hop(dev, N, False)
    hop.send(x, q, s, b, "relu", rows, K, 1)
    torch.cuda.synchronize(dev)
    assert torch.equal(hop.slot[:rows], ref)
    assert int(hop.flags_c[0]) == 1 and hop.flags_c[2:4].tolist() == [0, rows]
    assert hop.counter.tolist() == [0, 0, 0, 0]


def test_fp8_one_launch_hop_equals_gemv_fp8(dev):
    """The folded receive (in_flag) over fp8 weights at K = N = 1024, 2 rows: x is read from the
    L2-uncached slot once its flag is up, the rows are bitwise ops.gemv_fp8's, the producer is
    acked; a missing input blames the producer and writes no rows."""
    n = native()
    K, N, rows = 1024, 1024, 2
    x, q, s, b = _random_layer(dev, N, K, 7)
    ref = torch.empty(rows, N, dtype=torch.bfloat16, device=dev)
    ops.gemv_fp8(x[:rows], q, s, b, ref, act="relu")
    f_in = uncached_zeros((64,), torch.int32, dev)    # this stage: [0] flag, [2:4] header
    f_out = uncached_zeros((64,), torch.int32, dev)   # consumer: [0] flag, [2:4] header
    f_prod = uncached_zeros((64,), torch.int32, dev)  # producer: [8] ack
    slot_in = uncached_zeros((8, K), torch.bfloat16, dev)
    slot_out = uncached_zeros((8, N), torch.bfloat16, dev)
    err = torch.zeros(4, dtype=torch.int32, device=dev)
    counter = torch.zeros(4, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)

    def hop(seq, timeout=2.0):
        n.chain_gemv_send(st.cuda_stream, slot_in.data_ptr(), K, q.data_ptr(), K, b.data_ptr(),
                          1, rows, N, K, 0, slot_out.data_ptr(), N, f_out.data_ptr() + 8,
                          f_in.data_ptr() + 8, err.data_ptr(), 1, 0, 0, 0, f_out.data_ptr(),
                          seq, f_prod.data_ptr() + 32, counter.data_ptr(), timeout,
                          in_flag=f_in.data_ptr(), w_scale=s.data_ptr())

    torch.cuda.synchronize(dev)
    hop(1)  # enqueued before its input exists: it waits (on stream st; the writes below go
    slot_in.copy_(x)  # through the current stream -- no device-wide sync while it spins)
    f_in[2:4] = torch.tensor([0, rows], dtype=torch.int32, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    f_in[0] = 1  # the producer's flag
    torch.cuda.current_stream(dev).synchronize()
    st.synchronize()
    assert torch.equal(slot_out[:rows], ref)
    assert int(f_out[0]) == 1 and f_out[2:4].tolist() == [0, rows] and int(f_prod[8]) == 1
    slot_out.zero_()
    hop(2, timeout=0.2)  # request 2 never arrives: the producer (stage 0) is blamed
    st.synchronize()
    assert int(f_out[0]) == 2 and (int(f_out[2]) & 0xFF) == 4 and (int(f_out[2]) >> 8) == 0
    assert float(slot_out.float().abs().sum()) == 0.0 and counter.tolist() == [0, 0, 0, 0]


# ---- the persistent stage ---------------------------------------------------------------------

class _Stage:
    """A persistent fp8 stage kernel (chain_stage_run with w_scale) between a simulated producer
    (feed: input slot, header, flag) and a simulated consumer (wait_out, the ack word). The
    kernel has a dedicated stream; the test's own work runs on a side stream (`with st:`), and
    leaving the block sets the stop word first, so a failing assertion never leaves the kernel
    waiting for its idle timer."""

    def __init__(self, dev, q, scale, bias, K, N, act, nslot=4, out_f32=False, n_out=None):
        self.n, self.dev = native(), dev
        self.q, self.scale, self.bias = q, scale, bias
        self.K, self.N, self.nslot, self.act, self.out_f32 = K, N, nslot, act, out_f32
        self.n_out = n_out or N
        self.f_in = uncached_zeros((64,), torch.int32, dev)    # [0:nslot] flags, [16:] headers
        self.f_out = uncached_zeros((64,), torch.int32, dev)   # the consumer: same layout
        self.f_ack = uncached_zeros((16,), torch.int32, dev)   # [0] the consumer's ack
        self.f_prod = uncached_zeros((16,), torch.int32, dev)  # [0] the producer's ack
        self.slots_in = uncached_zeros((nslot, 8, K), torch.bfloat16, dev)
        self.slots_out = uncached_zeros((nslot, 8, N),
                                        torch.float32 if out_f32 else torch.bfloat16, dev)
        self.sync = torch.zeros(2 * nslot + 4, dtype=torch.int32, device=dev)
        self.hp, self.dp = self.n.host_alloc_mapped(64)
        self.ctl = np.ctypeslib.as_array((ctypes.c_uint32 * 16).from_address(self.hp))
        self.s_ptr = self.n.stream_create_dedicated()
        self.s = torch.cuda.ExternalStream(self.s_ptr, device=dev)
        self.side = torch.cuda.Stream(dev)
        self.epoch = 0

    def __enter__(self):
        self._prev = torch.cuda.current_stream(self.dev)
        torch.cuda.set_stream(self.side)
        return self

    def __exit__(self, *exc):
        try:
            self.ctl[0] = 1  # the kernel returns within ~20 us of waiting
            self.s.synchronize()
        finally:
            torch.cuda.set_stream(self._prev)
        self.n.host_free(self.hp)
        self.n.stream_destroy(self.s_ptr)

    def launch(self, start, idle=5.0, timeout=2.0, **kw):
        self.epoch += 1
        self.ctl[0] = 0
        es = self.slots_out.element_size()
        args = dict(w=self.q.data_ptr(), ldw=self.q.stride(0), K=self.K,
                    w_scale=self.scale.data_ptr())
        args.update(kw)
        return self.n.chain_stage_run(
            self.s.cuda_stream, self.f_in.data_ptr(), self.f_in.data_ptr() + 64,
            self.slots_in.data_ptr(), self.K, self.f_prod.data_ptr(), args["w"], args["ldw"],
            self.bias.data_ptr(), _act(self.act), self.n_out, args["K"], int(self.out_f32),
            self.slots_out.data_ptr(), 8 * self.N * es, self.N, self.f_out.data_ptr() + 64, 2,
            self.f_out.data_ptr(), self.f_ack.data_ptr(), self.dp, self.dp + 4,
            self.sync.data_ptr(), start, self.epoch, 1, self.nslot, 8, idle, timeout,
            w_scale=args["w_scale"])

    def feed(self, seq, x, status=0):
        slot = seq % self.nslot
        rows = x.shape[0]
        self.slots_in[slot, :rows].copy_(x)
        self.f_in[16 + 2 * slot:18 + 2 * slot] = torch.tensor([status, rows], dtype=torch.int32,
                                                              device=self.dev)
        torch.cuda.current_stream(self.dev).synchronize()
        self.f_in[slot] = seq
        torch.cuda.current_stream(self.dev).synchronize()

    def wait_out(self, seq, limit=10.0):
        slot = seq % self.nslot
        t0 = time.monotonic()
        while int(self.f_out[slot]) != seq:
            assert time.monotonic() - t0 < limit, f"request {seq} never reached the consumer"
            time.sleep(1e-3)
        return self.f_out[16 + 2 * slot:18 + 2 * slot].tolist(), self.slots_out[slot].clone()


@pytest.mark.timeout(120)
def test_fp8_persistent_stage_relu(dev):
    """K = 2064 (one step past the two-chunk sweep), N = 200 (no multiple of the neuron group:
    the n0 + j < N guard), exact-sum operands on padded codes: ONE launch serves 1, 3, 8, 2 and
    5 rows, each EQUAL to the fp64 oracle and bitwise ops.gemv_fp8; an upstream status travels
    on with no rows written; the stop word ends the launch within 1 s; a relaunch from `done`
    continues; the counters are left at zero."""
    K, N = 2064, 200
    x, _, w, q, scale, bias = gc.operands(N, K)
    qv = gc.padded_codes(q, dev)
    sv, bv = scale.float().to(dev), bias.float().to(dev)
    xb = x.to(torch.bfloat16).to(dev)
    reqs = [(1, 0), (3, 1), (8, 0), (2, 4), (5, 3)]  # rows, first row of x
    # the references first: nothing slow runs between two requests (the idle timer)
    refs = []
    for rows, off in reqs + [(3, 5)]:
        y = torch.empty(rows, N, dtype=torch.bfloat16, device=dev)
        ops.gemv_fp8(xb[off:off + rows], qv, sv, bv, y, act="relu")
        z = gc.oracle_z(x[off:off + rows], w, scale, bias, rows, N)
        refs.append((y, ao.act_fwd(z, "relu")))
    torch.cuda.synchronize(dev)
    with _Stage(dev, qv, sv, bv, K, N, "relu") as st:
        assert st.launch(0) == 13  # ceil(200 / 16) workgroups
        seq = 0
        for (rows, off), (y, ref) in zip(reqs, refs):
            seq += 1
            st.feed(seq, xb[off:off + rows])
            hdr, out = st.wait_out(seq)
            assert hdr == [0, rows], (seq, hdr)
            ao.assert_bf16_close(out[:rows], ref, 0, f"request {seq} ({rows} rows)")
            assert torch.equal(out[:rows], y), f"request {seq} ({rows} rows) is not gemv_fp8's"
            assert int(st.f_prod[0]) == seq and int(st.ctl[1]) == seq
            st.f_ack[0] = seq  # the consumer drained it
        # an upstream failure (stage 0 blamed for a deadline) travels on, no rows written
        seq += 1
        st.slots_out[seq % st.nslot].zero_()
        st.feed(seq, xb[:2], status=4 | (0 << 8))
        hdr, out = st.wait_out(seq)
        assert hdr == [4, 2] and float(out.float().abs().sum()) == 0.0
        st.f_ack[0] = seq
        # the host's stop word ends the launch promptly
        t0 = time.monotonic()
        st.ctl[0] = 1
        st.s.synchronize()
        assert time.monotonic() - t0 < 1.0
        done = int(st.ctl[1])
        assert done == seq
        # a relaunch from the progress counter continues
        st.launch(done)
        seq += 1
        st.feed(seq, xb[5:8])
        hdr, out = st.wait_out(seq)
        assert hdr == [0, 3] and torch.equal(out[:3], refs[-1][0])
        ao.assert_bf16_close(out[:3], refs[-1][1], 0, "after the relaunch")
        st.ctl[0] = 1
        st.s.synchronize()
        assert st.sync[:st.nslot].tolist() == [0] * st.nslot  # counters left at zero


@pytest.mark.timeout(120)
def test_fp8_persistent_stage_at_the_lds_limit(dev):
    """K = 4096 at 8 rows fills the 64 KiB of LDS a persistent stage may use: random operands,
    N = 64, 8 rows bitwise ops.gemv_fp8 -- and 1, 2 and 3 rows after them, so that every row
    capacity of the stage kernel meets inexact sums once."""
    K, N = 4096, 64
    x, q, s, b = _random_layer(dev, N, K, 4096)
    sizes = (8, 1, 2, 3)
    refs = []
    for rows in sizes:
        refs.append(torch.empty(rows, N, dtype=torch.bfloat16, device=dev))
        ops.gemv_fp8(x[8 - rows:], q, s, b, refs[-1], act="relu")
    torch.cuda.synchronize(dev)
    with _Stage(dev, q, s, b, K, N, "relu") as st:
        assert st.launch(0) == 4
        for seq, (rows, ref) in enumerate(zip(sizes, refs), start=1):
            st.feed(seq, x[8 - rows:])
            hdr, out = st.wait_out(seq)
            assert hdr == [0, rows] and torch.equal(out[:rows], ref), f"{rows} rows"
            st.f_ack[0] = seq


@pytest.mark.timeout(120)
def test_fp8_persistent_softmax_last_stage(dev):
    """The last stage's persistent kernel over fp8 weights: one workgroup, fp32 rows, the row
    softmax over the n_out real outputs against torch.softmax of ops.gemv_fp8's fp32 linear
    output (only __expf separates the two: the existing persistent-softmax bound)."""
    K, N, n_out = 1024, 64, 10
    x, q, s, b = _random_layer(dev, N, K, 5)
    sizes = (1, 8, 3)
    refs = []
    for rows in sizes:
        z = torch.empty(rows, N, dtype=torch.float32, device=dev)
        ops.gemv_fp8(x[:rows], q, s, b, z, act="linear")
        refs.append(torch.softmax(z[:, :n_out], dim=1))
    torch.cuda.synchronize(dev)
    got = []
    with _Stage(dev, q, s, b, K, N, "softmax", out_f32=True, n_out=n_out) as st:
        assert st.launch(0) == 1
        for seq, rows in enumerate(sizes, start=1):
            st.feed(seq, x[:rows])
            got.append(st.wait_out(seq))
            st.f_ack[0] = seq
    for rows, ref, (hdr, out) in zip(sizes, refs, got):
        assert hdr == [0, rows]
        torch.testing.assert_close(out[:rows, :n_out], ref, atol=1e-5, rtol=1e-4)


def test_fp8_chain_launchers_reject_bad_operands(dev):
    """K = 24 (no multiple of 16), a misaligned w and an ldw that is no multiple of 16 raise in
    both launchers, and nothing is launched: every flag stays 0."""
    K, N = 32, 8
    x, q, s, b = _random_layer(dev, N, K, 1)
    wide = torch.zeros(N, K + 8, dtype=torch.uint8, device=dev)
    bad = [dict(K=24), dict(w=q.data_ptr() + 8), dict(ldw=K + 8, w=wide.data_ptr())]
    hop = _Hop(dev, N, False)
    for kw in bad:
        with pytest.raises(RuntimeError):
            hop.send(x, q, s, b, "relu", 2, kw.get("K", K), 1, ldw=kw.get("ldw"), w=kw.get("w"))
    torch.cuda.synchronize(dev)
    assert hop.flags_c.tolist() == [0] * 64 and hop.counter.tolist() == [0, 0, 0, 0]
    with _Stage(dev, q, s, b, K, N, "relu") as st:
        for kw in bad:
            with pytest.raises(RuntimeError):
                st.launch(0, **kw)
        st.s.synchronize()
        assert st.f_out.tolist() == [0] * 64 and st.sync.tolist() == [0] * (2 * st.nslot + 4)


# ---- end to end -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model4_fp8(tmp_path_factory):
    """The fixture model of test_chain_fast_gpu.py (784-256-128-64-10, relu x3 + softmax) as
    two configurations, and its fp64 reference layers: dequant_ref(quant_ref(bf16 weight))."""
    d = tmp_path_factory.mktemp("fast_fp8")
    rng = np.random.default_rng(3)
    dims = [784, 256, 128, 64, 10]
    acts = ["relu", "relu", "relu", "softmax"]
    ws = [rng.standard_normal((dims[i + 1], dims[i])) * (2.0 / np.sqrt(dims[i])) for i in range(4)]
    bs = [rng.standard_normal(dims[i + 1]) * 0.1 for i in range(4)]
    cfgs = {}
    for name, dist in (("a", [1, 1, 1, 1]), ("b", [2, 1, 1])):
        cfgs[name] = d / f"model4_{name}.json"
        export_model_json(str(cfgs[name]), ws, bs, acts, layer_distribution=dist)
    x = rng.random((64, 784))
    inp = d / "inputs4.json"
    write_examples(str(inp), x, np.zeros(64, dtype=np.int64))
    ref = []
    for L in load_model_config(str(cfgs["a"])).layers:
        wb = torch.as_tensor(np.asarray(L.weight, np.float32)).to(torch.bfloat16)
        q, s, _ = fo.quant_ref(wb)
        ref.append(LayerWeights(fo.dequant_ref(q, s).double().numpy(), L.bias, L.activation))
    return cfgs, inp, x, ref


@pytest.mark.timeout(240)
@pytest.mark.parametrize("form", ["persistent", "host_loop", "native_request"])
def test_fp8_rank_chain_takes_the_device_side_chain(model4_fp8, tmp_path, form):
    """--weights fp8 on a rank chain: (persistent) one layer per rank with the default
    switches -- persistent stages and the doorbell; (host_loop) [2, 1, 1] with
    DNN_CHAIN_PERSIST=0 -- a multi-layer stage 0 and one-launch hops; (native_request) one layer
    per rank with DNN_CHAIN_PERSIST=0 -- rank 0's native request (ChainHost). Requests of 1, 3,
    8, 40 (the message chain, stages paused) and 1 rows and 48 concurrent mixed-size requests
    match the fp64 forward over the oracle's dequantised weights within the bf16 chain's 2e-2 (the error
    sources are the same: bf16 activations); the log names the device-side chain and no host
    chain."""
    cfgs, inp, x, layers = model4_fp8
    cfg = cfgs["b" if form == "host_loop" else "a"]
    env = None if form == "persistent" else {"DNN_CHAIN_PERSIST": "0"}
    port = _port()
    p = _start(cfg, inp, port, tmp_path, env, args=("--weights", "fp8"))
    ok = False
    try:
        c = LayerClient(f"127.0.0.1:{port}", timeout=60)
        for rows in (1, 3, 8, 40, 1):
            q = x[:rows] if rows != 3 else x[10:13]
            np.testing.assert_allclose(c.process(q), model_forward(layers, q), atol=2e-2)
        chunks = [x[i:i + 1 + i % 8] for i in range(48)]
        with ThreadPoolExecutor(8) as pool:
            outs = list(pool.map(c.process, chunks))
        for ch, out in zip(chunks, outs):
            np.testing.assert_allclose(out, model_forward(layers, ch), atol=2e-2)
        c.close()
        ok = True
    finally:
        out = _stop(p)
        if not ok:  # the servers' side of a failure
            print(out[-12000:])
    assert "device-side chain" in out, out[-3000:]
    assert "host chain" not in out, out[-3000:]
    assert "Shutdown complete." in out, out[-3000:]
