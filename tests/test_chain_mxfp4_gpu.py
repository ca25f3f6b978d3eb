"""The device-side serving chain over MXFP4 weights (csrc/kernels/chain.hip with ``w_e8m0``,
serve/fastpath.py): the fused layer-and-send and the persistent stage kernel read e2m1 codes and
their e8m0 block scales in place and must write, bit for bit, what ops.gemv_mxfp4 writes -- in
that kernel's unit for the request's rows and K, a whole block for 1 and 2 rows at K >= 2048,
half a block otherwise -- and on the exact-sum operands of _gemv_mxfp4_cases.py the fp64 value
itself. Then a 4-rank mxfp4 chain on one GPU with ``--mxfp4-chain device``, persistent stages,
host loop and native request, against the fp64 forward over the oracle's dequantised weights.
Every wait is bounded by the kernels' own timeouts."""
import ctypes
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import _act_oracle as ao
import _chain_mxfp4_cases as cc
import _gemv_mxfp4_cases as gc
import _mxfp4_oracle as mo
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

    def send(self, x, q, e, bias, act, rows, K, seq, ack_target=0, timeout=2.0, **kw):
        """``kw`` replaces an operand of the launch: w, ldw, lde, w_scale."""
        fp, fc = self.flags_p.data_ptr(), self.flags_c.data_ptr()
        self.n.chain_gemv_send(
            self.s.cuda_stream, x.data_ptr(), x.stride(0), kw.get("w", q.data_ptr()),
            kw.get("ldw", q.stride(0)), bias.data_ptr(), _act(act), rows, self.N, K,
            int(self.f32), self.slot.data_ptr(), self.N, fc + 8, 0, fp + 36, 0, 0, fp + 32,
            ack_target, fc, seq, 0, self.counter.data_ptr(), timeout,
            w_scale=kw.get("w_scale", 0), w_e8m0=e.data_ptr(), lde=kw.get("lde", e.stride(0)))


def _with_a_dead_row(N, K):
    """The exact-sum operands of (N, K) with row N - 1 made a row whose every block has E == 0
    over codes of 6.0: its weights are 0 whatever the codes hold. Copies: the shared operands
    stay as they are."""
    x, _, w, q, e, bias = gc.operands(N, K)
    q, e, w = q.clone(), e.clone(), w.clone()
    q[N - 1], e[N - 1], w[N - 1] = gc.Q_JUNK, 0, 0.0
    return x, w, q, e, bias


@pytest.mark.parametrize("N,K", [(5, 1056), (10, 832), (3, 2080), (4, 2048), (2, 2016),
                                 (7, 4096)])
def test_mxfp4_fused_send_equals_fp64_oracle(dev, N, K):
    """chain_gemv_send(w_e8m0=...) on exact-sum operands, codes and scale bytes on padded views
    (ldw > K / 2, lde > K / 32): the slot rows EQUAL act(x . w^T + bias) in fp64 for 1, 2, 3, 5
    and 8 rows, relu and linear, bf16 and fp32 slots -- no tolerance, every partial sum is
    exact; a row whose blocks all have E == 0 over codes of 6.0 gives act(bias); rows past the
    request stay untouched; header, flag and counter end as in the fp8 test; a consumer that
    never acks is blamed and no rows are written."""
    x, w, q, e, bias = _with_a_dead_row(N, K)
    qv, ev = gc.padded_codes(q, dev), gc.padded_scales(e, dev)
    assert qv.stride(0) > K // 2 and qv.stride(0) % 16 == 0 and qv.data_ptr() % 16 == 0
    assert ev.stride(0) > K // 32
    bv = bias.float().to(dev)
    _, xv = ao.padded(8, K, torch.bfloat16, float("nan"), dev, x)
    for f32 in (False, True):
        hop = _Hop(dev, N, f32)
        seq = 0
        for rows in (1, 2, 3, 5, 8):
            for act in ("relu", "linear"):
                seq += 1
                hop.slot.zero_()
                torch.cuda.synchronize(dev)
                hop.send(xv, qv, ev, bv, act, rows, K, seq)
                torch.cuda.synchronize(dev)
                ref = ao.act_fwd(gc.oracle_z(x, w, bias, rows, N), act)
                what = f"fused mxfp4 send {rows}x{N}x{K} {act} f32={f32}"
                got = hop.slot.cpu()
                if f32:
                    assert torch.equal(got[:rows].double(), ref), f"{what}: not the exact sum"
                else:
                    ao.assert_bf16_close(got[:rows], ref, 0, what)
                # every block of the last row has E == 0: the codes of 6.0 do not matter
                assert torch.equal(got[:rows, N - 1].double(),
                                   ao.act_fwd(bias[N - 1], act).expand(rows)), what
                assert float(got[rows:].float().abs().sum()) == 0.0, f"{what}: wrote past rows"
                assert int(hop.flags_c[0]) == seq and hop.flags_c[2:4].tolist() == [0, rows]
                assert hop.counter.tolist() == [0, 0, 0, 0]
        # the consumer never drained the slot (ack stays 0 < target): blamed (stage 0 + 1)
        seq += 1
        hop.slot.zero_()
        torch.cuda.synchronize(dev)
        hop.send(xv, qv, ev, bv, "relu", 3, K, seq, ack_target=seq, timeout=0.2)
        torch.cuda.synchronize(dev)
        assert int(hop.flags_c[0]) == seq and (int(hop.flags_c[2]) & 0xFF) == 4
        assert (int(hop.flags_c[2]) >> 8) & 0xFF == 1
        assert float(hop.slot.float().abs().sum()) == 0.0
        assert hop.counter.tolist() == [0, 0, 0, 0]


def _random_layer(dev, N, K):
    """_chain_mxfp4_cases.random_layer on the device: 8 bf16 input rows, codes, scale bytes,
    bias. Its fp32 linear outputs differ between the two lane orders
    (tests/test_chain_mxfp4_cpu.py shows it on the CPU emulation), its bf16 outputs do not: the
    comparisons that pin the order are fp32 and linear."""
    return tuple(t.to(dev) for t in cc.random_layer(N, K))


def _f32_linear_ref(x, q, e, b, rows):
    """ops.gemv_mxfp4's fp32 linear output: the sum in its lane order plus the bias, unrounded
    any further."""
    ref = torch.empty(rows, q.shape[0], dtype=torch.float32, device=x.device)
    ops.gemv_mxfp4(x[:rows], q, e, b, ref, act="linear")
    return ref


@pytest.mark.parametrize("N,K,rows", [(1024, 832, 1), (1024, 832, 3), (1024, 832, 8),
                                      (64, 2080, 1), (64, 2080, 2), (64, 2080, 3)])
def test_mxfp4_fused_send_random_equals_gemv_mxfp4(dev, N, K, rows):
    """Random operands, so the sums are inexact and the lane order shows -- in an fp32 slot of a
    linear layer, which is bitwise ops.gemv_mxfp4's fp32 output (in bf16 the two orders agree on
    these operands, so the bf16 relu slot, compared too, pins the epilogue and not the order).
    K = 832, N = 1024 (256 workgroups) on the half-block unit at 1, 3 and 8 rows; K = 2080 on
    the whole-block unit at 1 and 2 rows and on the half-block unit at 3."""
    assert (N, K) in cc.FUSED
    x, q, e, b = _random_layer(dev, N, K)
    ref32 = _f32_linear_ref(x, q, e, b, rows)
    ref16 = torch.empty(rows, N, dtype=torch.bfloat16, device=dev)
    ops.gemv_mxfp4(x[:rows], q, e, b, ref16, act="relu")
    for f32, act, ref in ((True, "linear", ref32), (False, "relu", ref16)):
        hop = _Hop(dev, N, f32)
        hop.send(x, q, e, b, act, rows, K, 1)
        torch.cuda.synchronize(dev)
        assert torch.equal(hop.slot[:rows], ref), f"f32={f32}: not gemv_mxfp4's rows"
        assert int(hop.flags_c[0]) == 1 and hop.flags_c[2:4].tolist() == [0, rows]
        assert hop.counter.tolist() == [0, 0, 0, 0]
    # and the CPU emulation of that order for this request's unit gives the same bits
    emu = cc.emulate(x[:rows].cpu(), q.cpu(), e.cpu(), b.cpu(), cc.unit(rows, K))
    assert np.array_equal(ref32.cpu().numpy(), emu), f"not the order of unit {cc.unit(rows, K)}"


def test_mxfp4_one_launch_hop_equals_gemv_mxfp4(dev):
    """The folded receive (in_flag) over mxfp4 weights at K = N = 1024, 2 rows: x is read from
    the L2-uncached slot once its flag is up, the fp32 linear rows are bitwise
    ops.gemv_mxfp4's fp32 output (fp32, so that the lane order shows), the producer is acked.
    The kernel is enqueued before its input exists and spins, so like a persistent stage it gets
    a stream with a hardware queue of its own: on a queue it shared with the stream that feeds
    it, the feed would wait behind it until its timeout (2 s: bounded)."""
    n = native()
    (N, K), rows = cc.FOLDED, 2
    x, q, e, b = _random_layer(dev, N, K)
    ref = _f32_linear_ref(x, q, e, b, rows)
    f_in = uncached_zeros((64,), torch.int32, dev)    # this stage: [0] flag, [2:4] header
    f_out = uncached_zeros((64,), torch.int32, dev)   # consumer: [0] flag, [2:4] header
    f_prod = uncached_zeros((64,), torch.int32, dev)  # producer: [8] ack
    slot_in = uncached_zeros((8, K), torch.bfloat16, dev)
    slot_out = uncached_zeros((8, N), torch.float32, dev)
    err = torch.zeros(4, dtype=torch.int32, device=dev)
    counter = torch.zeros(4, dtype=torch.int32, device=dev)
    s_ptr = n.stream_create_dedicated()
    st = torch.cuda.ExternalStream(s_ptr, device=dev)
    torch.cuda.synchronize(dev)
    n.chain_gemv_send(st.cuda_stream, slot_in.data_ptr(), K, q.data_ptr(), q.stride(0),
                      b.data_ptr(), _act("linear"), rows, N, K, 1, slot_out.data_ptr(), N,
                      f_out.data_ptr() + 8, f_in.data_ptr() + 8, err.data_ptr(), 1, 0, 0, 0,
                      f_out.data_ptr(), 1, f_prod.data_ptr() + 32, counter.data_ptr(), 2.0,
                      in_flag=f_in.data_ptr(), w_e8m0=e.data_ptr(), lde=e.stride(0))
    # enqueued before its input exists: it waits on stream st. The writes below go through a
    # side stream, as in _Stage: the default stream would wait for st, and there is no
    # device-wide sync while the kernel spins
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        slot_in.copy_(x)
        f_in[2:4] = torch.tensor([0, rows], dtype=torch.int32, device=dev)
        side.synchronize()
        f_in[0] = 1  # the producer's flag
        side.synchronize()
    st.synchronize()
    n.stream_destroy(s_ptr)
    assert int(f_out[0]) == 1 and f_out[2:4].tolist() == [0, rows], f_out[:4].tolist()
    assert torch.equal(slot_out[:rows], ref)
    assert int(f_prod[8]) == 1 and counter.tolist() == [0, 0, 0, 0]


# ---- the persistent stage ---------------------------------------------------------------------

class _Stage:
    """A persistent mxfp4 stage kernel (chain_stage_run with w_e8m0) between a simulated
    producer (feed: input slot, header, flag) and a simulated consumer (wait_out, the ack word).
    The kernel has a dedicated stream; the test's own work runs on a side stream (`with st:`),
    and leaving the block sets the stop word first, so a failing assertion never leaves the
    kernel waiting for its idle timer."""

    def __init__(self, dev, q, e, bias, K, N, act, nslot=4, out_f32=False, n_out=None):
        self.n, self.dev = native(), dev
        self.q, self.e, self.bias = q, e, bias
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
        """``kw`` replaces an operand of the launch: w, ldw, lde, K, w_scale."""
        self.epoch += 1
        self.ctl[0] = 0
        es = self.slots_out.element_size()
        args = dict(w=self.q.data_ptr(), ldw=self.q.stride(0), K=self.K, w_scale=0,
                    lde=self.e.stride(0))
        args.update(kw)
        return self.n.chain_stage_run(
            self.s.cuda_stream, self.f_in.data_ptr(), self.f_in.data_ptr() + 64,
            self.slots_in.data_ptr(), self.K, self.f_prod.data_ptr(), args["w"], args["ldw"],
            self.bias.data_ptr(), _act(self.act), self.n_out, args["K"], int(self.out_f32),
            self.slots_out.data_ptr(), 8 * self.N * es, self.N, self.f_out.data_ptr() + 64, 2,
            self.f_out.data_ptr(), self.f_ack.data_ptr(), self.dp, self.dp + 4,
            self.sync.data_ptr(), start, self.epoch, 1, self.nslot, 8, idle, timeout,
            w_scale=args["w_scale"], w_e8m0=self.e.data_ptr(), lde=args["lde"])

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
def test_mxfp4_persistent_stage_relu(dev):
    """K = 2080 (one block past a chunk of either unit), N = 200 (no multiple of the neuron
    group: the n0 + j < N guard), exact-sum operands on padded codes and scale bytes: ONE launch
    serves 1, 3, 8, 2 and 5 rows -- 1 and 2 on the whole-block unit, 3, 5 and 8 on the half-block
    unit -- each EQUAL to the fp64 oracle and bitwise ops.gemv_mxfp4; an upstream status travels
    on with no rows written; the stop word ends the launch within 1 s; a relaunch from `done`
    continues; the counters are left at zero."""
    K, N = 2080, 200
    assert K >= 2048  # rows 1 and 2 take the whole-block unit (gemv_mxfp4's rule)
    x, _, w, q, e, bias = gc.operands(N, K)
    qv, ev = gc.padded_codes(q, dev), gc.padded_scales(e, dev)
    bv = bias.float().to(dev)
    xb = x.to(torch.bfloat16).to(dev)
    reqs = [(1, 0), (3, 1), (8, 0), (2, 4), (5, 3)]  # rows, first row of x
    # the references first: nothing slow runs between two requests (the idle timer)
    refs = []
    for rows, off in reqs + [(3, 5)]:
        y = torch.empty(rows, N, dtype=torch.bfloat16, device=dev)
        ops.gemv_mxfp4(xb[off:off + rows], qv, ev, bv, y, act="relu")
        z = gc.oracle_z(x[off:off + rows], w, bias, rows, N)
        refs.append((y, ao.act_fwd(z, "relu")))
    torch.cuda.synchronize(dev)
    with _Stage(dev, qv, ev, bv, K, N, "relu") as st:
        assert st.launch(0) == 13  # ceil(200 / 16) workgroups
        seq = 0
        for (rows, off), (y, ref) in zip(reqs, refs):
            seq += 1
            st.feed(seq, xb[off:off + rows])
            hdr, out = st.wait_out(seq)
            assert hdr == [0, rows], (seq, hdr)
            ao.assert_bf16_close(out[:rows], ref, 0, f"request {seq} ({rows} rows)")
            assert torch.equal(out[:rows], y), f"request {seq} ({rows} rows) is not gemv_mxfp4's"
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
def test_mxfp4_persistent_stage_at_the_lds_limit(dev):
    """K = 4096 at 8 rows fills the 64 KiB of LDS a persistent stage may use: random operands,
    N = 64, a linear layer into fp32 slots, so that the lane order shows: 8 rows bitwise
    ops.gemv_mxfp4's fp32 output -- and 1, 2 (the whole-block unit) and 3 rows after them, so
    that every row capacity and both units of the stage kernel meet inexact sums once."""
    N, K = cc.LDS_LIMIT
    x, q, e, b = _random_layer(dev, N, K)
    sizes = (8, 1, 2, 3)
    refs = [_f32_linear_ref(x, q, e, b, rows) for rows in sizes]
    torch.cuda.synchronize(dev)
    with _Stage(dev, q, e, b, K, N, "linear", out_f32=True) as st:
        assert st.launch(0) == 4
        for seq, (rows, ref) in enumerate(zip(sizes, refs), start=1):
            st.feed(seq, x[:rows])
            hdr, out = st.wait_out(seq)
            assert hdr == [0, rows] and torch.equal(out[:rows], ref), f"{rows} rows"
            st.f_ack[0] = seq


@pytest.mark.timeout(120)
def test_mxfp4_persistent_softmax_last_stage(dev):
    """The last stage's persistent kernel over mxfp4 weights: one workgroup, fp32 rows, the row
    softmax over the n_out real outputs against torch.softmax of ops.gemv_mxfp4's fp32 linear
    output (only __expf separates the two: the existing persistent-softmax bound)."""
    K, N, n_out = 1024, 64, 10
    x, q, e, b = _random_layer(dev, N, K)
    sizes = (1, 8, 3)
    refs = []
    for rows in sizes:
        z = torch.empty(rows, N, dtype=torch.float32, device=dev)
        ops.gemv_mxfp4(x[:rows], q, e, b, z, act="linear")
        refs.append(torch.softmax(z[:, :n_out], dim=1))
    torch.cuda.synchronize(dev)
    got = []
    with _Stage(dev, q, e, b, K, N, "softmax", out_f32=True, n_out=n_out) as st:
        assert st.launch(0) == 1
        for seq, rows in enumerate(sizes, start=1):
            st.feed(seq, x[:rows])
            got.append(st.wait_out(seq))
            st.f_ack[0] = seq
    for rows, ref, (hdr, out) in zip(sizes, refs, got):
        assert hdr == [0, rows]
        torch.testing.assert_close(out[:rows, :n_out], ref, atol=1e-5, rtol=1e-4)


def test_mxfp4_chain_launchers_reject_bad_operands(dev):
    """K = 48 (no whole blocks), a w 8 bytes off its alignment, an ldw that is no multiple of
    16, an lde below K / 32, and fp8 row scales together with block scales raise in both
    launchers, and nothing is launched: every flag stays 0."""
    K, N = 64, 8
    x, q, e, b = _random_layer(dev, N, K)
    wide = torch.zeros(N, K // 2 + 8, dtype=torch.uint8, device=dev)
    scale = torch.ones(N, dtype=torch.float32, device=dev)
    bad = [dict(K=48), dict(w=q.data_ptr() + 8), dict(ldw=K // 2 + 8, w=wide.data_ptr()),
           dict(lde=K // 32 - 1), dict(w_scale=scale.data_ptr())]
    hop = _Hop(dev, N, False)
    for kw in bad:
        kw = dict(kw)
        with pytest.raises(RuntimeError):
            hop.send(x, q, e, b, "relu", 2, kw.pop("K", K), 1, **kw)
    torch.cuda.synchronize(dev)
    assert hop.flags_c.tolist() == [0] * 64 and hop.counter.tolist() == [0, 0, 0, 0]
    with _Stage(dev, q, e, b, K, N, "relu") as st:
        for kw in bad:
            with pytest.raises(RuntimeError):
                st.launch(0, **kw)
        st.s.synchronize()
        assert st.f_out.tolist() == [0] * 64 and st.sync.tolist() == [0] * (2 * st.nslot + 4)


# ---- end to end -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model4_mxfp4(tmp_path_factory):
    """The fixture model of test_chain_fast_gpu.py (784-256-128-64-10, relu x3 + softmax) as
    two configurations, and its fp64 reference layers: the oracle's values of
    quant_ref(padded bf16 weight)."""
    d = tmp_path_factory.mktemp("fast_mxfp4")
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
        # blocks are 32 columns of the PADDED row (a multiple of 64), as the stage quantises
        w = np.asarray(L.weight, np.float32)
        wp = torch.zeros(w.shape[0], -(-w.shape[1] // 64) * 64)
        wp[:, :w.shape[1]] = torch.as_tensor(w)
        q, e, _ = mo.quant_ref(wp.to(torch.bfloat16))
        ref.append(LayerWeights(mo.values(q, e)[:, :w.shape[1]], L.bias, L.activation))
    return cfgs, inp, x, ref


def _serve_and_check(cfg, inp, x, layers, tmp_path, env, args):
    port = _port()
    p = _start(cfg, inp, port, tmp_path, env, args=args)
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
    return out


@pytest.mark.timeout(240)
@pytest.mark.parametrize("form", ["persistent", "host_loop", "native_request"])
def test_mxfp4_rank_chain_takes_the_device_side_chain(model4_mxfp4, tmp_path, form):
    """--weights mxfp4 --mxfp4-chain device on a rank chain: (persistent) one layer per rank
    with the default switches -- persistent stages and the doorbell; (host_loop) [2, 1, 1] with
    DNN_CHAIN_PERSIST=0 -- a multi-layer stage 0 and one-launch hops; (native_request) one layer
    per rank with DNN_CHAIN_PERSIST=0 -- rank 0's native request (ChainHost). Requests of 1, 3,
    8, 40 (the message chain, stages paused) and 1 rows and 48 concurrent mixed-size requests
    match the fp64 forward over the oracle's dequantised weights within the bf16 chain's 2e-2
    (the error sources are the same: bf16 activations); the log names the device-side chain and
    no host chain."""
    cfgs, inp, x, layers = model4_mxfp4
    cfg = cfgs["b" if form == "host_loop" else "a"]
    env = None if form == "persistent" else {"DNN_CHAIN_PERSIST": "0"}
    out = _serve_and_check(cfg, inp, x, layers, tmp_path, env,
                           ("--weights", "mxfp4", "--mxfp4-chain", "device"))
    assert "device-side chain" in out, out[-3000:]
    assert "host chain" not in out, out[-3000:]
    assert "Shutdown complete." in out, out[-3000:]


@pytest.mark.timeout(240)
def test_mxfp4_rank_chain_defaults_to_the_host_chain(model4_mxfp4, tmp_path):
    """Without --mxfp4-chain the same chain answers the same requests within the same bound on
    the host chain and logs why."""
    cfgs, inp, x, layers = model4_mxfp4
    out = _serve_and_check(cfgs["a"], inp, x, layers, tmp_path, None, ("--weights", "mxfp4"))
    assert "host chain: the device-side chain reads mxfp4 weights only with" in out, out[-3000:]
    assert "device-side chain (" not in out, out[-3000:]
    assert "Shutdown complete." in out, out[-3000:]
