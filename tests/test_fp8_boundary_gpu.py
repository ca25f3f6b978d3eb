"""quant_rows_fp8_kernel / dequant_rows_fp8_kernel (csrc/kernels/elementwise.hip) against the
exact oracle of the hop format (tests/_fp8_oracle.py): codes, scales and bf16 output bit for bit,
with no allowance -- on contiguous tensors, on the row slices of wider buffers the engine
passes, through a Stage's pack / unpack methods, on tiny rows and on non-finite inputs.

Result on MI355X: the kernel's `448.f / amax` is the IEEE quotient and v_cvt_pk_fp8_f32 rounds
exact ties to the even code, so no tie exception exists: all 252 ties of the exhaustive row set
equal the oracle."""
import numpy as np
import pytest
import torch

import _act_oracle as ao
import _fp8_oracle as fo
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.utils.native import native

pytestmark = pytest.mark.gpu

Q_FILL, S_FILL = 0x55, -7.0


def _gpu_quant(x, dev):
    rows, cols = x.shape
    q = torch.full((rows, cols), Q_FILL, dtype=torch.uint8, device=dev)
    s = torch.full((rows,), S_FILL, device=dev)
    ops.quant_rows_fp8(x.to(dev), q, s)
    return q.cpu(), s.cpu()


def _gpu_dequant(q, s, like, dev):
    y = torch.full(like.shape, ao.SENTINEL, dtype=torch.bfloat16, device=dev)
    ops.dequant_rows_fp8(torch.as_tensor(q).to(dev), torch.as_tensor(s).to(dev), y)
    return y.cpu()


def _assert_quant(q, s, q_ref, s_ref, what):
    q, q_ref = np.asarray(q), np.asarray(q_ref)
    bad_s = (fo.bits32(s) != fo.bits32(s_ref)).nonzero()[0]
    assert bad_s.size == 0, (f"{what}: {bad_s.size} scales differ, first row {bad_s[0]}: "
                             f"{float(s[bad_s[0]])!r} != {float(s_ref[bad_s[0]])!r}")
    diff = q != q_ref
    assert not diff.any(), (f"{what}: {int(diff.sum())} of {diff.size} codes differ, first at "
                            f"{np.argwhere(diff)[:4].tolist()}: {q[diff][:4]} != {q_ref[diff][:4]}")


def test_tiny_row_constant_is_shared():
    assert native().fp8_tiny_amax() == ops.FP8_TINY_AMAX == float(fo.TINY_AMAX)


@pytest.mark.parametrize("name", fo.CASES)
def test_kernels_equal_oracle(dev, name):
    """GPU codes and scales = quant_ref; GPU dequantisation of the oracle's codes = dequant_ref;
    the round trip through both kernels within the format's bound."""
    x = fo.case(name)
    q_ref, s_ref, tie, y_ref = fo.reference(name)
    q, s = _gpu_quant(x, dev)
    _assert_quant(q, s, q_ref, s_ref, name)
    y = _gpu_dequant(q_ref, s_ref, x, dev)
    assert torch.equal(fo.bits16(y), fo.bits16(y_ref)), f"{name}: dequantised bf16"
    ratio = fo.assert_round_trip(x, _gpu_dequant(q, s, x, dev), name)
    print(f"\nfp8 {name}: {x.numel()} elements, {int(tie.sum())} exact ties, "
          f"round trip at {ratio:.3f} x the bound")


def _window(rows, cols, dtype, fill, dev, pad_c, start):
    """(buffer, view): ``rows`` rows from row ``start`` of a [rows + 13][cols] window that lies
    at (PAD, pad_c) of a sentinel-filled buffer with row stride cols + 3 * pad_c -- what a
    micro-batch slice of a wider engine buffer looks like, as _act_oracle.padded builds it."""
    buf = torch.full((rows + 13 + 2 * ao.PAD, cols + 3 * pad_c), fill, dtype=dtype, device=dev)
    r0 = ao.PAD + start
    return buf, buf[r0:r0 + rows, pad_c:pad_c + cols]


def _assert_outside_untouched(buf, view, fill, what):
    r0 = (view.data_ptr() - buf.data_ptr()) // buf.element_size() // buf.stride(0)
    c0 = (view.data_ptr() - buf.data_ptr()) // buf.element_size() % buf.stride(0)
    outside = torch.ones(buf.shape, dtype=torch.bool)
    outside[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = False
    assert bool((buf.cpu()[outside] == fill).all()), f"{what}: wrote outside the slice"


@pytest.mark.parametrize("rows,cols,start", [(1, 8, 1), (5, 136, 5), (33, 520, 3), (7, 1032, 6)])
def test_row_slices_of_wider_buffers(dev, rows, cols, start):
    """x, q and the output are row slices (start row not a multiple of 4) of wider buffers
    (ldx > cols, ldq > cols; x and the output 16-byte aligned, q on the 8 bytes one lane
    stores), scale a slice of a longer vector: same bits, nothing outside the slice changes."""
    name = f"log6-{rows}x{cols}"
    x = fo.case(name)
    q_ref, s_ref, _, y_ref = fo.reference(name)
    xbuf, xv = _window(rows, cols, torch.bfloat16, float("nan"), dev, 8, start)
    xv.copy_(x)
    qbuf, qv = _window(rows, cols, torch.uint8, Q_FILL, dev, 16, start)
    sbuf = torch.full((rows + 16,), S_FILL, device=dev)
    sv = sbuf[7:7 + rows]
    assert xv.stride(0) > cols and qv.stride(0) > cols and xv.data_ptr() % 16 == 0
    ops.quant_rows_fp8(xv, qv, sv)
    _assert_quant(qv.cpu(), sv.cpu(), q_ref, s_ref, name)
    _assert_outside_untouched(qbuf, qv, Q_FILL, f"{name} q")
    assert bool((sbuf[:7] == S_FILL).all()) and bool((sbuf[7 + rows:] == S_FILL).all())
    ybuf, yv = _window(rows, cols, torch.bfloat16, ao.SENTINEL, dev, 8, start)
    ops.dequant_rows_fp8(qv, sv, yv)
    assert torch.equal(fo.bits16(yv), fo.bits16(y_ref)), f"{name}: dequantised bf16"
    _assert_outside_untouched(ybuf, yv, ao.SENTINEL, f"{name} output")
    _assert_outside_untouched(qbuf, qv, Q_FILL, f"{name} q after dequant")
    assert torch.isnan(xbuf.cpu().float()).sum() == xbuf.numel() - rows * cols  # x unchanged


@pytest.mark.parametrize("cols", fo.WIDTHS)
def test_finite_rows_stay_finite(dev, cols):
    """Tiny-row rule in the kernel: finite, non-negative scales, no NaN code, a finite round
    trip; the rows under 2^-110 (and only they and the zero row) arrive as zeros."""
    x = fo.case(f"special-{fo.N_SPECIAL}x{cols}")
    q, s = _gpu_quant(x, dev)
    assert bool(torch.isfinite(s).all()) and bool((s >= 0).all())
    assert not bool(((q & 0x7F) == 0x7F).any())
    y = _gpu_dequant(q, s, x, dev)
    assert bool(torch.isfinite(y.float()).all())
    for r in range(fo.N_SPECIAL):
        zero_row = bool((y[r] == 0).all()) and float(s[r]) == 0.0
        assert zero_row == (r in fo.SENT_AS_ZERO), r


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_inputs_do_not_come_back_finite(dev, bad):
    """A NaN or +-inf element dequantises to a non-finite value at its position; what happens
    to the rest of such a row is not specified (and differs between the CPU path and here)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(6, 520, generator=g).to(torch.bfloat16)
    x[1] = 0
    x[2] *= 1e-36  # a row under the threshold apart from its non-finite element
    where = [(0, 0), (1, 7), (2, 519), (4, 64), (4, 513)]
    for r, c in where:
        x[r, c] = bad
    q, s = _gpu_quant(x, dev)
    y = _gpu_dequant(q, s, x, dev).float()
    for r, c in where:
        assert not bool(torch.isfinite(y[r, c])), (r, c)
    for r in (3, 5):  # rows without one are unaffected
        assert bool(torch.isfinite(y[r]).all())


def test_stage_pack_unpack_equal_oracle(dev):
    """The engine's own calls: a middle Stage with the fp8 boundary on both sides, 2
    micro-batches of 64 rows, hop widths 64 (input side) and 192 (layer width 136, padded to the
    64-column tiles of the engine). pack_* of each micro-batch, the hop as a plain copy,
    unpack_*: every buffer equals the oracle row for row."""
    from docker_dist_nn_amd import MLPSpec
    from docker_dist_nn_amd.engine.stage import Stage

    st = Stage(MLPSpec.parse("32-64-136-10"), 1, 2, micro_batch=64, num_micro=2, device=dev,
               stage_index=1, num_stages=3)
    st.enable_fp8_boundary(True, True)
    assert st.output.shape == (128, 192) and st.dx_send.shape == (128, 64)
    g = torch.Generator().manual_seed(11)
    act = (torch.randn(128, 192, generator=g) * torch.logspace(-6, 6, 128)[:, None]).to(
        torch.bfloat16)
    dx = (torch.randn(128, 64, generator=g) * torch.logspace(6, -6, 128)[:, None]).to(
        torch.bfloat16)
    act[70], dx[3] = 0, 1e-37  # a zero row and a row under the threshold
    st.output.copy_(act)
    st.dx_send.copy_(dx)
    for j in range(2):
        st.pack_fwd(j)
        st.pack_bwd(j)
    for (x, q, s) in ((act, st.q_out, st.s_out), (dx, st.q_dx, st.s_dx)):
        q_ref, s_ref, _ = fo.quant_ref(x)
        _assert_quant(q.cpu(), s.cpu(), q_ref, s_ref, f"stage pack {tuple(x.shape)}")
    # the hop: what a neighbour packed arrives in this stage's receive buffers
    st.q_gin.copy_(st.q_out), st.s_gin.copy_(st.s_out)
    st.q_in.copy_(st.q_dx), st.s_in.copy_(st.s_dx)
    st.grad_out.fill_(ao.SENTINEL), st.x_in.fill_(ao.SENTINEL)
    for j in (1, 0):
        st.unpack_fwd(j)
        st.unpack_bwd(j)
    for (x, out) in ((act, st.grad_out), (dx, st.x_in)):
        q_ref, s_ref, _ = fo.quant_ref(x)
        assert torch.equal(fo.bits16(out), fo.bits16(fo.dequant_ref(q_ref, s_ref)))
        fo.assert_round_trip(x, out, f"stage round trip {tuple(x.shape)}")
