"""The MXFP4-weight serving GEMV (csrc/kernels/gemv_mxfp4.hip, ops.gemv_mxfp4) and the
quantiser / dequantiser kernels (csrc/kernels/mxfp4.hip) on the GPU, against the exact oracles
of _mxfp4_oracle.py (the format) and _act_oracle.py (the activations): operands and method in
_gemv_mxfp4_cases.py."""
import numpy as np
import pytest
import torch

import _act_oracle as ao
import _gemv_mxfp4_cases as gc
import _mxfp4_oracle as mo
from test_gemv_gpu import SIGMOID_F32_MAX_ULP
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.utils.native import native

pytestmark = pytest.mark.gpu

Q_FILL, E_FILL = 0x55, 0xEE


@pytest.mark.parametrize("N,K", gc.NK)
def test_gemv_mxfp4_equals_fp64_oracle(dev, N, K):
    """M = 1..8, every activation, fp32 and bf16 output, bias (longer than N) and None. fp32:
    linear / relu bit-equal to fp64, sigmoid within SIGMOID_F32_MAX_ULP of test_gemv_gpu.py
    (the same act_fwd runs on an exact z, so that measured bound carries over). bf16: linear /
    relu bit-equal to RN_bf16(fp64), sigmoid within 1 bf16 ulp. Nothing outside [M][N] is
    written; the junk around x, q, e and bias is never read."""
    worst = gc.check_exact_shape(ops.gemv_mxfp4, N, K, dev, SIGMOID_F32_MAX_ULP)
    print(f"\ngemv_mxfp4 N={N} K={K}: sigmoid fp32 worst {worst:.2f} ulp (bound "
          f"{SIGMOID_F32_MAX_ULP:g})")


def test_gemv_mxfp4_decodes_every_code_in_both_nibbles(dev):
    """Row n holds code n & 15 in column n >> 4 (0: a low nibble, 1: a high nibble) and zero
    codes elsewhere; x = [1, 3, 0, ...]: y[0][n] is (1 or 3) times the kernel's decode of the
    code, at E = 127, 128 and 120. Confirms on the device that the hardware conversion returns
    the low nibble as the even column. (Code 0x8, -0, arrives as the sum 0 + (-0) = +0.)"""
    code = np.zeros((32, 32), dtype=np.uint8)
    for n in range(32):
        code[n, n >> 4] = n & 15
    x = torch.zeros(1, 32, dtype=torch.bfloat16)
    x[0, 0], x[0, 1] = 1.0, 3.0
    q = torch.from_numpy(mo.pack(code)).to(dev)
    for E in (127, 128, 120):
        e = torch.full((32, 1), E, dtype=torch.uint8, device=dev)
        y = torch.full((1, 32), ao.SENTINEL, dtype=torch.float32, device=dev)
        ops.gemv_mxfp4(x.to(dev), q, e, None, y, "linear")
        want = np.concatenate([mo.DEC, 3.0 * mo.DEC]) * 2.0 ** (E - 127) + 0.0
        assert np.array_equal(y.cpu().numpy()[0].astype(np.float64), want), E


def test_gemv_mxfp4_zero_blocks_add_nothing(dev):
    gc.check_zero_blocks_add_nothing(ops.gemv_mxfp4, dev)


@pytest.mark.parametrize("N,K,M", gc.LAYERS)
def test_gemv_mxfp4_random_operands_within_derived_bound(dev, N, K, M):
    """Random bf16 x and weights through quant_ref, against the fp64 product with the ORIGINAL
    bf16 weights: |y - ref| <= |x| @ format_bound^T + summation_bound (gc.check_layer)."""
    w, b, x = gc.layer_case(N, K, M)
    q, e, _ = mo.quant_ref(w)
    _, xv = ao.padded(M, K, torch.bfloat16, float("nan"), dev, x)
    ybuf, yv = ao.padded(M, N, torch.float32, ao.SENTINEL, dev)
    ops.gemv_mxfp4(xv, gc.padded_codes(torch.from_numpy(q), dev),
                   gc.padded_scales(torch.from_numpy(e), dev), b.to(dev), yv, "linear")
    ratio = gc.check_layer(yv.cpu().double().numpy(), w, b, x)
    print(f"\ngemv_mxfp4 random {M}x{N}x{K}: error at {ratio:.3f} x the derived bound")
    ao.assert_padding_untouched(ybuf, M, N, what="gemv_mxfp4 random")


def test_gemv_mxfp4_rejects_bad_operands(dev):
    x = torch.zeros(9, 64, dtype=torch.bfloat16, device=dev)
    q = torch.zeros(4, 32, dtype=torch.uint8, device=dev)
    e = torch.full((4, 2), 127, dtype=torch.uint8, device=dev)
    y = torch.zeros(9, 4, device=dev)
    with pytest.raises(ValueError):
        ops.gemv_mxfp4(x, q, e, None, y)  # 9 rows
    with pytest.raises(ValueError):
        ops.gemv_mxfp4(x[:2, :48], q, e, None, y)  # K % 32
    with pytest.raises(ValueError):
        ops.gemv_mxfp4(x[:2], q, e[:, :1], None, y)  # fewer scale bytes than blocks
    with pytest.raises(TypeError):
        ops.gemv_mxfp4(x[:2], q.to(torch.int8), e, None, y)
    with pytest.raises(ValueError):  # rows of codes not 16-byte aligned: the launcher's -2
        ops.gemv_mxfp4(x[:2, :32], torch.zeros(4, 24, dtype=torch.uint8, device=dev)[:, :16],
                       e, None, y)


def test_gemv_mxfp4_native_program_replay_equals_eager(dev):
    """A recorded native Program of gemv_mxfp4 replays to the bits of the eager launch."""
    N, K, M = 10, 832, 5
    x, _, _, q, e, bias = gc.operands(N, K)
    xv = x[:M].to(torch.bfloat16).to(dev)
    qv, ev, bv = q.to(dev), e.to(dev), bias.float().to(dev)
    eager = torch.zeros(M, N, dtype=torch.float32, device=dev)
    ops.gemv_mxfp4(xv, qv, ev, bv, eager, "relu")
    y = torch.full((M, N), ao.SENTINEL, dtype=torch.float32, device=dev)
    prog = native().Program()
    native().record_begin(prog)
    try:
        prog.mark("fwd")
        ops.gemv_mxfp4(xv, qv, ev, bv, y, "relu")
    finally:
        native().record_end()
    y.fill_(ao.SENTINEL)
    torch.cuda.synchronize()
    prog.run(["fwd"], torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(y, eager) and bool((y != ao.SENTINEL).any())


# ---- quantiser / dequantiser kernels --------------------------------------------------------

def _window(rows, cols, dtype, fill, dev, pad_c):
    """(buffer, view): a [rows][cols] window at (PAD, pad_c) of a buffer filled with ``fill``,
    row stride cols + 3 * pad_c."""
    buf = torch.full((rows + 2 * ao.PAD, cols + 3 * pad_c), fill, dtype=dtype, device=dev)
    return buf, buf[ao.PAD:ao.PAD + rows, pad_c:pad_c + cols]


def _assert_outside_untouched(buf, view, fill, what):
    off = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    r0, c0 = off // buf.stride(0), off % buf.stride(0)
    outside = torch.ones(buf.shape, dtype=torch.bool)
    outside[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = False
    assert bool((buf.cpu()[outside] == fill).all()), f"{what}: wrote outside the view"


@pytest.mark.parametrize("name", mo.CASES)
def test_quant_dequant_kernels_equal_oracle(dev, name):
    """On padded views (ldx > cols, ldq > cols / 2, lde > cols / 32): GPU codes and scale bytes
    = quant_ref; GPU dequantisation of the oracle's codes = dequant_ref; nothing outside the
    views is written; the round trip through both kernels meets the format's bound."""
    x = mo.case(name)
    rows, cols = x.shape
    q_ref, e_ref, tie, y_ref = mo.reference(name)
    xbuf, xv = _window(rows, cols, torch.bfloat16, float("nan"), dev, 8)
    xv.copy_(x)
    qbuf, qv = _window(rows, cols // 2, torch.uint8, Q_FILL, dev, 16)
    ebuf, ev = _window(rows, cols // 32, torch.uint8, E_FILL, dev, 3)
    assert xv.stride(0) > cols and qv.stride(0) > cols // 2 and ev.stride(0) > cols // 32
    ops.quant_rows_mxfp4(xv, qv, ev)
    e, q = ev.cpu().numpy(), qv.cpu().numpy()
    bad_e = np.argwhere(e != e_ref)
    assert bad_e.size == 0, (f"{name}: {len(bad_e)} scale bytes differ, first at "
                             f"{bad_e[:4].tolist()}")
    diff = mo.unpack(q) != mo.unpack(q_ref)
    assert not diff.any(), (f"{name}: {int(diff.sum())} of {diff.size} codes differ, first at "
                            f"{np.argwhere(diff)[:4].tolist()}")
    _assert_outside_untouched(qbuf, qv, Q_FILL, f"{name} q")
    _assert_outside_untouched(ebuf, ev, E_FILL, f"{name} e")
    ybuf, yv = _window(rows, cols, torch.bfloat16, ao.SENTINEL, dev, 8)
    ops.dequant_rows_mxfp4(qv, ev, yv)
    assert torch.equal(mo.bits16(yv), mo.bits16(y_ref)), f"{name}: dequantised bf16"
    _assert_outside_untouched(ybuf, yv, ao.SENTINEL, f"{name} output")
    ratio = mo.assert_format_bound(x, yv, e_ref, name)
    print(f"\nmxfp4 {name}: {x.numel()} elements, {int(tie.sum())} exact ties, "
          f"round trip at {ratio:.3f} x the bound")


def test_dequant_kernel_zero_scale_gives_plus_zero(dev):
    """A block with E == 0 dequantises to +0 whatever its nibbles hold; its neighbour does
    not."""
    q = torch.full((3, 32), 0xF7, dtype=torch.uint8, device=dev)  # 6.0 and -6.0
    e = torch.tensor([[0, 127]] * 3, dtype=torch.uint8, device=dev)
    y = torch.full((3, 64), ao.SENTINEL, dtype=torch.bfloat16, device=dev)
    ops.dequant_rows_mxfp4(q, e, y)
    want = mo.dequant_ref(q.cpu().numpy(), e.cpu().numpy())
    assert torch.equal(mo.bits16(y), mo.bits16(want))
    assert bool((mo.bits16(y)[:, :32] == 0).all()) and float(y[0, 32]) == 6.0
    assert float(y[0, 33]) == -6.0
