"""Operands and checks shared by the MXFP4-weight GEMV tests (tests/test_gemv_mxfp4_gpu.py and
tests/test_mxfp4_engine_gpu.py on the GPU, tests/test_mxfp4_weights_cpu.py for the CPU
reference), by the method of _gemv_fp8_cases.py.

Exact-sum operands: x holds integers in [-2, 2]; the codes are drawn directly, uniform over the
16 codes (not through the quantiser, so every code meets every scale); the scale byte of block b
of row n cycles over E in {126, 127, 128, 0} with n + b; the bias holds multiples of 1/4. A
weight is then at most 6 * 2 = 12 with one fraction bit at most 2 (0.5 * 2^-1), so |S| <= 2 * 12
* 8224 < 2^18 with 2 fraction bits: every product and every partial sum in any order is exact in
fp32, and the kernel's pre-activation EQUALS the fp64 value. A block with E = 0 contributes
nothing whatever its codes are.

Sigmoid needs |z| <= 80 (_act_oracle.py), so its x rows keep NNZ_SIGMOID = 8 non-zero entries
spread over all of K, the first and last column among them; |z| <= 80 is asserted per case.

How each K falls against gemv_mxfp4_kernel. A lane's unit is half a block (16 columns, a chunk
1024 columns) except for 1-2 rows at K >= 2048, where it is a whole block (a chunk 2048
columns); a sweep is 4096 columns for 1-2 rows and 2048 for 3-8 rows in either form. 32 is one
block (two lanes); 832 an unaligned middle of a chunk; 1056 one block past a 1024-column chunk;
2080 one block past a chunk of either size, past the short sweep and in the middle of the long
one; 4096 ends both sweeps; 4128 is one block past both; 8224 two long sweeps and a block. Added
to the issue's list for the threshold between the two units: 2016, the last K on the half-block
kernels at 1-2 rows, and 2048, the first on the whole-block ones (exactly one full chunk).
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import _act_oracle as ao
import _mxfp4_oracle as mo
from _gemv_fp8_cases import f32_ulps

NK = [(1, 32), (5, 1056), (10, 832), (3, 2080), (7, 4096), (6, 4128), (9, 8224), (2, 2016),
      (4, 2048)]
NNZ_SIGMOID = 8
SCALE_BYTES = (126, 127, 128, 0)
QPAD = 16  # bytes in front of a padded row of codes (rows stay 16-byte aligned)
EPAD = 3  # bytes in front of a padded row of scale bytes (no alignment is required)
Q_JUNK = 0x77  # two codes of 6.0
E_JUNK = 0xFE  # 2^127: the largest scale
E_NAN = 0xFF  # e8m0's NaN: rows of scale bytes past N


@functools.lru_cache(maxsize=None)
def operands(N: int, K: int):
    """(x, x_sigmoid, w, q, e, bias): fp64 tensors, q / e uint8 (packed codes, scale bytes), w
    the fp64 weights they stand for. bias carries 5 NaN entries past N that must never be read.
    Computed once per shape; never modified."""
    g = torch.Generator().manual_seed(7919 * N + K)
    x = torch.randint(-2, 3, (8, K), generator=g).double()
    code = torch.randint(0, 16, (N, K), generator=g).to(torch.uint8).numpy()
    nb = K // mo.BLOCK
    e = np.array([[SCALE_BYTES[(n + b) % 4] for b in range(nb)] for n in range(N)], dtype=np.uint8)
    q = mo.pack(code)
    w = torch.from_numpy(mo.values(q, e))
    assert float(w.abs().max()) <= 12.0
    bias = torch.randint(-16, 17, (N + 5,), generator=g).double() * 0.25
    bias[N:] = float("nan")
    keep = torch.zeros(8, K, dtype=torch.bool)
    for m in range(8):
        keep[m, torch.randperm(K, generator=g)[:NNZ_SIGMOID]] = True
    keep[:, 0] = keep[:, K - 1] = True
    xs = torch.where(keep, x, torch.zeros_like(x))
    xs[:, 0], xs[:, K - 1] = 2.0, -1.0
    return x, xs, w, torch.from_numpy(q), torch.from_numpy(e), bias


def oracle_z(x, w, bias, M, N):
    """fp64 pre-activation x . w^T + bias of rows [0, M)."""
    z = x[:M] @ w.t()
    return z if bias is None else z + bias[:N]


def _padded_bytes(t: torch.Tensor, dev, pad_c: int, fill: int, fill_rows: int):
    """A uint8 matrix as a view inside a wider, taller buffer: ``fill`` to the left and right
    of every row, ``fill_rows`` in the rows above and below."""
    n, c = t.shape
    buf = torch.full((n + 2 * ao.PAD, c + 3 * pad_c), fill_rows, dtype=torch.uint8)
    buf[ao.PAD:ao.PAD + n] = fill
    buf[ao.PAD:ao.PAD + n, pad_c:pad_c + c] = t
    buf = buf.to(dev)
    return buf, buf[ao.PAD:ao.PAD + n, pad_c:pad_c + c]


def padded_codes(q: torch.Tensor, dev):
    """The packed codes as a view inside a buffer of 6.0 codes (ldq > K / 2, 16-byte aligned
    rows)."""
    return _padded_bytes(q, dev, QPAD, Q_JUNK, Q_JUNK)[1]


def padded_scales(e: torch.Tensor, dev):
    """The scale bytes as a view inside a buffer whose bytes beside them are 2^127 and whose
    rows past N are e8m0 NaN (lde > K / 32)."""
    return _padded_bytes(e, dev, EPAD, E_JUNK, E_NAN)[1]


def check_exact_shape(entry, N, K, dev, sigmoid_f32_max_ulp):
    """M = 1..8, every activation, fp32 and bf16 output, bias and None, on padded views.
    Returns the worst fp32 sigmoid distance in ulps (asserted against the given bound)."""
    x, xs, w, q, e, bias = operands(N, K)
    qv, ev = padded_codes(q, dev), padded_scales(e, dev)
    assert qv.stride(0) > K // 2 and qv.stride(0) % 16 == 0 and qv.data_ptr() % 16 == 0
    assert ev.stride(0) > K // 32
    worst = 0.0
    for M in range(1, 9):
        xin = {}
        for name, data in (("x", x), ("xs", xs)):
            _, xin[name] = ao.padded(M, K, torch.bfloat16, float("nan"), dev, data[:M])
            assert xin[name].stride(0) > K
        for b in (bias, None):
            bv = None if b is None else b.float().to(dev)
            for act in ao.ACTS:
                src = "xs" if act == "sigmoid" else "x"
                z = oracle_z(xs if act == "sigmoid" else x, w, b, M, N)
                if act == "sigmoid":
                    assert float(z.abs().max()) <= 80.0
                ref = ao.act_fwd(z, act)
                what = f"gemv_mxfp4 {M}x{N}x{K} {act} bias={b is not None}"
                ybuf, yv = ao.padded(M, N, torch.float32, ao.SENTINEL, dev)
                entry(xin[src], qv, ev, bv, yv, act)
                y = yv.detach().to(ao.CPU)
                if act == "sigmoid":
                    assert bool(torch.isfinite(y).all()), what
                    worst = max(worst, f32_ulps(y, ref))
                else:
                    assert torch.equal(y.double(), ref), f"{what} fp32: not the exact sum"
                ao.assert_padding_untouched(ybuf, M, N, what=f"{what} fp32")
                ybuf, yv = ao.padded(M, N, torch.bfloat16, ao.SENTINEL, dev)
                entry(xin[src], qv, ev, bv, yv, act)
                ao.assert_bf16_close(yv, ref, 1 if act == "sigmoid" else 0, f"{what} bf16")
                ao.assert_padding_untouched(ybuf, M, N, what=f"{what} bf16")
    assert worst <= sigmoid_f32_max_ulp, f"sigmoid fp32: {worst:.2f} ulp from fp64"
    return worst


def check_zero_blocks_add_nothing(entry, dev):
    """Rows whose every scale byte is 0 over codes of 6.0 and -6.0 give act(bias) exactly; a row
    with one live block gives that block's sum alone."""
    N, K = 4, 1056
    code = np.full((N, K), 7, dtype=np.uint8)
    code[:, 1::2] = 15
    e = np.zeros((N, K // 32), dtype=np.uint8)
    e[2, 5], e[3, 32] = 127, 126  # row 2: block 5; row 3: the block past the first chunk (1024)
    x = torch.arange(K, dtype=torch.float64).remainder(5) - 2.0
    w = mo.values(mo.pack(code), e)
    want = torch.from_numpy(w @ x.numpy())[None, :] + 0.25
    assert want[0, 0] == 0.25 and want[0, 1] == 0.25 and want[0, 2] != 0.25 and want[0, 3] != 0.25
    y = torch.full((1, N), ao.SENTINEL, dtype=torch.float32, device=dev)
    entry(x[None, :].to(torch.bfloat16).to(dev), torch.from_numpy(mo.pack(code)).to(dev),
          torch.from_numpy(e).to(dev), torch.full((N,), 0.25, device=dev), y, "linear")
    assert torch.equal(y.cpu().double(), want)


# ---- random operands: the format's accuracy and the summation bound --------------------------

def lane_terms(K: int, M: int) -> int:
    """T of the summation bound: the products one lane of gemv_mxfp4_kernel accumulates at M
    rows: 32 (a whole block) per 2048-column chunk for 1-2 rows at K >= 2048, otherwise 16
    (half a block) per 1024-column chunk."""
    if M <= 2 and K >= 2048:
        return 32 * math.ceil(K / 2048)
    return 16 * math.ceil(K / 1024)


def summation_bound(K: int, M: int, mag: np.ndarray, bias: np.ndarray) -> np.ndarray:
    """(T + 6 + 2) * 2^-24 * (sum |x deq| + |bias|): dec * scale * x is exact in fp32, so the
    error is that of T additions in a lane, 6 shuffle levels, the bias add and one spare unit,
    each at most 2^-24 of the running magnitude (no scale multiply after the reduction)."""
    return (lane_terms(K, M) + 6 + 2) * 2.0 ** -24 * (mag + np.abs(bias))


@functools.lru_cache(maxsize=None)
def layer_case(N: int, K: int, M: int):
    """An K -> N linear layer with random bf16 weights (randn / sqrt(K)), a bias, and M bf16
    input rows: every product |x| * |deq| is zero or far inside fp32's normal range."""
    g = torch.Generator().manual_seed(100 * N + K)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(N, generator=g).float()
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    return w, b, x


# (N, K, M): the smallest padded layer; a long odd one on the half-block and on the whole-block unit
LAYERS = [(24, 64, 1), (9, 2080, 8), (9, 2080, 2)]


def check_layer(y: np.ndarray, w, b, x) -> float:
    """y [M][N]: the MXFP4 layer's linear answer; within the format's per-weight bound summed
    against |x| plus the summation bound, of the fp64 product with the ORIGINAL bf16 weights.
    Returns the worst ratio."""
    w64, x64, b64 = w.double().numpy(), x.double().numpy(), b.double().numpy()
    q, e, _ = mo.quant_ref(w)
    deq = mo.values(q, e)
    fmt = mo.format_bound(w64, e)
    assert (np.abs(deq - w64) <= fmt).all()
    prod = np.abs(x64)[:, None, :] * np.abs(deq)[None, :, :]
    assert prod[prod > 0].min() > 2.0 ** -126 and prod.max() < 2.0 ** 127
    ref = x64 @ w64.T + b64
    bound = np.abs(x64) @ fmt.T + summation_bound(w.shape[1], x.shape[0],
                                                  np.abs(x64) @ np.abs(deq).T, b64)
    ratio = float((np.abs(y - ref) / bound).max())
    assert ratio <= 1.0, f"mxfp4 layer at {ratio:.3f} x the format + summation bound"
    return ratio
