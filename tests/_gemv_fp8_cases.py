"""Operands and checks shared by the fp8-weight GEMV tests (tests/test_gemv_fp8_gpu.py on the
GPU, tests/test_fp8_weights_cpu.py for the CPU reference), by the method of _act_oracle.py.

Exact-sum operands: x holds integers in [-2, 2], w multiples of 1/4 in [-2, 2] -- all 17 are
e4m3 values, so ``_fp8_oracle.encode`` returns their codes with no tie and ``DEC[q] == w`` --
the scale of row n cycles over {0.5, 1, 2, 0} and the bias holds multiples of 1/4. Then
|scale * S| + |bias| <= 2 * 4 * 8208 + 4 < 2^17 with 3 fraction bits: every product, every
partial sum in any order and the scale multiply are exact in fp32, and the kernel's
pre-activation EQUALS the fp64 value. Row n with scale 0 must give act(bias[n]).

Sigmoid needs |z| <= 80 (_act_oracle.py), so its x rows keep NNZ_SIGMOID = 16 non-zero entries
spread over all of K, the first and last column among them: the sum S then has a standard
deviation of about sqrt(16 * 2 * 1.5) = 7, z = 2 S + bias stays far inside 80, and that is
asserted per case.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import _act_oracle as ao
import _fp8_oracle as fo

# N below, at and across the 4 waves of a block; K on, and one 16-byte step past, a 1024-column
# chunk (1040), an unaligned middle (832), and the sweeps of the k loop: 4096 columns (4 chunks)
# for 1-2 rows and 2048 (2 chunks) for 3-8 rows. 2064 is one step past the short sweep and in
# the middle of the long one; 4096 ends both; 4112 is one step past both; 8208 two long sweeps
# and a step.
NK = [(1, 16), (5, 1040), (10, 832), (3, 2064), (7, 4096), (6, 4112), (9, 8208)]
NNZ_SIGMOID = 16
SCALES = (0.5, 1.0, 2.0, 0.0)
QPAD = 16  # bytes in front of a padded row of codes (rows stay 16-byte aligned)
NAN_CODE = 0x7F


@functools.lru_cache(maxsize=None)
def operands(N: int, K: int):
    """(x, x_sigmoid, w, q, scale, bias): fp64 tensors, q uint8. scale and bias carry 5 NaN
    entries past N that must never be read. Computed once per shape; never modified."""
    g = torch.Generator().manual_seed(7919 * N + K)
    x = torch.randint(-2, 3, (8, K), generator=g).double()
    w = torch.randint(-8, 9, (N, K), generator=g).double() * 0.25
    bias = torch.randint(-16, 17, (N + 5,), generator=g).double() * 0.25
    scale = torch.tensor([SCALES[n % 4] for n in range(N)] + [0.0] * 5, dtype=torch.float64)
    bias[N:] = scale[N:] = float("nan")
    keep = torch.zeros(8, K, dtype=torch.bool)
    for m in range(8):
        keep[m, torch.randperm(K, generator=g)[:NNZ_SIGMOID]] = True
    keep[:, 0] = keep[:, K - 1] = True
    xs = torch.where(keep, x, torch.zeros_like(x))
    xs[:, 0], xs[:, K - 1] = 2.0, -1.0
    code, tie = fo.encode(w.numpy().astype(np.float32))
    assert not tie.any() and np.array_equal(fo.DEC[code], w.numpy())  # w IS its e4m3 value
    return x, xs, w, torch.from_numpy(code), scale, bias


def oracle_z(x, w, scale, bias, M, N):
    """fp64 pre-activation scale * (x . w^T) + bias of rows [0, M)."""
    z = scale[:N] * (x[:M] @ w.t())
    return z if bias is None else z + bias[:N]


def padded_codes(q: torch.Tensor, dev):
    """The codes as a view inside a wider, taller buffer of NaN codes (ldq > K, 16-byte
    aligned rows)."""
    N, K = q.shape
    buf = torch.full((N + 2 * ao.PAD, K + 3 * QPAD), NAN_CODE, dtype=torch.uint8)
    buf[ao.PAD:ao.PAD + N, QPAD:QPAD + K] = q
    buf = buf.to(dev)
    return buf[ao.PAD:ao.PAD + N, QPAD:QPAD + K]


def f32_ulps(got, ref):
    """|got - ref| in units of the fp32 spacing at ref (fp64 arithmetic)."""
    ulp = torch.pow(torch.tensor(2.0, dtype=torch.float64),
                    torch.floor(torch.log2(ref.abs())) - 23)
    return float(((got.double() - ref).abs() / ulp).max())


def check_exact_shape(entry, N, K, dev, sigmoid_f32_max_ulp):
    """M = 1..8, every activation, fp32 and bf16 output, bias and None, on padded views.
    Returns the worst fp32 sigmoid distance in ulps (asserted against the given bound)."""
    x, xs, w, q, scale, bias = operands(N, K)
    qv = padded_codes(q, dev)
    sv = scale.float().to(dev)
    assert qv.stride(0) > K and qv.stride(0) % 16 == 0 and qv.data_ptr() % 16 == 0
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
                z = oracle_z(xs if act == "sigmoid" else x, w, scale, b, M, N)
                if act == "sigmoid":
                    assert float(z.abs().max()) <= 80.0
                ref = ao.act_fwd(z, act)
                what = f"gemv_fp8 {M}x{N}x{K} {act} bias={b is not None}"
                ybuf, yv = ao.padded(M, N, torch.float32, ao.SENTINEL, dev)
                entry(xin[src], qv, sv, bv, yv, act)
                y = yv.detach().to(ao.CPU)
                if act == "sigmoid":
                    assert bool(torch.isfinite(y).all()), what
                    worst = max(worst, f32_ulps(y, ref))
                else:
                    assert torch.equal(y.double(), ref), f"{what} fp32: not the exact sum"
                ao.assert_padding_untouched(ybuf, M, N, what=f"{what} fp32")
                ybuf, yv = ao.padded(M, N, torch.bfloat16, ao.SENTINEL, dev)
                entry(xin[src], qv, sv, bv, yv, act)
                ao.assert_bf16_close(yv, ref, 1 if act == "sigmoid" else 0, f"{what} bf16")
                ao.assert_padding_untouched(ybuf, M, N, what=f"{what} bf16")
    assert worst <= sigmoid_f32_max_ulp, f"sigmoid fp32: {worst:.2f} ulp from fp64"
    return worst


# ---- the format's accuracy ------------------------------------------------------------------

def format_bound(w64: np.ndarray) -> np.ndarray:
    """Per element: |s * dec(q) - w| <= 2^-4 (1 + 2^-10) |w| + amax / 448 * 2^-10 (1 + 2^-6):
    half an e4m3 step at the bottom of a binade (2^-4 relative; the two fp32 quotients and the
    product that place w on the grid cost the 2^-10 spare), or half a subnormal step of the
    row's grid (amax / 448 * 2^-10, its fp32 roundings in the 2^-6 spare)."""
    amax = np.abs(w64).max(axis=1, keepdims=True)
    return 2.0 ** -4 * (1 + 2.0 ** -10) * np.abs(w64) + amax / 448.0 * 2.0 ** -10 * (1 + 2.0 ** -6)


def lane_terms(K: int) -> int:
    """T of the summation bound: the products one lane of gemv_fp8_kernel accumulates, 16 per
    1024-column chunk over ceil(K / 1024) chunks."""
    return 16 * math.ceil(K / 1024)


def summation_bound(K: int, mag: np.ndarray, bias: np.ndarray) -> np.ndarray:
    """(T + 6 + 3) * 2^-24 * (s * sum |x dec| + |bias|): dec * x is exact in fp32, so the error
    is that of T additions in a lane, 6 shuffle levels, the scale multiply, the bias add and
    one spare unit, each at most 2^-24 of the running magnitude."""
    return (lane_terms(K) + 6 + 3) * 2.0 ** -24 * (mag + np.abs(bias))


def one_layer_case(seed=24):
    """A 64 -> 24 linear layer with random bf16 weights, a bias, and one bf16 input row."""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(24, 64, generator=g) / 8.0).to(torch.bfloat16)
    b = torch.randn(24, generator=g).float()
    x = torch.randn(1, 64, generator=g).to(torch.bfloat16)
    return w, b, x


def check_one_layer(y: np.ndarray, w, b, x):
    """y [1][24]: the fp8 layer's answer; within the format's bound summed against |x| plus the
    summation bound of the fp64 product with the ORIGINAL bf16 weights. Returns the ratio."""
    w64, x64, b64 = w.double().numpy(), x.double().numpy(), b.double().numpy()
    q, s, _ = fo.quant_ref(w)
    deq = s.astype(np.float64)[:, None] * fo.DEC[q]
    fmt = format_bound(w64)
    assert (np.abs(deq - w64) <= fmt).all()
    ref = x64 @ w64.T + b64
    bound = np.abs(x64) @ fmt.T + summation_bound(64, np.abs(x64) @ np.abs(deq).T, b64)
    ratio = float((np.abs(y - ref) / bound).max())
    assert ratio <= 1.0, f"fp8 layer at {ratio:.3f} x the format + summation bound"
    return ratio
