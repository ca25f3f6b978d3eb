"""Operands and checks shared by the fp8-weight GEMM tests (tests/test_linear_fp8_gpu.py on the
GPU, tests/test_linear_fp8_cpu.py for the CPU reference): the exact-sum construction of
_gemv_fp8_cases.operands for any number of rows M.

x holds integers in [-2, 2], w multiples of 1/4 in [-2, 2] -- all 17 are e4m3 values, so
``_fp8_oracle.encode`` returns their codes with no tie and ``DEC[q] == w`` -- the scale of row n
cycles over {0.5, 1, 2, 0}, the bias holds multiples of 1/4 in [-4, 4], and scale and bias carry
5 NaN entries past N. With K <= 8208, |scale * S| + |bias| <= 2 * 4 * 8208 + 4 < 2^17 with 3
fraction bits: every product, every partial sum IN ANY ORDER and the scale multiply are exact in
fp32, so the kernel's pre-activation must EQUAL the fp64 value whatever its tile, its K split
and its MFMA slot order.

Sigmoid rows keep exactly NNZ_SIGMOID = 8 non-zero entries, the first and the last column among
them: |z| <= 2 * (8 * 4) + 4 = 68 < 80 (_act_oracle.py) by construction for every M and N; it is
asserted anyway.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import _act_oracle as ao
import _fp8_oracle as fo
import _gemv_fp8_cases as gc

NNZ_SIGMOID = 8
K_MAX = 8208


@functools.lru_cache(maxsize=None)
def operands(M: int, N: int, K: int):
    """(x, x_sigmoid, w, q, scale, bias): fp64 tensors, q uint8. Computed once per shape; never
    modified."""
    assert 16 <= K <= K_MAX and K % 16 == 0
    g = torch.Generator().manual_seed(104729 * M + 7919 * N + K)
    x = torch.randint(-2, 3, (M, K), generator=g).double()
    w = torch.randint(-8, 9, (N, K), generator=g).double() * 0.25
    bias = torch.randint(-16, 17, (N + 5,), generator=g).double() * 0.25
    scale = torch.tensor([gc.SCALES[n % 4] for n in range(N)] + [0.0] * 5, dtype=torch.float64)
    bias[N:] = scale[N:] = float("nan")
    nonzero = torch.tensor([-2.0, -1.0, 1.0, 2.0], dtype=torch.float64)
    xs = torch.zeros(M, K, dtype=torch.float64)
    for m in range(M):
        inner = 1 + torch.randperm(K - 2, generator=g)[:NNZ_SIGMOID - 2]
        cols = torch.cat([torch.tensor([0, K - 1]), inner])
        xs[m, cols] = nonzero[torch.randint(0, 4, (NNZ_SIGMOID,), generator=g)]
    assert bool(((xs != 0).sum(1) == NNZ_SIGMOID).all())
    assert bool((xs[:, 0] != 0).all()) and bool((xs[:, K - 1] != 0).all())
    code, tie = fo.encode(w.numpy().astype(np.float32))
    assert not tie.any() and np.array_equal(fo.DEC[code], w.numpy())  # w IS its e4m3 value
    return x, xs, w, torch.from_numpy(code), scale, bias


def check_exact(entry, M, N, K, dev, sigmoid_f32_max_ulp, **kw):
    """One (M, N, K): every activation, fp32 and bf16 output, bias and None, on NaN-padded views
    (ao.padded, gc.padded_codes). linear / relu bit-equal to fp64 (bf16: RN_bf16(fp64)); sigmoid
    within the given fp32 bound / 1 bf16 ulp; nothing written outside y[M][N]. Returns the worst
    fp32 sigmoid distance in ulps."""
    x, xs, w, q, scale, bias = operands(M, N, K)
    qv = gc.padded_codes(q, dev)
    sv = scale.float().to(dev)
    assert qv.stride(0) > K and qv.stride(0) % 16 == 0 and qv.data_ptr() % 16 == 0
    xin = {}
    for name, data in (("x", x), ("xs", xs)):
        _, xin[name] = ao.padded(M, K, torch.bfloat16, float("nan"), dev, data)
        assert xin[name].stride(0) > K
    worst = 0.0
    for b in (bias, None):
        bv = None if b is None else b.float().to(dev)
        for act in ao.ACTS:
            src = "xs" if act == "sigmoid" else "x"
            z = gc.oracle_z(xs if act == "sigmoid" else x, w, scale, b, M, N)
            if act == "sigmoid":
                assert float(z.abs().max()) <= 68.0
            ref = ao.act_fwd(z, act)
            what = f"linear_fp8 {M}x{N}x{K} {kw} {act} bias={b is not None}"
            ybuf, yv = ao.padded(M, N, torch.float32, ao.SENTINEL, dev)
            entry(xin[src], qv, sv, bv, yv, act, **kw)
            y = yv.detach().to(ao.CPU)
            if act == "sigmoid":
                assert bool(torch.isfinite(y).all()), what
                worst = max(worst, gc.f32_ulps(y, ref))
            else:
                assert torch.equal(y.double(), ref), f"{what} fp32: not the exact sum"
            ao.assert_padding_untouched(ybuf, M, N, what=f"{what} fp32")
            ybuf, yv = ao.padded(M, N, torch.bfloat16, ao.SENTINEL, dev)
            entry(xin[src], qv, sv, bv, yv, act, **kw)
            ao.assert_bf16_close(yv, ref, 1 if act == "sigmoid" else 0, f"{what} bf16")
            ao.assert_padding_untouched(ybuf, M, N, what=f"{what} bf16")
    assert worst <= sigmoid_f32_max_ulp, f"sigmoid fp32: {worst:.2f} ulp from fp64"
    return worst
