"""Operands and checks shared by the w8a8 tests (tests/test_linear_w8a8_gpu.py on the GPU,
tests/test_linear_w8a8_cpu.py for the CPU reference): ops.linear_w8a8 multiplies e4m3 codes by
e4m3 codes and applies one fp32 scale per data row and one per neuron,

    y[m][n] = act(fl32(sx[m] * fl32(sw[n] * sum_k dec(xq[m][k]) * dec(q[n][k]))) + b[n]).

Exact-sum operands: those of _linear_fp8_cases.operands -- x integers in [-2, 2], w multiples of
1/4 in [-2, 2], weight scales cycling over {0.5, 1, 2, 0}, bias multiples of 1/4 in [-4, 4] --
with x given as its e4m3 codes (all five values are e4m3 values: ``_fp8_oracle.encode`` has no
tie and ``DEC[code] == x``, asserted) and a row scale sx[m] cycling over {1, 0.5, 2, 0}, which is
a different phase from the weight scales, so every pair of scales meets. With K <= 8208,
|z| <= 2 * 2 * (4 * 8208) + 4 < 2^18 with 4 fraction bits (2 from the products, one from each
scale of 0.5): every product, every partial sum IN ANY ORDER and both scale multiplies are exact
in fp32, so the pre-activation must EQUAL the fp64 value whatever the tile, the lane map and the
MFMA's internal order. A zero row (sx = 0) and a zero neuron (sw = 0) must give act(b[n]).

Sigmoid needs |z| <= 80 (_act_oracle.py: beyond it the fp32 result leaves the normal range).
The 8-non-zero rows of _linear_fp8_cases.operands reach |z| = 2 * 2 * (8 * 4) + 4 = 132 under a
row scale of 2 (and do, at the 8192-neuron shapes), so the sigmoid rows here are their SIGNS: the
same 8 non-zero columns per row, the first and the last among them, entries +-1. Then |S| <= 16
and |z| <= 2 * 2 * 16 + 4 = 68 < 80 by construction for every M, N and K, as in
_linear_fp8_cases; it is asserted anyway.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import _act_oracle as ao
import _fp8_oracle as fo
import _gemv_fp8_cases as gc
import _linear_fp8_cases as lc

ROW_SCALES = (1.0, 0.5, 2.0, 0.0)


def codes_of(x: torch.Tensor) -> torch.Tensor:
    """e4m3 codes of a tensor of e4m3 values: no tie, and the codes decode to x exactly."""
    code, tie = fo.encode(x.numpy().astype(np.float32))
    assert not tie.any() and np.array_equal(fo.DEC[code], x.numpy())
    return torch.from_numpy(code)


@functools.lru_cache(maxsize=None)
def operands(M: int, N: int, K: int):
    """(x, x_sigmoid, xq, xq_sigmoid, sx, w, q, sw, bias): fp64 tensors and uint8 codes. sx, sw
    and bias carry 5 NaN entries past M / N. Computed once per shape; never modified."""
    x, xs, w, q, sw, bias = lc.operands(M, N, K)
    xs = torch.sign(xs)
    assert bool(((xs != 0).sum(1) == lc.NNZ_SIGMOID).all())
    sx = torch.tensor([ROW_SCALES[m % 4] for m in range(M)] + [float("nan")] * 5,
                      dtype=torch.float64)
    return x, xs, codes_of(x), codes_of(xs), sx, w, q, sw, bias


def oracle_z(x, sx, w, sw, bias, M, N):
    """fp64 pre-activation sx * (sw * (x . w^T)) + bias."""
    z = sx[:M, None] * (sw[:N] * (x[:M] @ w.t()))
    return z if bias is None else z + bias[:N]


def check_exact(entry, M, N, K, dev, sigmoid_f32_max_ulp, **kw):
    """One (M, N, K) through ``entry(xq, sx, q, sw, bias, y, act, **kw)``: every activation, fp32
    and bf16 output, bias and None, on NaN-padded views of xq, q (gc.padded_codes), sx, sw and
    bias. linear / relu bit-equal to fp64 (bf16: RN_bf16(fp64)); sigmoid within the given fp32
    bound / 1 bf16 ulp; nothing written outside y[M][N]. Returns the worst fp32 sigmoid distance
    in ulps."""
    x, xs, xq, xqs, sx, w, q, sw, bias = operands(M, N, K)
    qv = gc.padded_codes(q, dev)
    xin = {"x": gc.padded_codes(xq, dev), "xs": gc.padded_codes(xqs, dev)}
    for v in (qv, *xin.values()):
        assert v.stride(0) > K and v.stride(0) % 16 == 0 and v.data_ptr() % 16 == 0
    sxv, swv = sx.float().to(dev), sw.float().to(dev)
    worst = 0.0
    for b in (bias, None):
        bv = None if b is None else b.float().to(dev)
        for act in ao.ACTS:
            src = "xs" if act == "sigmoid" else "x"
            z = oracle_z(xs if act == "sigmoid" else x, sx, w, sw, b, M, N)
            if act == "sigmoid":
                assert float(z.abs().max()) <= 68.0
            ref = ao.act_fwd(z, act)
            what = f"linear_w8a8 {M}x{N}x{K} {kw} {act} bias={b is not None}"
            ybuf, yv = ao.padded(M, N, torch.float32, ao.SENTINEL, dev)
            entry(xin[src], sxv, qv, swv, bv, yv, act, **kw)
            y = yv.detach().to(ao.CPU)
            if act == "sigmoid":
                assert bool(torch.isfinite(y).all()), what
                worst = max(worst, gc.f32_ulps(y, ref))
            else:
                assert torch.equal(y.double(), ref), f"{what} fp32: not the exact sum"
            ao.assert_padding_untouched(ybuf, M, N, what=f"{what} fp32")
            ybuf, yv = ao.padded(M, N, torch.bfloat16, ao.SENTINEL, dev)
            entry(xin[src], sxv, qv, swv, bv, yv, act, **kw)
            ao.assert_bf16_close(yv, ref, 1 if act == "sigmoid" else 0, f"{what} bf16")
            ao.assert_padding_untouched(ybuf, M, N, what=f"{what} bf16")
    assert worst <= sigmoid_f32_max_ulp, f"sigmoid fp32: {worst:.2f} ulp from fp64"
    return worst


def chain_terms(K: int) -> int:
    """T of the summation bound: additions into one accumulator of linear_w8a8_kernel on its
    longest chain. Every tile gives a wave all of K for its outputs, one MFMA per 128-column
    k-step, and an MFMA adds its 128 products into the accumulator: 128 * ceil(K / 128)."""
    return 128 * -(-K // 128)


def summation_bound(K: int, mag: np.ndarray, bias: np.ndarray, u: float = 2.0 ** -24):
    """(T + 4) * u * (sx * sw * sum |dec dec| + |bias|): a product of two e4m3 values is exact in
    fp32 (4 x 4 significant bits), so the error is that of the T additions, the two scale
    multiplies, the bias add and one spare unit, each at most u of the running magnitude."""
    return (chain_terms(K) + 4) * u * (mag + np.abs(bias))


def element_bound(v: np.ndarray) -> np.ndarray:
    """Per element of a bf16 matrix quantised by rows: |s * dec(code) - v| <= fo.
    round_trip_bound without its bf16 term (the codes are multiplied undecoded: nothing is
    rounded to bf16), i.e. 2^-4 |v| + amax / 448 * 2^-10 (1 + 2^-6)."""
    t = torch.from_numpy(v)
    amax = t.abs().amax(1, keepdim=True)
    return (fo.round_trip_bound(t, amax) - 2.0 ** -8 * t.abs()).numpy()
