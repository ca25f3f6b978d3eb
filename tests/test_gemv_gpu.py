"""The serving GEMV (csrc/kernels/gemv.hip, ops.gemv and ops.linear_fwd for <= 8 rows) against
the exact fp64 oracle, by the method of tests/_act_oracle.py: x and w hold integers in [-2, 2]
and the bias multiples of 1/4, so every product and every partial sum is exact in fp32 in any
order (|sum| <= 4 * 8200 + 4 < 2^24, with two fraction bits to spare) and the kernel's
pre-activation EQUALS the fp64 value. Linear and ReLU outputs are then bit-equal to the
reference (fp32) or to its single rounding RN_bf16 (bf16): a dropped term, a wrong bias entry or
a wrong rounding mode cannot hide. Operands are views inside NaN-filled wider buffers (ldx, ldw
> K), the result a view inside a sentinel buffer (ldy > N) that must stay untouched outside
[M][N].

Sigmoid: as in _act_oracle the method needs |z| <= 80 (beyond it e^-z leaves fp32's normal
range), so the sigmoid operands keep 64 non-zero x entries per row, spread over all of K, which
bounds |z| by reasoning about the sum's spread (std 16) and is asserted per case.
"""
import math

import pytest
import torch

import _act_oracle as ao
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.ops import kernels as K_

pytestmark = pytest.mark.gpu

# N below, at and across the 4 waves of a block; K on and one 16-byte step past each
# 512-column chunk and the 4 x 512 unroll
NK = [(1, 8), (5, 520), (10, 832), (7, 2048), (6, 2056), (3, 4104), (9, 8200)]
NNZ_SIGMOID = 64

# Largest distance of the fp32 sigmoid output from the fp64 sigmoid, in fp32 ulps of the
# reference value, measured over all shapes of this file on MI355X: 45.09 (at N=10, K=832; 3.4
# to 28.1 at the other shapes); the bound is the next power of two. It comes from __expf (the
# argument z * log2(e) rounded to fp32 costs up to |z| * 2^-24 relative, then v_exp_f32) plus
# one add and one division.
SIGMOID_F32_MAX_ULP = 64.0


def _operands(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (8, K), generator=g).double()
    w = torch.randint(-2, 3, (N, K), generator=g).double()
    bias = torch.randint(-16, 17, (N + 5,), generator=g).double() * 0.25
    bias[N:] = float("nan")  # never read
    # sigmoid: NNZ_SIGMOID entries of each x row survive, the first and last column among them
    keep = torch.zeros(8, K, dtype=torch.bool)
    for m in range(8):
        keep[m, torch.randperm(K, generator=g)[:NNZ_SIGMOID]] = True
    keep[:, 0] = keep[:, K - 1] = True
    xs = torch.where(keep, x, torch.zeros_like(x))
    xs[:, 0], xs[:, K - 1] = 2.0, -1.0
    return x, xs, w, bias


def _f32_ulps(got, ref):
    """|got - ref| in units of the fp32 spacing at ref (fp64 arithmetic)."""
    ulp = torch.pow(torch.tensor(2.0, dtype=torch.float64),
                    torch.floor(torch.log2(ref.abs())) - 23)
    return float(((got.double() - ref).abs() / ulp).max())


def _run(entry, x, w, bias, M, N, K, act, dtype, dev):
    _, xv = ao.padded(M, K, torch.bfloat16, float("nan"), dev, x[:M])
    _, wv = ao.padded(N, K, torch.bfloat16, float("nan"), dev, w)
    ybuf, yv = ao.padded(M, N, dtype, ao.SENTINEL, dev)
    assert xv.stride(0) > K and wv.stride(0) > K and yv.stride(0) > N
    entry(xv, wv, None if bias is None else bias.float().to(dev), yv, act)
    return ybuf, yv.detach().to(ao.CPU)


@pytest.mark.parametrize("N,K", NK)
def test_gemv_equals_fp64_oracle(dev, N, K):
    """M = 1..8, every activation, fp32 and bf16 output, with a bias vector longer than N and
    with bias=None, through ops.gemv and ops.linear_fwd. fp32: linear / relu bit-equal, sigmoid
    within SIGMOID_F32_MAX_ULP fp32 ulps of fp64 (measured worst: 45.09). bf16: linear /
    relu bit-equal to RN_bf16(fp64), sigmoid within 1 bf16 ulp."""
    x, xs, w, bias = _operands(N, K, 7919 * N + K)
    worst, share, elems = 0.0, 0.0, 0
    for M in range(1, 9):
        for b in (bias, None):
            add = 0.0 if b is None else b[:N]
            z = {a: (xs if a == "sigmoid" else x)[:M] @ w.t() + add for a in ao.ACTS}
            assert float(z["sigmoid"].abs().max()) <= 80.0
            for entry in (ops.gemv, ops.linear_fwd):
                for act in ao.ACTS:
                    ref = ao.act_fwd(z[act], act)
                    xin = xs if act == "sigmoid" else x
                    what = f"{entry.__name__} {M}x{N}x{K} {act} bias={b is not None}"
                    ybuf, y = _run(entry, xin, w, b, M, N, K, act, torch.float32, dev)
                    if act == "sigmoid":
                        assert bool(torch.isfinite(y).all()), what
                        worst = max(worst, _f32_ulps(y, ref))
                    else:
                        assert torch.equal(y.double(), ref), f"{what} fp32: not the exact sum"
                    ao.assert_padding_untouched(ybuf, M, N, what=f"{what} fp32")
                    ybuf, y = _run(entry, xin, w, b, M, N, K, act, torch.bfloat16, dev)
                    d = ao.assert_bf16_close(y, ref, 1 if act == "sigmoid" else 0, f"{what} bf16")
                    ao.assert_padding_untouched(ybuf, M, N, what=f"{what} bf16")
                    if act == "sigmoid":
                        share, elems = share + d * y.numel(), elems + y.numel()
    print(f"\ngemv N={N} K={K}: sigmoid fp32 worst {worst:.2f} ulp (bound "
          f"{SIGMOID_F32_MAX_ULP:g}); bf16 sigmoid {share / elems:.2%} of {elems} one ulp off")
    assert worst <= SIGMOID_F32_MAX_ULP, f"sigmoid fp32: {worst:.2f} ulp from fp64"


def test_linear_fwd_dispatches_to_gemv(dev, monkeypatch):
    calls = []
    real = K_.gemv
    monkeypatch.setattr(K_, "gemv", lambda *a, **k: (calls.append(a[0].shape[0]), real(*a, **k))[1])
    w = torch.ones(64, 64, dtype=torch.bfloat16, device=dev)
    for M in (1, 8, 64):
        x = torch.ones(M, 64, dtype=torch.bfloat16, device=dev)
        y = torch.zeros(M, 64, dtype=torch.bfloat16, device=dev)
        ops.linear_fwd(x, w, None, y, act="linear")
        assert bool((y == 64).all())
    assert calls == [1, 8]  # 64 rows run the MFMA GEMM


def test_gemv_random_operands_within_derived_bound(dev):
    """Random (non-integer) bf16 operands at 8 x 300 x 4104 against the fp64 product: products
    of bf16 pairs are exact in fp32, so the error is that of the additions only -- per lane
    8 * ceil(K / 512) terms, then 6 shuffle levels, the bias and the conversion, each at most
    2^-24 of the running magnitude <= sum |x_k w_k| (+ |bias|, which the 8 spare units cover):
    |y - ref| <= (8 * ceil(K / 512) + 8) * 2^-24 * sum_k |x_k w_k| per output."""
    M, N, K = 8, 300, 4104
    g = torch.Generator().manual_seed(4104)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    bias = torch.randn(N, generator=g)
    ref = x.double() @ w.double().t() + bias.double()
    mag = x.double().abs() @ w.double().abs().t()
    assert float((bias.double().abs() / mag).max()) <= 1.0
    bound = (8 * math.ceil(K / 512) + 8) * 2.0 ** -24 * mag
    ybuf, y = _run(ops.gemv, x, w, bias, M, N, K, "linear", torch.float32, dev)
    ratio = float(((y.double() - ref).abs() / bound).max())
    print(f"\ngemv random 8x300x4104: error at {ratio:.3f} x the derived bound")
    assert ratio <= 1.0
    ao.assert_padding_untouched(ybuf, M, N, what="gemv random")
