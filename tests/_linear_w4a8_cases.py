"""Operands and checks shared by the w4a8 tests (tests/test_linear_w4a8_gpu.py on the GPU,
tests/test_linear_w4a8_cpu.py for the CPU reference): ops.linear_w4a8 multiplies e4m3 activation
codes by MXFP4 weights (e2m1 codes, one e8m0 scale byte per 32 columns) and applies one fp32
scale per data row,

    y[m][n] = act(fl32(sx[m] * sum_k dec(xq[m][k]) * dec(q[n][k]) * 2^(e[n][k / 32] - 127)) + b[n]),

a block whose scale byte is 0 contributing nothing.

Exact-sum operands, by the method of _linear_w8a8_cases.py and _gemv_mxfp4_cases.py: x holds
integers in [-2, 2], given as their e4m3 codes (``_fp8_oracle.encode`` has no tie and ``DEC[code]
== x``, asserted); the row scale sx[m] cycles over {1, 0.5, 2, 0}; the weight codes are drawn
uniformly over all 16 codes, not through the quantiser; the scale byte of block b of neuron n
cycles over {126, 127, 128, 0} with n + b, so every lane position meets every scale and the E =
0 blocks carry non-zero junk codes; the bias holds multiples of 1/4 in [-4, 4]. A weight is at
most 6 * 2 = 12 with two fraction bits (0.5 * 2^-1). With K <= 8224, |z| <= 2 * 2 * 12 * 8224 + 4
< 2^19 with three fraction bits (one more from a row scale of 0.5): every product, every partial
sum IN ANY ORDER and the row-scale multiply are exact in fp32, so the pre-activation must EQUAL
the fp64 value whatever the tile, the lane map and the MFMA's internal order; the magnitude is
asserted per case. A zero row (sx = 0) must give act(b[n]).

Sigmoid needs |z| <= 80 (_act_oracle.py). Its rows hold 8 non-zero entries +-1, the first and
the last column among them; a +-1 entry against a weight of up to 12 under a row scale of 2
would reach 2 * 8 * 12 + 4 = 196, and smaller entries cannot fix that (the e4m3 codes must stay
integers for the exactness argument), so the sigmoid cases draw their weight codes from
magnitudes up to 2 only (code & 7 <= 4): with block scales up to 2 a weight is at most 4 and
|z| <= 2 * 8 * 4 + 4 = 68, asserted per case.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import _act_oracle as ao
import _fp8_oracle as fo
import _gemv_fp8_cases as gc
import _gemv_mxfp4_cases as mg
import _mxfp4_oracle as mo

ROW_SCALES = (1.0, 0.5, 2.0, 0.0)
NNZ_SIGMOID = 8
K_MAX = 8224
ONE = 0x38  # the e4m3 code of 1.0


def codes_of(x: torch.Tensor) -> torch.Tensor:
    """e4m3 codes of a tensor of e4m3 values: no tie, and the codes decode to x exactly."""
    code, tie = fo.encode(x.numpy().astype(np.float32))
    assert not tie.any() and np.array_equal(fo.DEC[code], x.numpy())
    return torch.from_numpy(code)


@functools.lru_cache(maxsize=None)
def operands(M: int, N: int, K: int):
    """dict of fp64 tensors and uint8 codes: x / xs (sigmoid rows) with their codes xq / xqs, sx,
    w / q (all 16 codes) and ws / qs (sigmoid: magnitudes up to 2), the scale bytes e shared by
    both, bias. sx and bias carry 5 NaN entries past M / N. Computed once per shape; never
    modified."""
    assert K % mo.BLOCK == 0 and K <= K_MAX
    g = torch.Generator().manual_seed(104729 * M + 7919 * N + K)
    x = torch.randint(-2, 3, (M, K), generator=g).double()
    keep = torch.zeros(M, K, dtype=torch.bool)
    for m in range(M):
        keep[m, torch.randperm(K, generator=g)[:NNZ_SIGMOID - 2]] = True
    keep[:, 0] = keep[:, K - 1] = True
    sign = torch.randint(0, 2, (M, K), generator=g).double() * 2.0 - 1.0
    xs = torch.where(keep, sign, torch.zeros_like(sign))
    assert bool(((xs != 0).sum(1) <= NNZ_SIGMOID).all()) and bool((xs[:, 0] != 0).all()) \
        and bool((xs[:, K - 1] != 0).all())
    code = torch.randint(0, 16, (N, K), generator=g).to(torch.uint8).numpy()
    mag = torch.randint(0, 5, (N, K), generator=g).to(torch.uint8).numpy()
    sgn = torch.randint(0, 2, (N, K), generator=g).to(torch.uint8).numpy()
    code_s = mag | (sgn << 3)
    nb = K // mo.BLOCK
    e = np.array([[mg.SCALE_BYTES[(n + b) % 4] for b in range(nb)] for n in range(N)],
                 dtype=np.uint8)
    q, qs = mo.pack(code), mo.pack(code_s)
    w, ws = torch.from_numpy(mo.values(q, e)), torch.from_numpy(mo.values(qs, e))
    assert float(w.abs().max()) <= 12.0 and float(ws.abs().max()) <= 4.0
    sx = torch.tensor([ROW_SCALES[m % 4] for m in range(M)] + [float("nan")] * 5,
                      dtype=torch.float64)
    bias = torch.randint(-16, 17, (N + 5,), generator=g).double() * 0.25
    bias[N:] = float("nan")
    return {"x": x, "xs": xs, "xq": codes_of(x), "xqs": codes_of(xs), "sx": sx, "w": w, "ws": ws,
            "q": torch.from_numpy(q), "qs": torch.from_numpy(qs), "e": torch.from_numpy(e),
            "bias": bias}


def oracle_z(x, sx, w, bias, M, N):
    """fp64 pre-activation sx * (x . w^T) + bias."""
    z = sx[:M, None] * (x[:M] @ w.t())
    return z if bias is None else z + bias[:N]


def check_exact(entry, M, N, K, dev, sigmoid_f32_max_ulp, **kw):
    """One (M, N, K) through ``entry(xq, sx, q, e, bias, y, act, **kw)``: every activation, fp32
    and bf16 output, bias and None. xq sits in a buffer of NaN codes, q in one of 6.0 codes, e in
    one of 0xFE beside it and 0xFF in the rows past N with an odd byte offset in front of each
    row, sx and bias in front of NaN entries, y in a sentinel-filled buffer. linear / relu
    bit-equal to fp64 (bf16: RN_bf16(fp64)); sigmoid within the given fp32 bound / 1 bf16 ulp;
    nothing written outside y[M][N]. Returns the worst fp32 sigmoid distance in ulps."""
    o = operands(M, N, K)
    ev = mg.padded_scales(o["e"], dev)
    assert ev.stride(0) > K // 32 and ev.storage_offset() % 2 == 1
    qin = {"x": mg.padded_codes(o["q"], dev), "xs": mg.padded_codes(o["qs"], dev)}
    xin = {"x": gc.padded_codes(o["xq"], dev), "xs": gc.padded_codes(o["xqs"], dev)}
    for v in (*qin.values(), *xin.values()):
        assert v.stride(0) % 16 == 0 and v.data_ptr() % 16 == 0
    assert xin["x"].stride(0) > K and qin["x"].stride(0) > K // 2
    sxv = o["sx"].float().to(dev)
    worst = 0.0
    for b in (o["bias"], None):
        bv = None if b is None else b.float().to(dev)
        for act in ao.ACTS:
            src = "xs" if act == "sigmoid" else "x"
            z = oracle_z(o[src], o["sx"], o["ws" if act == "sigmoid" else "w"], b, M, N)
            assert float(z.abs().max()) <= (68.0 if act == "sigmoid" else 2.0 ** 19)
            ref = ao.act_fwd(z, act)
            what = f"linear_w4a8 {M}x{N}x{K} {kw} {act} bias={b is not None}"
            ybuf, yv = ao.padded(M, N, torch.float32, ao.SENTINEL, dev)
            entry(xin[src], sxv, qin[src], ev, bv, yv, act, **kw)
            y = yv.detach().to(ao.CPU)
            if act == "sigmoid":
                assert bool(torch.isfinite(y).all()), what
                worst = max(worst, gc.f32_ulps(y, ref))
            else:
                assert torch.equal(y.double(), ref), f"{what} fp32: not the exact sum"
            ao.assert_padding_untouched(ybuf, M, N, what=f"{what} fp32")
            ybuf, yv = ao.padded(M, N, torch.bfloat16, ao.SENTINEL, dev)
            entry(xin[src], sxv, qin[src], ev, bv, yv, act, **kw)
            ao.assert_bf16_close(yv, ref, 1 if act == "sigmoid" else 0, f"{what} bf16")
            ao.assert_padding_untouched(ybuf, M, N, what=f"{what} bf16")
    assert worst <= sigmoid_f32_max_ulp, f"sigmoid fp32: {worst:.2f} ulp from fp64"
    return worst


def _unit_x(dev):
    """9 rows of 32 e4m3 codes: 1.0 in column 0 of row 0, zeros elsewhere; row scales 1."""
    assert fo.DEC[ONE] == 1.0
    xq = torch.zeros(9, 32, dtype=torch.uint8)
    xq[0, 0] = ONE
    return xq.to(dev), torch.ones(9, device=dev)


def check_decode(entry, dev, **kw):
    """16 codes times every scale byte the quantiser can write (15 .. 252), as 3808 neurons with
    K = 32 whose column 0 holds the code: y[0][n] = DEC[code] * 2^(E - 127) bit for bit after
    adding +0.0 (every such value is a normal fp32 or a zero), rows 1..8 are +0."""
    Es = np.arange(mo.E_MIN, mo.E_MAX + 1)
    N = 16 * len(Es)
    assert N == 3808
    code = np.zeros((N, 32), dtype=np.uint8)
    code[:, 0] = np.arange(N) % 16
    e = np.repeat(Es, 16).astype(np.uint8).reshape(N, 1).copy()
    xq, sx = _unit_x(dev)
    y = torch.full((9, N), ao.SENTINEL, dtype=torch.float32, device=dev)
    entry(xq, sx, torch.from_numpy(mo.pack(code)).to(dev), torch.from_numpy(e).to(dev), None, y,
          "linear", **kw)
    got = y.cpu().numpy()
    want64 = mo.DEC[code[:, 0]] * np.exp2(e[:, 0].astype(np.float64) - 127)
    want = want64.astype(np.float32) + np.float32(0.0)
    assert np.array_equal(want.astype(np.float64), want64)  # exact in fp32
    assert np.array_equal(fo.bits32(got[0]), fo.bits32(want)), "the MFMA's decode differs"
    assert not fo.bits32(got[1:]).any()  # +0: no bit set


def check_zero_block(entry, dev, **kw):
    """A block with E = 0 gives +0 for all 16 codes (the hardware scale would be 2^-127)."""
    code = np.zeros((16, 32), dtype=np.uint8)
    code[:, 0] = np.arange(16)
    code[:, 1:] = 7  # junk: 6.0 against the zeros of x
    e = np.zeros((16, 1), dtype=np.uint8)
    xq, sx = _unit_x(dev)
    y = torch.full((9, 16), ao.SENTINEL, dtype=torch.float32, device=dev)
    entry(xq, sx, torch.from_numpy(mo.pack(code)).to(dev), torch.from_numpy(e).to(dev), None, y,
          "linear", **kw)
    assert not fo.bits32(y.cpu().numpy()).any(), "an E = 0 block contributed"


def chain_terms(K: int) -> int:
    """T of the summation bound: additions into one accumulator of linear_w4a8_kernel on its
    longest chain. Every tile gives a wave all of K for its outputs, one MFMA per 128-column
    k-step, and an MFMA adds its 128 products into the accumulator: 128 * ceil(K / 128) (the k
    loop's rounding up to whole trips only adds zeros)."""
    return 128 * -(-K // 128)


def summation_bound(K: int, mag: np.ndarray, bias: np.ndarray, u: float = 2.0 ** -24):
    """(T + 3) * u * (sx * sum |dec value| + |bias|): the product of an e4m3 value (4
    significant bits) and an e2m1 value (2) times a power of two is exact in fp32, so the error
    is that of the T additions, the row-scale multiply, the bias add and one spare unit, each at
    most u of the running magnitude."""
    return (chain_terms(K) + 3) * u * (mag + np.abs(bias))
