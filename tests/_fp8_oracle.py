"""Exact oracle of the fp8 pipeline-boundary format (ops.quant_rows_fp8 / dequant_rows_fp8),
shared by the CPU and GPU tests. numpy only, integer and fp64 arithmetic plus IEEE fp32
division and multiplication -- no fp8 cast of torch or of the hardware is involved, so both can
be compared with it bit for bit.

The format: per row, amax = max |x|, scale = fl32(amax / 448), inv = fl32(448 / amax) (IEEE
quotients), code = e4m3(fl32(x * inv)) with round to nearest, ties to the even code (OCP e4m3:
1 sign, 4 exponent bits with bias 7, 3 mantissa bits, subnormals at exponent 0, 0x7F / 0xFF =
NaN, no infinities, largest finite 448). A row with amax < 2^-110 is a zero row: scale = inv =
0. Dequantisation: bf16(fl32(dec(code) * scale)), round to nearest even.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from _act_oracle import rn_bf16

FP8_MAX = np.float32(448.0)
TINY_AMAX = np.float32(2.0 ** -110)  # rows below it are sent as zeros


# ---- the 256 codes --------------------------------------------------------------------------

def decode_table() -> np.ndarray:
    """fp64 value of every code, from the bit fields."""
    out = np.empty(256, dtype=np.float64)
    for c in range(256):
        s, e, m = c >> 7, (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = float("nan")
        elif e == 0:
            v = m * 2.0 ** -9  # subnormal: (m / 8) * 2^(1 - 7)
        else:
            v = (1.0 + m / 8.0) * 2.0 ** (e - 7)
        out[c] = -v if s else v
    return out


DEC = decode_table()
MAG = DEC[:127].copy()  # the 127 finite magnitudes 0 .. 448, ascending; index = code
assert MAG[126] == 448.0 and np.all(np.diff(MAG) > 0)


def encode(t: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """fp32 -> (code, exact-tie mask): the nearest of the 127 finite magnitudes, a tie to the
    even code, the sign from the sign bit (-0 -> 0x80). NaN, +-inf and magnitudes of 464 or
    more (nearer to the absent 480 than to 448) give the NaN code; no finite row produces one."""
    assert t.dtype == np.float32
    a = np.abs(t.astype(np.float64))
    bad = ~np.isfinite(a) | (a >= 464.0)
    a = np.where(bad, 0.0, a)
    hi = np.minimum(np.searchsorted(MAG, a, side="left"), 126)  # first magnitude >= a
    lo = np.maximum(hi - 1, 0)
    dlo, dhi = a - MAG[lo], MAG[hi] - a  # exact: both operands are fp32 values within 2^10
    tie = (dlo == dhi) & (hi != lo)
    code = np.where(dhi < dlo, hi, lo)
    code = np.where(tie, np.where(lo % 2 == 0, lo, hi), code)
    code = np.where(bad, 0x7F, code)
    code = code | np.where(np.signbit(t), 0x80, 0)
    return code.astype(np.uint8), tie & ~bad


# ---- reference quantiser / dequantiser ------------------------------------------------------

def quant_ref(x: torch.Tensor):
    """bf16 [rows][cols] of finite values -> (codes uint8, scale fp32, tie mask), numpy."""
    assert x.dtype == torch.bfloat16 and x.dim() == 2
    xf = x.float().numpy()
    assert np.isfinite(xf).all(), "the format is specified for finite rows only"
    amax = np.abs(xf).max(axis=1)
    send = amax >= TINY_AMAX
    safe = np.where(send, amax, np.float32(1.0))
    scale = np.where(send, safe / FP8_MAX, np.float32(0.0)).astype(np.float32)
    inv = np.where(send, FP8_MAX / safe, np.float32(0.0)).astype(np.float32)
    t = xf * inv[:, None]
    assert t.dtype == np.float32
    code, tie = encode(t)
    return code, scale, tie


def dequant_ref(q: np.ndarray, scale: np.ndarray) -> torch.Tensor:
    """(codes, scale) -> bf16: one fp32 multiply, one rounding to bf16 (nearest even)."""
    v = DEC.astype(np.float32)[q] * scale.astype(np.float32)[:, None]
    assert v.dtype == np.float32
    return rn_bf16(torch.from_numpy(v))


def round_trip_bound(x: torch.Tensor, amax: torch.Tensor) -> torch.Tensor:
    """Accuracy of the format itself against fp64: half an e4m3 step at the bottom of a binade
    (2^-4 relative) plus the bf16 rounding of the result, and half a subnormal step of the row
    (amax / 448 * 2^-9)."""
    x, amax = x.double(), amax.double()
    return (2.0 ** -4 + 2.0 ** -8) * x.abs() + (amax / 448.0) * 2.0 ** -10 * (1.0 + 2.0 ** -6)


def bits16(t: torch.Tensor) -> torch.Tensor:
    assert t.dtype == torch.bfloat16
    return t.detach().cpu().contiguous().view(torch.int16)


def bits32(a) -> np.ndarray:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.int32)


# ---- cases ----------------------------------------------------------------------------------

# rows x cols: smallest legal width; rows not a multiple of 4 (a block holds 4 rows); odd width;
# one full 512-column sweep plus one lane's tail; wider rows; two sweeps plus a tail
SHAPES = [(1, 8), (3, 64), (5, 136), (33, 520), (64, 1024), (7, 1032)]
WIDTHS = [c for _, c in SHAPES]
EXHAUSTIVE = (552, 64)


def _bf16(bits: int) -> float:
    return float(torch.tensor([bits], dtype=torch.int16).view(torch.bfloat16)[0])


BF16_MAX = _bf16(0x7F7F)
BELOW_TINY = _bf16(0x087F)  # the largest bf16 below 2^-110 (0x0880)


def exhaustive_rows() -> torch.Tensor:
    """Every bf16 value with |v| <= 448 (2 * 17377 of them), 63 to a row behind a leading 448:
    amax = 448, so scale = inv = 1 and t = x exactly. The last row is padded with zeros."""
    pos = torch.arange(0, 0x43E0 + 1, dtype=torch.int32)
    allv = torch.cat([pos, pos + 0x8000])
    allv = torch.where(allv >= 0x8000, allv - 0x10000, allv).to(torch.int16).view(torch.bfloat16)
    rows, cols = EXHAUSTIVE
    x = torch.zeros(rows, cols, dtype=torch.bfloat16)
    x[:, 0] = 448.0
    body = torch.zeros(rows * (cols - 1), dtype=torch.bfloat16)
    body[:allv.numel()] = allv
    x[:, 1:] = body.view(rows, cols - 1)
    return x


def special_rows(cols: int) -> torch.Tensor:
    """One row per edge of the format, at any legal width."""
    g = torch.Generator().manual_seed(1000 + cols)
    sign = lambda: torch.randint(0, 2, (cols,), generator=g).float() * 2 - 1  # noqa: E731
    mant = lambda: 1.0 + torch.rand(cols, generator=g)  # noqa: E731
    rows = []
    z = torch.zeros(cols)
    z[1] = -0.0
    rows.append(z)  # all zero, one of them -0
    one = torch.zeros(cols)
    one[cols - 1] = -3.0
    rows.append(one)  # a single non-zero element, in the last column
    rows.append(sign() * 1.5)  # +-amax only
    # more than 2^15 of dynamic range: the small ones land in e4m3 subnormals and at zero
    wide = sign() * mant() * torch.pow(2.0, -torch.randint(0, 21, (cols,), generator=g).float())
    wide[0], wide[cols - 1] = 1.75, 2.0 ** -20
    rows.append(wide)
    # tiny rows on both sides of the 2^-110 threshold
    below = sign() * mant() * 2.0 ** -113
    below[2] = BELOW_TINY
    rows.append(below)  # just below: sent as zeros
    at = sign() * mant() * torch.pow(2.0, -111 - torch.randint(0, 24, (cols,), generator=g).float())
    at[3] = 2.0 ** -110
    rows.append(at)  # amax exactly the threshold; the smallest elements are bf16 subnormals
    sub = torch.zeros(cols)
    sub[:4] = torch.tensor([1e-37, -5e-38, 2e-38, 1e-40])
    rows.append(sub)  # 448 / amax overflows fp32; holds bf16 subnormals: sent as zeros
    above = sign() * mant() * torch.pow(2.0, -110 - torch.randint(0, 8, (cols,), generator=g).float())
    above[5] = -1.5 * 2.0 ** -109
    rows.append(above)  # just above
    top = torch.randn(cols, generator=g) * 1e38
    top[4], top[6] = BF16_MAX, -BF16_MAX
    rows.append(top.clamp(-BF16_MAX, BF16_MAX))  # bf16's largest finite magnitude
    return torch.stack(rows).to(torch.bfloat16)


N_SPECIAL = 9
SENT_AS_ZERO = (0, 4, 6)  # rows of special_rows that must arrive as zero rows


@functools.lru_cache(maxsize=None)
def case(name: str) -> torch.Tensor:
    """bf16 input of a named case (see CASES); never modified by a test."""
    if name == "exhaustive":
        return exhaustive_rows()
    kind, shape = name.split("-")
    rows, cols = map(int, shape.split("x"))
    if kind == "special":
        x = special_rows(cols)
        assert x.shape[0] == rows
        return x
    g = torch.Generator().manual_seed(rows * 10007 + cols + len(kind))
    span = {"log6": 6.0, "log30": 30.0}[kind]
    x = torch.randn(rows, cols, generator=g) * torch.logspace(-span, span, max(rows, 2))[:rows, None]
    return x.to(torch.bfloat16)


CASES = [f"{k}-{r}x{c}" for k in ("log6", "log30") for r, c in SHAPES] + \
    [f"special-{N_SPECIAL}x{c}" for c in WIDTHS] + ["exhaustive"]


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(codes, scale, ties, dequantised bf16) of a case, computed once."""
    q, s, tie = quant_ref(case(name))
    return q, s, tie, dequant_ref(q, s)


def assert_round_trip(x: torch.Tensor, y: torch.Tensor, what: str) -> float:
    """|y - x| within round_trip_bound, everything finite; returns the worst ratio."""
    xf, yf = x.cpu().double(), y.detach().cpu().double()
    assert torch.isfinite(yf).all(), f"{what}: non-finite value from a finite row"
    bound = round_trip_bound(xf, xf.abs().amax(1, keepdim=True))
    # a row sent as zeros: the error is |x| < 2^-110 by the tiny-row rule
    bound = bound + float(TINY_AMAX) * (xf.abs().amax(1, keepdim=True) < float(TINY_AMAX))
    err = (yf - xf).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    assert bool((err <= bound).all()), f"{what}: round trip at {ratio:.3f} x the bound"
    return ratio
