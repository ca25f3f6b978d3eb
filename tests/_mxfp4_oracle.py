"""Exact oracle of the MXFP4 weight format (ops.quant_rows_mxfp4 / dequant_rows_mxfp4 /
gemv_mxfp4), shared by the CPU and GPU tests. numpy only, integer and fp64 arithmetic -- no fp4
cast of torch or of the hardware is involved, so both can be compared with it bit for bit.

The format (OCP microscaling FP4): a row of K bf16 values, K % 32 == 0. An element is a 4-bit
code s|ee|m whose magnitude is one of {0, 0.5, 1, 1.5, 2, 3, 4, 6}, indexed by the low 3 bits;
bit 3 is the sign. Byte j of a row holds column 2j in its low nibble and column 2j + 1 in its
high one. One byte E per 32 consecutive columns, in a tensor of its own, is the block's scale
2^(E - 127).

Quantiser, per block: amax = max |x|. amax < 2^-110: a zero block, E = 0 and all 32 nibbles 0x0.
Otherwise E = floor(log2 amax) - 2 + 127 (always in [15, 252]), t = x * 2^(127 - E) (exact,
|t| < 8), |t| > 6 saturates to 6, otherwise t rounds to the nearest magnitude, a tie to the even
code; the sign comes from the sign bit (a -0 or a negative value that rounds to 0 is 0x8).
Dequantiser: bf16(dec(code) * 2^(E - 127)); a block with E == 0 gives +0. For E in [15, 252]
every value is a normal bf16 with two significant bits: exact, no rounding anywhere.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from _act_oracle import rn_bf16

BLOCK = 32
TINY_AMAX = 2.0 ** -110  # blocks below it are zero blocks
MAG = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])  # index = code & 7
E_MIN, E_MAX = 15, 252  # range of the scale byte of a block that is not a zero block


# ---- the 16 codes ---------------------------------------------------------------------------

def decode_table() -> np.ndarray:
    """fp64 value of every code, from the bit fields: 1 sign, 2 exponent bits with bias 1, 1
    mantissa bit, subnormals at exponent 0; no NaN and no infinity."""
    out = np.empty(16, dtype=np.float64)
    for c in range(16):
        s, e, m = c >> 3, (c >> 1) & 3, c & 1
        v = m * 0.5 if e == 0 else (1.0 + m / 2.0) * 2.0 ** (e - 1)
        out[c] = -v if s else v
    return out


DEC = decode_table()
assert np.array_equal(DEC[:8], MAG) and np.array_equal(DEC[8:], -MAG) and np.signbit(DEC[8])


def encode(t: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """fp64 t with |t| < 8 -> (code, exact-tie mask): the nearest of the 8 magnitudes, anything
    above 6 saturating to 6, a tie to the even code, the sign from the sign bit (-0 -> 0x8)."""
    assert t.dtype == np.float64
    a = np.abs(t)
    assert np.isfinite(a).all() and (a < 8.0).all()
    hi = np.minimum(np.searchsorted(MAG, a, side="left"), 7)  # first magnitude >= a
    lo = np.maximum(hi - 1, 0)
    dlo, dhi = a - MAG[lo], MAG[hi] - a  # exact: t has at most 8 significant bits
    tie = (dlo == dhi) & (hi != lo)
    code = np.where(dhi < dlo, hi, lo)
    code = np.where(tie, np.where(lo % 2 == 0, lo, hi), code)
    code = np.where(a > 6.0, 7, code)
    code = code | np.where(np.signbit(t), 8, 0)
    return code.astype(np.uint8), tie


def pack(code: np.ndarray) -> np.ndarray:
    """[rows][K] codes -> [rows][K / 2] bytes: column 2j low, column 2j + 1 high."""
    return (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)


def unpack(q: np.ndarray) -> np.ndarray:
    """[rows][K / 2] bytes -> [rows][K] codes."""
    out = np.empty((q.shape[0], q.shape[1] * 2), dtype=np.uint8)
    out[:, 0::2], out[:, 1::2] = q & 15, q >> 4
    return out


# ---- reference quantiser / dequantiser ------------------------------------------------------

def quant_ref(x: torch.Tensor):
    """bf16 [rows][cols] of finite values -> (packed codes uint8 [rows][cols / 2], scale bytes
    uint8 [rows][cols / 32], tie mask [rows][cols]), numpy."""
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] % BLOCK == 0
    rows, cols = x.shape
    xd = x.double().numpy().reshape(rows, cols // BLOCK, BLOCK)
    assert np.isfinite(xd).all(), "the format is specified for finite rows only"
    amax = np.abs(xd).max(axis=2)
    send = amax >= TINY_AMAX
    _, ex = np.frexp(np.where(send, amax, 1.0))  # amax = f * 2^ex, f in [0.5, 1)
    E = np.where(send, (ex - 1) - 2 + 127, 0)  # floor(log2 amax) = ex - 1
    assert ((E[send] >= E_MIN) & (E[send] <= E_MAX)).all()
    t = np.ldexp(xd, (127 - E)[:, :, None])  # exact: a power-of-two scaling inside fp64's range
    t = np.where(send[:, :, None], t, 0.0)
    code, tie = encode(t)
    code = np.where(send[:, :, None], code, 0)  # a zero block drops the signs too
    tie = tie & send[:, :, None]
    return pack(code.reshape(rows, cols)), E.astype(np.uint8), tie.reshape(rows, cols)


def values(q: np.ndarray, e: np.ndarray) -> np.ndarray:
    """fp64 [rows][K] of dec(code) * 2^(E - 127); +0 for a block with E == 0."""
    E = np.repeat(e.astype(np.int64), BLOCK, axis=1)
    v = np.ldexp(DEC[unpack(q)], E - 127)
    return np.where(E == 0, 0.0, v)


def dequant_ref(q: np.ndarray, e: np.ndarray) -> torch.Tensor:
    """(packed codes, scale bytes) -> bf16. The rounding of rn_bf16 never acts for E >= 15:
    tests/test_mxfp4_oracle.py asserts that the bf16 result equals the fp64 value."""
    return rn_bf16(torch.from_numpy(values(q, e)))


def format_bound(w64: np.ndarray, e: np.ndarray) -> np.ndarray:
    """Per element |deq - w| <= max(2^(E - 127) / 4, |w| / 4), exact and without slack: a
    quarter of the block's scale is half the finest step of the grid (0.5), a quarter of |w|
    covers half a step at the bottom of the coarse binades (2 -> 3: step 1, 4 -> 6: step 2) and
    the saturating interval (6, 8): 8 - 6 = 8 / 4. A zero block (E == 0): |w| < 2^-110 is
    dropped, covered by |w| itself."""
    E = np.repeat(e.astype(np.int64), BLOCK, axis=1)
    bound = np.maximum(np.ldexp(0.25, E - 127), np.abs(w64) / 4.0)
    return np.where(E == 0, np.abs(w64), bound)


def bits16(t: torch.Tensor) -> torch.Tensor:
    assert t.dtype == torch.bfloat16
    return t.detach().cpu().contiguous().view(torch.int16)


# ---- cases ----------------------------------------------------------------------------------

# rows x cols: smallest legal width; rows not a multiple of 4 (a block of threads holds 4 rows);
# an odd number of blocks; more than 4 rows with an odd block count; 32 blocks; one block more
SHAPES = [(1, 32), (3, 64), (5, 160), (33, 544), (64, 1024), (7, 1056)]
WIDTHS = [c for _, c in SHAPES]
EXHAUSTIVE_COLS = 1024


def _bf16(bits: int) -> float:
    return float(torch.tensor([bits], dtype=torch.int16).view(torch.bfloat16)[0])


BF16_MAX = _bf16(0x7F7F)
BELOW_TINY = _bf16(0x087F)  # the largest bf16 below 2^-110 (0x0880)
N_BELOW_8 = 0x4100  # bf16 bit patterns of the magnitudes below 8.0 (0x4100), zero included


def exhaustive_rows() -> torch.Tensor:
    """Every bf16 value with |v| < 8, both signs (2 * 16640 of them), 31 to a block behind a
    leading 4.0: amax is in [4, 8), so E = 127 and t = x in every block. Rows of 1024 columns;
    the tail of the last row is padded with zeros behind its leading 4.0s."""
    pos = torch.arange(0, N_BELOW_8, dtype=torch.int32)
    allv = torch.cat([pos, pos + 0x8000])
    allv = torch.where(allv >= 0x8000, allv - 0x10000, allv).to(torch.int16).view(torch.bfloat16)
    per_row = (EXHAUSTIVE_COLS // BLOCK) * (BLOCK - 1)
    rows = -(-allv.numel() // per_row)
    body = torch.zeros(rows * per_row, dtype=torch.bfloat16)
    body[:allv.numel()] = allv
    x = torch.zeros(rows, EXHAUSTIVE_COLS // BLOCK, BLOCK, dtype=torch.bfloat16)
    x[:, :, 0] = 4.0
    x[:, :, 1:] = body.view(rows, EXHAUSTIVE_COLS // BLOCK, BLOCK - 1)
    return x.view(rows, EXHAUSTIVE_COLS)


def special_rows(cols: int) -> torch.Tensor:
    """One row per edge of the format, at any legal width."""
    g = torch.Generator().manual_seed(2000 + cols)
    sign = lambda: torch.randint(0, 2, (cols,), generator=g).float() * 2 - 1  # noqa: E731
    mant = lambda: 1.0 + torch.rand(cols, generator=g)  # noqa: E731
    last = cols - BLOCK  # first column of the last block
    rows = []
    z = torch.zeros(cols)
    z[1] = -0.0
    rows.append(z)  # all zero, one of them -0: zero blocks, the sign is dropped
    one = torch.zeros(cols)
    one[cols - 1] = -3.0
    rows.append(one)  # a single non-zero element, in the last column
    rows.append(sign() * 1.5)  # +-amax only
    # per-block scales: in every block the small elements round to zero against its amax; the
    # last block's amax is 2^20 times smaller than its neighbours' and must keep its own grid
    per = sign() * mant() * torch.pow(2.0, -torch.randint(0, 8, (cols,), generator=g).float())
    per[::BLOCK] = 1.75
    per[last:] = per[last:] * 2.0 ** -20
    rows.append(per)
    below = sign() * mant() * 2.0 ** -113
    below[2] = BELOW_TINY
    rows.append(below)  # every block just below 2^-110: zero blocks
    at = sign() * mant() * torch.pow(2.0, -111 - torch.randint(0, 24, (cols,), generator=g).float())
    at[::BLOCK] = 2.0 ** -110
    rows.append(at)  # every block's amax exactly the threshold: E = 15
    sub = torch.zeros(cols)
    sub[:4] = torch.tensor([1e-37, -5e-38, 2e-38, 1e-40])
    rows.append(sub)  # bf16 subnormals among values under the threshold: zero blocks
    above = sign() * mant() * torch.pow(2.0, -110 - torch.randint(0, 8, (cols,), generator=g).float())
    above[::BLOCK] = -1.5 * 2.0 ** -110
    rows.append(above)  # just above
    top = torch.randn(cols, generator=g) * 1e38
    top[4 % cols], top[6 % cols] = BF16_MAX, -BF16_MAX
    rows.append(top.clamp(-BF16_MAX, BF16_MAX))  # bf16's largest finite magnitude: E = 252
    mixed = sign() * mant()
    mixed[3] = 1e-39  # a bf16 subnormal inside a normal block: rounds to +0
    mixed[5] = -1e-39  # and to -0
    rows.append(mixed)
    return torch.stack(rows).to(torch.bfloat16)


N_SPECIAL = 10
ZERO_ROWS = (0, 4, 6)  # rows of special_rows whose every block is a zero block


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
    """(packed codes, scale bytes, ties, dequantised bf16) of a case, computed once."""
    q, e, tie = quant_ref(case(name))
    return q, e, tie, dequant_ref(q, e)


def assert_format_bound(x: torch.Tensor, y: torch.Tensor, e: np.ndarray, what: str) -> float:
    """|y - x| <= format_bound, everything finite; returns the worst ratio."""
    xd, yd = x.cpu().double().numpy(), y.detach().cpu().double().numpy()
    assert np.isfinite(yd).all(), f"{what}: non-finite value from a finite row"
    bound, err = format_bound(xd, e), np.abs(yd - xd)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), f"{what}: round trip at {ratio:.6f} x the bound"
    return ratio
