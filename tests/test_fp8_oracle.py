"""The fp8 hop format against its exact oracle (tests/_fp8_oracle.py), on the CPU path of
ops.quant_rows_fp8 / dequant_rows_fp8: bit for bit in codes, scales and bf16 output. The GPU
kernels meet the same oracle in tests/test_fp8_boundary_gpu.py."""
import numpy as np
import pytest
import torch

import _fp8_oracle as fo
from docker_dist_nn_amd import ops


def _cpu_quant(x):
    q = torch.full(x.shape, 0x55, dtype=torch.uint8)
    s = torch.full((x.shape[0],), -7.0)
    ops.quant_rows_fp8(x, q, s)
    return q, s


def _cpu_dequant(q, s, like):
    y = torch.full_like(like, 5.0)
    ops.dequant_rows_fp8(q, s, y)
    return y


def test_constants_match():
    assert ops.FP8_MAX == float(fo.FP8_MAX)
    assert ops.FP8_TINY_AMAX == float(fo.TINY_AMAX) == 2.0 ** -110
    # both quotients stay finite and normal in fp32 down to the threshold
    tiny = np.float32(fo.TINY_AMAX)
    assert np.isfinite(fo.FP8_MAX / tiny) and tiny / fo.FP8_MAX >= np.finfo(np.float32).tiny


def test_decode_table_is_e4m3fn():
    want = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double().numpy()
    nan = np.isnan(fo.DEC)
    assert np.array_equal(nan, np.isnan(want)) and nan.nonzero()[0].tolist() == [0x7F, 0xFF]
    assert np.array_equal(fo.DEC[~nan], want[~nan])
    assert np.array_equal(np.signbit(fo.DEC[~nan]), np.signbit(want[~nan]))  # 0x80 is -0


def test_encoder_inverts_the_table_and_breaks_ties_to_even():
    finite = np.array([c for c in range(256) if c & 0x7F != 0x7F], dtype=np.uint8)
    code, tie = fo.encode(fo.DEC[finite].astype(np.float32))
    assert np.array_equal(code, finite) and not tie.any()
    mid = ((fo.MAG[:-1] + fo.MAG[1:]) / 2).astype(np.float32)  # exact in fp32
    code, tie = fo.encode(mid)
    assert tie.all() and not (code & 1).any()
    assert np.array_equal(np.abs(code.astype(int) - np.arange(126)) <= 1, np.ones(126, bool))
    code, _ = fo.encode(np.array([-0.0, np.nan, np.inf, 463.9, 2.0 ** -10, 2.0 ** -10 * 1.001],
                                 dtype=np.float32))
    assert code.tolist() == [0x80, 0x7F, 0x7F, 0x7E, 0x00, 0x01]


def test_exhaustive_rows_match_oracle_ties_included():
    """Every bf16 value in [-448, 448] at inv = scale = 1: the CPU path (torch's software e4m3
    cast) equals the oracle on all of them; 252 are exact ties, rounded to the even code."""
    x = fo.case("exhaustive")
    q_ref, s_ref, tie, y_ref = fo.reference("exhaustive")
    assert int(tie.sum()) == 252 and not (q_ref[tie] & 1).any()
    assert np.all(s_ref == 1.0)
    vals = x.float().numpy()
    assert np.unique(vals[:, 1:]).size == 2 * 17377 - 1  # +0 and -0 count once here
    q, s = _cpu_quant(x)
    assert np.array_equal(fo.bits32(s), fo.bits32(s_ref))
    assert np.array_equal(q.numpy(), q_ref)
    assert torch.equal(fo.bits16(_cpu_dequant(q, s, x)), fo.bits16(y_ref))


@pytest.mark.parametrize("name", fo.CASES)
def test_cpu_path_equals_oracle(name):
    x = fo.case(name)
    q_ref, s_ref, _, y_ref = fo.reference(name)
    q, s = _cpu_quant(x)
    assert np.array_equal(fo.bits32(s), fo.bits32(s_ref)), "scales"
    diff = q.numpy() != q_ref
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} codes differ"
    y = _cpu_dequant(torch.from_numpy(q_ref), torch.from_numpy(s_ref), x)
    assert torch.equal(fo.bits16(y), fo.bits16(y_ref)), "dequantised bf16"
    fo.assert_round_trip(x, y, name)


@pytest.mark.parametrize("cols", fo.WIDTHS)
def test_finite_rows_stay_finite(cols):
    """Tiny-row rule: for every row of finite inputs the scale is finite and non-negative, no
    code is NaN and the dequantised row is finite; rows under 2^-110 arrive as zeros."""
    x = fo.case(f"special-{fo.N_SPECIAL}x{cols}")
    q, s = _cpu_quant(x)
    assert bool(torch.isfinite(s).all()) and bool((s >= 0).all())
    assert not bool(((q & 0x7F) == 0x7F).any())
    y = _cpu_dequant(q, s, x)
    assert bool(torch.isfinite(y.float()).all())
    for r in range(fo.N_SPECIAL):
        zero_row = bool((y[r] == 0).all()) and float(s[r]) == 0.0
        assert zero_row == (r in fo.SENT_AS_ZERO), r


def test_oracle_reproduces_reciprocal_overflow_without_the_rule(monkeypatch):
    """What the rule prevents: with the threshold at 0 the row [1e-37, -5e-38, ...] has
    inv = inf, NaN codes and a NaN round trip."""
    monkeypatch.setattr(fo, "TINY_AMAX", np.float32(0.0))
    x = fo.case(f"special-{fo.N_SPECIAL}x8")[6:7]
    with np.errstate(all="ignore"):
        q, s, _ = fo.quant_ref(x)
        y = fo.dequant_ref(q, s)
    assert ((q & 0x7F) == 0x7F).all() and bool(torch.isnan(y.float()).all())


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_inputs_do_not_come_back_finite(bad):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(6, 136, generator=g).to(torch.bfloat16)
    x[1] = 0
    x[2] *= 1e-36  # a row under the threshold apart from its non-finite element
    where = [(0, 0), (1, 7), (2, 135), (4, 64), (4, 65)]
    for r, c in where:
        x[r, c] = bad
    q, s = _cpu_quant(x)
    y = _cpu_dequant(q, s, x).float()
    for r, c in where:
        assert not bool(torch.isfinite(y[r, c])), (r, c)
    for r in (3, 5):  # rows without one are unaffected
        assert bool(torch.isfinite(y[r]).all())
