"""The MXFP4 weight format against its exact oracle (tests/_mxfp4_oracle.py): the oracle against
itself and the specification, then the CPU path of ops.quant_rows_mxfp4 / dequant_rows_mxfp4
bit for bit in codes, scale bytes and bf16 output. The GPU kernels meet the same oracle in
tests/test_gemv_mxfp4_gpu.py."""
import numpy as np
import pytest
import torch

import _mxfp4_oracle as mo
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.ops import reference as ref

Q_FILL, E_FILL = 0x55, 0xEE


def _cpu_quant(x):
    rows, cols = x.shape
    q = torch.full((rows, cols // 2), Q_FILL, dtype=torch.uint8)
    e = torch.full((rows, cols // 32), E_FILL, dtype=torch.uint8)
    ops.quant_rows_mxfp4(x, q, e)
    return q.numpy(), e.numpy()


def _cpu_dequant(q, e, like):
    y = torch.full_like(like, 5.0)
    ops.dequant_rows_mxfp4(torch.as_tensor(q), torch.as_tensor(e), y)
    return y


def test_decode_tables_agree():
    assert mo.DEC.tolist() == [0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6]
    got = ref.e2m1_table().numpy()
    assert np.array_equal(got.view(np.int64), mo.DEC.view(np.int64))  # -0 included
    assert ops.MXFP4_BLOCK == mo.BLOCK == 32


def test_encoder_inverts_the_table_and_breaks_ties_to_even():
    code, tie = mo.encode(mo.DEC.copy())
    assert np.array_equal(code, np.arange(16)) and not tie.any()
    # the tie table of the specification
    ties = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    code, tie = mo.encode(ties)
    assert tie.all() and mo.MAG[code].tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    assert not (code & 1).any()
    code, tie = mo.encode(-ties)
    assert tie.all() and mo.DEC[code].tolist() == [-0.0, -1.0, -1.0, -2.0, -2.0, -4.0, -4.0]
    assert code[0] == 0x8  # a negative value that rounds to zero keeps its sign
    # one bf16 step to either side of each tie goes to the nearer magnitude
    eps = 2.0 ** -9
    lo, _ = mo.encode(ties * (1 - eps))
    hi, _ = mo.encode(ties * (1 + eps))
    assert lo.tolist() == [0, 1, 2, 3, 4, 5, 6] and hi.tolist() == [1, 2, 3, 4, 5, 6, 7]
    # the saturation interval (6, 8)
    code, tie = mo.encode(np.array([6.0, 6.03125, 7.0, 7.96875, -7.96875, -0.0]))
    assert code.tolist() == [7, 7, 7, 7, 15, 8] and not tie.any()


def test_exhaustive_rows_match_oracle_ties_included():
    """Every bf16 value below 8 in magnitude at E = 127 (t = x): the CPU path equals the oracle
    on all of them; the exact ties are the 7 of the table, once per sign, each on the even
    code; the round trip meets the format's bound with the worst ratio exactly 1."""
    x = mo.case("exhaustive")
    q_ref, e_ref, tie, y_ref = mo.reference("exhaustive")
    vals = x.float().numpy()
    assert np.unique(np.abs(vals)).size == mo.N_BELOW_8 and x.shape == (34, 1024)
    assert np.unique(vals).size == 2 * mo.N_BELOW_8 - 1  # +0 and -0 count once here
    assert (e_ref == 127).all()
    assert int(tie.sum()) == 14 and not (mo.unpack(q_ref)[tie] & 1).any()
    assert sorted(np.abs(vals[tie]).tolist()) == [.25, .25, .75, .75, 1.25, 1.25, 1.75, 1.75,
                                                  2.5, 2.5, 3.5, 3.5, 5.0, 5.0]
    codes = mo.unpack(q_ref)
    assert (codes[(np.abs(vals) > 6.0)] & 7 == 7).all()
    assert (codes[np.signbit(vals)] & 8 == 8).all() and (codes[~np.signbit(vals)] & 8 == 0).all()
    q, e = _cpu_quant(x)
    assert np.array_equal(e, e_ref) and np.array_equal(q, q_ref)
    y = _cpu_dequant(q, e, x)
    assert torch.equal(mo.bits16(y), mo.bits16(y_ref))
    assert mo.assert_format_bound(x, y, e_ref, "exhaustive") == 1.0


@pytest.mark.parametrize("name", mo.CASES)
def test_cpu_path_equals_oracle(name):
    x = mo.case(name)
    q_ref, e_ref, _, y_ref = mo.reference(name)
    # E in [15, 252] or 0; a zero block has every nibble 0x0
    assert (((e_ref >= mo.E_MIN) & (e_ref <= mo.E_MAX)) | (e_ref == 0)).all()
    zero = np.repeat(e_ref == 0, mo.BLOCK, axis=1)
    assert (mo.unpack(q_ref)[zero] == 0).all()
    # the dequantiser is exact in bf16: no rounding anywhere
    assert np.array_equal(y_ref.double().numpy(), mo.values(q_ref, e_ref))
    q, e = _cpu_quant(x)
    assert np.array_equal(e, e_ref), "scale bytes"
    diff = q != q_ref
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} code bytes differ"
    y = _cpu_dequant(q_ref, e_ref, x)
    assert torch.equal(mo.bits16(y), mo.bits16(y_ref)), "dequantised bf16"
    ratio = mo.assert_format_bound(x, y, e_ref, name)
    assert ratio <= 1.0


@pytest.mark.parametrize("cols", mo.WIDTHS)
def test_special_rows(cols):
    """Zero blocks (and only they) carry E = 0 and dequantise to +0; the threshold row has
    E = 15, bf16's largest magnitude E = 252; scales are per block; a subnormal inside a normal
    block keeps its sign on the zero code."""
    x = mo.case(f"special-{mo.N_SPECIAL}x{cols}")
    q, e, _, y = mo.reference(f"special-{mo.N_SPECIAL}x{cols}")
    codes = mo.unpack(q)
    for r in range(mo.N_SPECIAL):
        assert bool((e[r] == 0).all()) == (r in mo.ZERO_ROWS), r
    for r in mo.ZERO_ROWS:
        assert (codes[r] == 0).all()
        assert (mo.bits16(y[r]) == 0).all()  # +0, the -0 of row 0 included
    # an amax sits in the top binade of its block's grid: -3 = -6 * 2^-1, 1.5 = 6 * 2^-2
    assert (e[1, :-1] == 0).all() and e[1, -1] == 126 and codes[1, -1] == 0x8 | 7
    assert float(y[1, -1]) == -3.0
    assert set((codes[2] & 7).tolist()) == {7} and (e[2] == 125).all()
    assert torch.equal(mo.bits16(y[2]), mo.bits16(x[2]))
    assert (e[5] == 15).all() and e[7].min() == 15 and e[7].max() <= 16  # just above: 15 or 16
    assert e[8, 0] == 252
    nb = cols // mo.BLOCK
    if nb > 1:  # the last block keeps a grid of its own, 2^20 finer than its neighbour's
        assert int(e[3, -2]) - int(e[3, -1]) == 20
        assert codes[3, -mo.BLOCK] == codes[3, -2 * mo.BLOCK] == 7  # 1.75 = 7 * 2^-2: saturates
    assert (codes[3] & 7 == 0).any()  # small elements round to zero inside their block
    assert codes[9, 3] == 0x0 and codes[9, 5] == 0x8


def test_tiny_threshold():
    """A block whose amax is the largest bf16 below 2^-110 is a zero block; at 2^-110 it is
    not."""
    x = torch.zeros(2, 32, dtype=torch.bfloat16)
    x[0, 7], x[1, 7] = mo.BELOW_TINY, 2.0 ** -110
    q, e, _ = mo.quant_ref(x)
    assert e[:, 0].tolist() == [0, 15] and (q[0] == 0).all()
    assert mo.unpack(q)[1, 7] == 6  # 2^-110 = 4 * 2^(15 - 127)
    assert ref.MXFP4_TINY_EXP_FIELD == 17  # the bf16 exponent field of 2^-110


def test_ops_reject_bad_operands():
    x = torch.zeros(2, 64, dtype=torch.bfloat16)
    q = torch.zeros(2, 32, dtype=torch.uint8)
    e = torch.zeros(2, 2, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.quant_rows_mxfp4(x[:, :48], q, e)  # cols % 32
    with pytest.raises(ValueError):
        ops.quant_rows_mxfp4(x, q[:, :16], e)  # q too narrow
    with pytest.raises(ValueError):
        ops.dequant_rows_mxfp4(q, e[:, :1], x)  # e too narrow
    with pytest.raises(TypeError):
        ops.quant_rows_mxfp4(x, q.to(torch.int8), e)
    with pytest.raises(TypeError):
        ops.quant_rows_mxfp4(x.float(), q, e)
