"""The fp64 activation oracle (tests/_act_oracle.py) checked without a GPU: its comparator on
hand-made values, and its case generators and references run through the CPU path of the same
public ops the GPU tests call (ops.gemm / ops.dact_colsum / ops.bias_act_cast)."""
import pytest
import torch

import _act_oracle as ao
from docker_dist_nn_amd.ops import KMAJ, MNMAJ

CPU = torch.device("cpu")
bf = torch.bfloat16


def test_ulp_distance_and_single_rounding():
    a = torch.tensor([1.0, 1.0, -1.0, 0.0, 0.0, 1.0, float("nan")], dtype=bf)
    b = torch.tensor([1.0078125, 0.99609375, -1.0078125, -0.0, 2.0 ** -133, -1.0, 1.0], dtype=bf)
    #                 next up    next down    next down   same  smallest denormal
    assert ao.bf16_ulp_distance(a, b).tolist() == [1, 1, 1, 0, 1, 2 * 0x3F80, 1 << 16]
    # 1 + 2^-8 is the midpoint of 1 and 1 + 2^-7: just above it must round up, although
    # double -> float first rounds it ONTO the midpoint, which then goes to even (down)
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -8, -(1.0 + 2.0 ** -8 + 2.0 ** -40),
                      3.0 * 2.0 ** -8 + 1.0 - 2.0 ** -40], dtype=torch.float64)
    assert x.float().to(bf).tolist()[0] == 1.0  # the double rounding this guards against
    assert ao.rn_bf16(x).tolist() == [1.0078125, 1.0, -1.0078125, 1.0078125]
    assert ao.bf16_ulp(torch.tensor([1.0, 1.5, 0.75, 300.0])).tolist() == \
        [2.0 ** -7, 2.0 ** -7, 2.0 ** -8, 2.0]
    with pytest.raises(AssertionError, match="bf16 ulp"):
        ao.assert_bf16_close(torch.tensor([1.015625], dtype=bf), torch.tensor([1.0]), 1)
    with pytest.raises(AssertionError, match="NaN"):
        ao.assert_bf16_close(torch.tensor([float("nan")], dtype=bf), torch.tensor([1.0]), 1)


@pytest.mark.parametrize("la,lb", ao.LAYOUTS)
def test_forward_cases_on_cpu_path(la, lb):
    for (M, N, K) in ((152, 104, 64), (88, 168, 192)):
        ao.check_fwd(ao.fwd_case(M, N, K, la, lb, seed=M + la + 2 * lb), CPU, tiles=(128, 64))


@pytest.mark.parametrize("lb", [MNMAJ, KMAJ])
def test_backward_cases_on_cpu_path(lb):
    for (M, N, K) in ((152, 104, 64), (88, 168, 192), (128, 128, 64)):
        case = ao.bwd_case(M, N, K, lb, seed=M + lb)
        y = case["aux"].float()
        assert bool((y == 0).any()) and bool((y == 1).any()) and bool(((y > 0) & (y < 1)).any())
        ao.check_bwd(case, CPU, (64, 64))


def test_oracle_catches_the_mistakes_it_is_for():
    """A swapped column pair in the activation, or a derivative taken one row off, must not
    pass the oracle's comparison."""
    case = ao.bwd_case(72, 104, 64, MNMAJ, seed=1)
    ref = ao.act_bwd(case["prod"], case["aux"], "sigmoid")
    y = case["aux"].double()
    swapped = y.view(72, 52, 2).flip(2).reshape(72, 104)
    for wrong in (swapped, y.roll(1, 0)):
        bad = ao.rn_bf16(ao.act_bwd(case["prod"], wrong, "sigmoid"))
        with pytest.raises(AssertionError):
            ao.assert_bf16_close(bad, ref, 1)
    ao.assert_bf16_close(ao.rn_bf16(ref), ref, 0)


@pytest.mark.parametrize("act", ao.ACTS)
def test_elementwise_cases_on_cpu_path(act):
    ao.check_dact_colsum(ao.dact_case(200, 192, 5), act, CPU, 3)
    ao.check_dact_colsum(ao.dact_case(200, 192, 5), act, CPU, 3, with_part=False)
    for with_bias in (True, False):
        ao.check_bias_act_cast(ao.bias_case(200, 68, 6), act, CPU, with_bias)
