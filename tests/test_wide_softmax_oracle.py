"""The tight bounds of tests/_wide_softmax_oracle.py checked without a GPU: the chain depth they
are derived from, the mutants of the oracle they must reject at every tested width (including
the one lo's serial-sum bound cannot see), and the CPU path of ops.softmax_xent /
ops.softmax_rows run through the cases the GPU tests use, so both meet one oracle."""
import pytest
import torch

import _loss_oracle as lo
import _wide_softmax_oracle as wo

CPU = torch.device("cpu")


def test_kernel_depth_matches_the_sweep():
    """D = (terms of lane 0 - 1) serial roundings + 6 butterfly levels, counted here term by
    term from the column-to-lane map of the kernel."""
    for n_cls in (257, 290, 320, 512, 513, 1000, 1024, 1025, 2101, 32768):
        cols = torch.arange(n_cls)
        per_lane = torch.bincount((cols % 256) // 4, minlength=64)
        assert int(per_lane.max()) == int(per_lane[0])
        assert wo.kernel_depth(n_cls) == int(per_lane[0]) - 1 + 6
        assert wo.kernel_depth(n_cls) < n_cls - 1
    assert [wo.kernel_depth(n) for n in (257, 1000, 1025, 2101)] == [10, 21, 22, 41]


def test_wide_case_keeps_the_shared_edge_rows():
    for _, n_cls in wo.WIDE_SHAPES:
        base, case = lo.logits_case(300, n_cls, seed=5), wo.wide_case(300, n_cls, seed=5)
        keep = torch.ones(300, dtype=torch.bool)
        keep[[4, 5]] = False
        assert torch.equal(base["x"][keep], case["x"][keep])
        assert torch.equal(base["labels"][keep], case["labels"][keep])
        ref = lo.xent_ref(case["x"], case["labels"], 1.0)
        assert ref["argmax"][:6].tolist() == [0, n_cls // 3, 0, n_cls // 2, n_cls - 1, 256]
        assert ref["correct"][:6].tolist() == [False, False, False, True, True, False]
    short = wo.wide_case(5, 300, seed=5)
    assert torch.equal(short["x"], lo.logits_case(5, 300, seed=5)["x"])


def _judge(case, width, scale, mutant=None):
    wo.judge_softmax_xent(wo.oracle_outputs(case, width, scale, mutant), case, width, scale)


@pytest.mark.parametrize("width,n_cls", wo.WIDE_SHAPES)
def test_tight_comparators_reject_the_mutants(width, n_cls):
    case = wo.wide_case(300, n_cls, seed=width + n_cls)
    for scale in (1.0, 1.0 / 300):
        _judge(case, width, scale)
        for mutant in wo.MUTANTS:
            if mutant == "pad_col_nonzero" and width == n_cls:
                continue  # no padding column to spoil
            with pytest.raises(AssertionError):
                _judge(case, width, scale, mutant)


def test_serial_sum_bound_misses_the_dropped_chunk():
    """Why the tight bounds exist: on an all-equal row of 1000 classes the probabilities with
    one 64-column chunk missing from the sum stay inside lo's (n_cls + 8) u -- and far outside
    the bound derived from the kernel's chain."""
    n_cls = 1000
    x = torch.full((1, n_cls), 2.5, dtype=torch.float64)
    ref = lo.xent_ref(x, torch.tensor([n_cls - 1], dtype=torch.int32), 1.0)
    wrong = torch.full((1, n_cls), 1.0 / (n_cls - 64), dtype=torch.float64)
    assert float((wrong - ref["p"]).abs().max()) > wo.p_terms(n_cls) * wo.U * 10
    with pytest.raises(AssertionError):
        wo.assert_probs_tight(wrong, ref)
    wrong1 = torch.full((1, n_cls), 1.0 / (n_cls - 50), dtype=torch.float64)
    lo.assert_probs(wrong1, ref)  # 50 missing columns pass the serial-sum bound ...
    with pytest.raises(AssertionError):
        wo.assert_probs_tight(wrong1, ref)  # ... and not this one


@pytest.mark.parametrize("width,n_cls", wo.WIDE_SHAPES)
def test_softmax_xent_wide_cases_on_cpu_path(width, n_cls):
    """The CPU reference path through the cases of the GPU test. Its summation order is
    torch's, not the kernel's: it is held to the depth any order satisfies, n_cls - 1."""
    stats = lo.new_stats()
    for rows in lo.XENT_ROWS:
        case = wo.wide_case(rows, n_cls, seed=rows + n_cls)
        for scale in (1.0, 1.0 / rows):
            wo.check_softmax_xent(case, width, scale, CPU, stats, depth=n_cls - 1)
        wo.check_softmax_xent(case, width, 1.0 / rows, CPU, stats, depth=n_cls - 1,
                              colsum=False)
        wo.check_softmax_xent(case, width, 1.0, CPU, stats, depth=n_cls - 1, loss=False,
                              correct=False)
    for layout in wo.LAYOUTS:  # the three layouts of the alignment test exist on the CPU too
        out = wo.run_softmax_xent(case, width, 1.0 / rows, CPU, layout)
        wo.judge_softmax_xent(out, case, width, 1.0 / rows, depth=n_cls - 1)
    print("\n" + lo.statline(f"cpu softmax_xent wide {width}/{n_cls}", stats))


@pytest.mark.parametrize("n_cls", wo.ROWS_CLS)
def test_softmax_rows_wide_cases_on_cpu_path(n_cls):
    stats = lo.new_stats()
    for rows in lo.ROWS_ROWS:
        case = wo.wide_case(rows, n_cls, seed=3 * rows + n_cls)
        wo.check_softmax_rows(case, CPU, stats, depth=n_cls - 1)
    wo.check_softmax_rows(case, CPU, depth=n_cls - 1, out=False)
    wo.check_softmax_rows(case, CPU, depth=n_cls - 1, labels=False)
    wo.check_softmax_rows(case, CPU, depth=n_cls - 1, pred=False)
    wo.check_softmax_rows(case, CPU, depth=n_cls - 1, inplace=True)
    wo.check_softmax_rows(case, CPU, depth=n_cls - 1, base=7)
    print("\n" + lo.statline(f"cpu softmax_rows wide /{n_cls}", stats))


def test_host_side_checks_raise_before_a_launch():
    """Arguments that cannot be launched are refused with ValueError on either device path."""
    from docker_dist_nn_amd import ops
    lg = torch.zeros(64, 320)
    dz = torch.zeros(64, 320, dtype=torch.bfloat16)
    lab = torch.zeros(64, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.softmax_xent(lg, lab, dz, 321, 1.0)  # more classes than columns
    with pytest.raises(ValueError):
        ops.softmax_xent(lg[:, :256], lab, dz, 300, 1.0)  # logits narrower than n_cls
    with pytest.raises(ValueError):
        ops.softmax_xent(lg, lab, dz, 300, 1.0, colsum=torch.zeros(1, 319))  # narrow colsum
    with pytest.raises(ValueError):
        ops.softmax_xent(lg, lab, dz, 300, 1.0, loss_part=torch.zeros(0))
    with pytest.raises(ValueError):
        ops.softmax_rows(lg, None, 321)
    with pytest.raises(ValueError):
        ops.softmax_rows(lg, torch.zeros(64, 299), 300)  # out narrower than n_cls
