"""The weight-gradient oracle (tests/_wgrad_oracle.py) on the CPU: the public ops' reference
path meets it exactly at the cases the GPU tests run, and each of a handful of deliberately
wrong implementations -- the defects the GPU tests exist to catch -- is rejected by the checker
that would meet it."""
import pytest
import torch

import _wgrad_oracle as wo
from docker_dist_nn_amd import ops

CPU = wo.CPU
R, N, K = 448, 128, 192  # 7 k-steps; S = 7 is one step per split, S = 3 is uneven (2, 2, 3)


@pytest.fixture(scope="module")
def case():
    return wo.wgrad_case(R, N, K, seed=11)


# ---- the reference path of the ops meets the oracle -----------------------------------------

@pytest.mark.parametrize("form", wo.FORMS)
@pytest.mark.parametrize("S", [1, 3, 7])
def test_gemm_split_k_cpu(case, form, S):
    wo.check_split_k(case, form, S, CPU)


@pytest.mark.parametrize("form", wo.FORMS)
@pytest.mark.parametrize("S", [1, 3, 7])
def test_linear_wgrad_cpu(case, form, S):
    wo.check_split_k(case, form, S, CPU, run=wo.linear_wgrad_run(case, CPU))


def test_slab_ranges_follow_the_range_rule():
    assert [wo.slab_range(s, 3, 448) for s in range(3)] == [(0, 128), (128, 256), (256, 448)]
    assert [wo.slab_range(s, 7, 448) for s in range(7)] == [(64 * s, 64 * s + 64)
                                                             for s in range(7)]
    for S, Rr in ((5, 64 * 23), (256, 64 * 385), (9, 64 * 14)):  # cover, in order, 1 step apart
        r = [wo.slab_range(s, S, Rr) for s in range(S)]
        assert r[0][0] == 0 and r[-1][1] == Rr
        assert all(a[1] == b[0] for a, b in zip(r, r[1:]))
        steps = {(b - a) // 64 for a, b in r}
        assert max(steps) - min(steps) <= 1 and min(steps) >= 1


def test_operands_are_poisoned_and_aligned(case):
    for form in wo.FORMS:
        a, b, layout = wo.operands(case, form, CPU)
        for t, width in ((a, N), (b, K)):
            base = t._base
            assert t.stride(0) > t.shape[1] and t.stride(0) % 8 == 0 and t.stride(1) == 1
            assert t.storage_offset() % 8 == 0  # 16 bytes of bf16
            assert int(torch.isnan(base.float()).sum()) == base.numel() - t.numel()
            assert not torch.isnan(t.float()).any()
            logical = t if form == wo.ROWS else t.t()
            assert logical.shape == (R, width)
        assert torch.equal(a if form == wo.ROWS else a.t(), case["dz"])
        assert layout == (ops.MNMAJ if form == wo.ROWS else ops.KMAJ)


@pytest.mark.parametrize("cid,Rr,Nn,Kk,nwg,expect", wo.STREAMK_CASES,
                         ids=[c[0] for c in wo.STREAMK_CASES])
def test_streamk_cases_cpu(cid, Rr, Nn, Kk, nwg, expect):
    """Each case has the edge its name claims, the fp64 model of the two kernels reproduces the
    product, and the op's CPU path meets the checker."""
    g = wo.streamk_geometry(Nn, Kk, Rr, nwg)
    assert {k: g[k] for k in expect} == expect
    assert g["ipw"] <= g["ksteps"]  # at most two segments per workgroup
    assert max(nwg, g["tiles"]) >= g["launched"]  # the scratch holds every launched workgroup
    c = wo.wgrad_case(Rr, Nn, Kk, seed=nwg)
    assert torch.equal(wo.streamk_model(c, nwg), c["full"])
    wo.check_streamk(c, CPU, nwg)


def test_streamk_cases_cover_the_edges():
    gs = [wo.streamk_geometry(c[2], c[3], c[1], c[4]) for c in wo.STREAMK_CASES]
    assert {(g["bm"], g["bn"]) for g in gs} == {(128, 128), (128, 64), (64, 128), (64, 64)}
    assert any(g["launched"] % 8 for g in gs) and any(g["straddle"] for g in gs)
    assert any(g["ipw"] == 1 for g in gs) and any(g["ksteps"] == 1 for g in gs)
    assert any(c[4] < g["tiles"] for c, g in zip(wo.STREAMK_CASES, gs))


def test_group_problems_cpu():
    """The grouped cases: one 64x64 configuration the launch accepts (the planner's split count,
    kernel-default stages, under the size bound), workgroup counts that are no multiples of 8,
    a first item with >= 8 column tiles; the CPU path (which launches nothing) meets the
    checker."""
    probs = wo.group_problems()
    assert len(probs) >= 3 and len({S for _, S, _ in probs}) >= 3
    assert {acc for _, _, acc in probs} == {False, True}
    for c, S, _ in probs:
        p = ops.plan("wgrad", c["N"], c["K"], c["R"])
        assert p.tiles == (64, 64) and p.splits == S and not p.stages and not p.persist
        nwg = (c["N"] // 64) * (c["K"] // 64) * S
        assert nwg % 8 and nwg < 256
    assert probs[0][0]["K"] // 64 == 9 and probs[0][0]["N"] // 64 == 5
    rest = wo.check_group(probs, CPU)
    assert rest == list(range(len(probs)))


@pytest.mark.parametrize("n_src", [1, 3, 8, 17, 40, 64, 128, 300])
def test_reductions_cpu(n_src):
    for acc in (False, True):
        rc = wo.reduce_case(n_src, 1024 + 64, n_src, acc)
        wo.check_reduce_slabs(rc, 0.25, CPU)
        wo.check_reduce_multi([rc, wo.reduce_case(3, 256, 5, not acc)], [0.5, 2.0], CPU)


@pytest.mark.parametrize("form", wo.FORMS)
def test_chain_cpu(case, form):
    wo.check_chain(case, form, 3, 0.125, CPU)


@pytest.mark.parametrize("form", wo.FORMS)
def test_raster_case_cpu(form):
    """The raster cases' shape arithmetic (partial last tile both ways, one k-step per split)
    and both raster checkers on the CPU path."""
    c = wo.raster_case(5, 9, (64, 64), 2, seed=4)
    assert (c["R"], c["N"], c["K"]) == (128, 4 * 64 + 24, 8 * 64 + 40)
    wo.check_split_k(c, form, 2, CPU, accumulate=False, tiles=(64, 64), group_m=3)
    c1 = wo.raster_case(5, 9, (64, 64), 1, seed=5)
    assert float((c1["full"].abs().max())) > 64  # the bf16 output is not trivially small
    wo.check_raster_bf16(c1, form, CPU, (64, 64), group_m=3)


def test_random_bound_cpu():
    c = wo.wgrad_case(64 * 23, 128, 192, seed=3, random=True)
    for form in wo.FORMS:
        ratio = wo.random_ratio(wo.reduced_gradient(c, form, 5, CPU), c, 5)
        assert 0.0 < ratio <= 1.0
    # an error of one part in 2^12 of the product's magnitude is far outside the bound
    off = c["full"] + c["absprod"] * 2.0 ** -12
    assert wo.random_ratio(off.float(), c, 5) > 1.0


# ---- deliberately wrong implementations: every one must be rejected -------------------------

def _fill(slabs, vals, accumulate):
    if accumulate:
        slabs += vals.float()
    else:
        slabs.copy_(vals.float())


def _logical(a, b, layout):
    """dz[R][N], x[R][K] in fp64 from the operand views."""
    return (a.double(), b.double()) if layout == ops.MNMAJ else (a.t().double(), b.t().double())


def _right_slabs(dz, x, S, Rr):
    rows = [slice(*wo.slab_range(s, S, Rr)) for s in range(S)]
    return torch.stack([dz[r].t() @ x[r] for r in rows])


def wrong_even_ranges(a, b, slabs, layout, Nn, Kk, Rr, S, accumulate=False):
    """ceil(ks / S) steps per split instead of the floor rule: the sum is still right."""
    dz, x = _logical(a, b, layout)
    per = -(-(Rr // 64) // S) * 64
    _fill(slabs, torch.stack([dz[s * per:(s + 1) * per].t() @ x[s * per:(s + 1) * per]
                              for s in range(S)]), accumulate)


def wrong_dropped_step(a, b, slabs, layout, Nn, Kk, Rr, S, accumulate=False):
    """The last split stops one 64-row step early."""
    dz, x = _logical(a, b, layout)
    out = []
    for s in range(S):
        r0, r1 = wo.slab_range(s, S, Rr)
        r1 -= 64 if s == S - 1 else 0
        out.append(dz[r0:r1].t() @ x[r0:r1])
    _fill(slabs, torch.stack(out), accumulate)


def wrong_swapped_tiles(a, b, slabs, layout, Nn, Kk, Rr, S, accumulate=False):
    """Two 64x64 output tiles of the last slab change places (one visited twice in effect)."""
    dz, x = _logical(a, b, layout)
    out = _right_slabs(dz, x, S, Rr)
    t0 = out[S - 1, :64, :64].clone()
    out[S - 1, :64, :64] = out[S - 1, 64:128, 64:128]
    out[S - 1, 64:128, 64:128] = t0
    _fill(slabs, out, accumulate)


def wrong_ldc(a, b, slabs, layout, Nn, Kk, Rr, S, accumulate=False):
    """Rows of every slab stored Kk apart instead of the view's leading dimension."""
    dz, x = _logical(a, b, layout)
    for s in range(S):
        r0, r1 = wo.slab_range(s, S, Rr)
        dense = torch.as_strided(slabs, (Nn, Kk), (Kk, 1),
                                 slabs.storage_offset() + s * slabs.stride(0))
        _fill(dense, dz[r0:r1].t() @ x[r0:r1], accumulate)


def wrong_nan_neighbour(a, b, slabs, layout, Nn, Kk, Rr, S, accumulate=False):
    """The last split's k-range runs one row into the neighbouring micro-batch."""
    if layout == ops.MNMAJ:
        a1 = torch.as_strided(a, (Rr + 1, Nn), a.stride(), a.storage_offset())
        b1 = torch.as_strided(b, (Rr + 1, Kk), b.stride(), b.storage_offset())
    else:
        a1 = torch.as_strided(a, (Nn, Rr + 1), a.stride(), a.storage_offset()).t()
        b1 = torch.as_strided(b, (Kk, Rr + 1), b.stride(), b.storage_offset()).t()
    dz, x = a1.double(), b1.double()
    out = []
    for s in range(S):
        r0, r1 = wo.slab_range(s, S, Rr)
        r1 += 1 if s == S - 1 else 0
        out.append(dz[r0:r1].t() @ x[r0:r1])
    _fill(slabs, torch.stack(out), accumulate)


WRONG = [wrong_even_ranges, wrong_dropped_step, wrong_swapped_tiles, wrong_ldc,
         wrong_nan_neighbour]


@pytest.mark.parametrize("form", wo.FORMS)
@pytest.mark.parametrize("wrong", WRONG, ids=lambda f: f.__name__)
def test_split_k_checker_rejects(case, form, wrong):
    with pytest.raises(AssertionError):
        wo.check_split_k(case, form, 3, CPU, run=wrong)


@pytest.mark.parametrize("form", wo.FORMS)
def test_split_k_checker_accepts_the_right_model(case, form):
    """The same scaffolding with the defect taken out passes: the rejections above are due to
    the defects."""
    def right(a, b, slabs, layout, Nn, Kk, Rr, S, accumulate=False):
        dz, x = _logical(a, b, layout)
        _fill(slabs, _right_slabs(dz, x, S, Rr), accumulate)
    wo.check_split_k(case, form, 3, CPU, run=right)


def test_group_checker_rejects_a_wrong_item():
    def run(items):
        rest = wo.group_run(items)
        items[2][2][1, :64, :64] += 1.0  # one tile of one slab of one item
        return rest
    with pytest.raises(AssertionError):
        wo.check_group(wo.group_problems(), CPU, run=run)


def test_group_checker_rejects_an_item_left_out():
    with pytest.raises(AssertionError, match="left out"):
        wo.check_group(wo.group_problems(), CPU, must_launch=True)


def test_streamk_checker_rejects_first_segment_everywhere(case):
    """A reduce that takes segment 0 where segment 1 belongs (R = 448, N = 128, K = 192, 5
    workgroups: shares of 5 steps over tiles of 7, two segments per workgroup)."""
    assert wo.streamk_geometry(N, K, R, 5)["straddle"]
    wrong = wo.streamk_model(case, 5, first_segment_always=True)
    assert not torch.equal(wrong, case["full"])

    def run(dz, x, grad, part, accumulate, nwg):
        if accumulate:
            grad += wrong.float()
        else:
            grad.copy_(wrong.float())
    with pytest.raises(AssertionError):
        wo.check_streamk(case, CPU, 5, run=run)
    # without a straddling share the same defect changes nothing: the case matters
    assert torch.equal(wo.streamk_model(case, 3, first_segment_always=True), case["full"])


def test_streamk_checker_rejects_scratch_overrun(case):
    def run(dz, x, grad, part, accumulate, nwg):
        wo.streamk_run(dz, x, grad, part, accumulate, nwg)
        torch.as_strided(part, (part.numel() + 1,), (1,), part.storage_offset())[-1] = 0.0
    with pytest.raises(AssertionError, match="outside"):
        wo.check_streamk(case, CPU, 5, run=run)


def test_reduce_checker_rejects():
    rc = wo.reduce_case(17, 512, 1, True)

    def skips_a_source(src, n_src, stride, n, out, scale=1.0, accumulate=False):
        ops.reduce_slabs(src, n_src - 1, stride, n, out, scale=scale, accumulate=accumulate)

    def reads_the_gap(src, n_src, stride, n, out, scale=1.0, accumulate=False):
        ops.reduce_slabs(src, n_src, stride, n + 1, out, scale=scale, accumulate=accumulate)
    for run in (skips_a_source, reads_the_gap):
        with pytest.raises(AssertionError):
            wo.check_reduce_slabs(rc, 0.25, CPU, run=run)
