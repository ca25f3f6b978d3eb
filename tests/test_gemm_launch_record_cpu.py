"""Which configuration every GEMM launch gets, record for record (no GPU: the native extension
is a recorder, tests/_gemm_launch_cases.py). tests/golden/gemm_launches.json was written before
the configuration choice moved into ops/gemm_plan.py; every tile, split count, stage code,
persist argument, layout, stride and library-path decision of every case must still be equal,
integers and floats alike, with no tolerance."""
import collections
import json

import pytest

import _gemm_launch_cases as C


@pytest.fixture(scope="module")
def golden():
    by_case = collections.defaultdict(list)
    for r in C.load_golden():
        by_case[r[0]].append(r)
    return by_case


CASES = C.cases()


def test_golden_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(c[0] for c in CASES)
    assert len(C.table_signatures()) >= 51 and len(C.SWITCH_SUBSET) >= 12


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_launches_match_record(golden, case):
    got = C.run_case(case)
    want = golden[case[0]]
    for g, w in zip(got, want):
        assert g == w
        # == lets 1 pass for 1.0 and True: the types must be those recorded, too
        assert json.dumps(g, sort_keys=True) == json.dumps(w, sort_keys=True)
    assert len(got) == len(want)


def test_recipe_wgrads_run_grouped(golden):
    recs = [r for r in golden["default|group"] if r[1] == "recipe"]
    assert [r[2] for r in recs] == ["gemm_bf16_group", "returned"]
    assert len(recs[0][3][0]) == len(C.RECIPE) and recs[1][3] == [[]]
    mixed = [r for r in golden["default|group"] if r[1] == "mixed"]
    assert any(r[2] == "gemm_bf16_group" for r in mixed) and mixed[-1][3][0]  # some of each
