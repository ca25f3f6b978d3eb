"""ops/gemm_plan.py against the launch record (tests/golden/gemm_launches.json): the GemmPlan
of every recorded product carries what its launch carried, the sizing helpers the engine
allocates from are views of the same plans, and the one switch parser keeps each switch's
validation."""
import collections
import warnings

import pytest

import _gemm_launch_cases as C
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.ops import gemm_plan as P

SETTINGS = {s["id"]: s for s in [C.DEFAULT, *C.SETTINGS]}
# gemm_bf16's positional arguments (csrc/bindings.cpp): ... bm, bn, splits at 18, 19, 20
BM, BN, SPLITS = 18, 19, 20
# the split count a wgrad variant passes, from the chosen one
WGRAD_SPLITS = {"s": lambda s: s, "acc": lambda s: s, "kk": lambda s: s, "s+1": lambda s: s + 1,
                "kk-s+1": lambda s: s + 1, "one": lambda s: 1, "upd": lambda s: 1}


def _parse(cid):
    setting, sig = cid.split("|")
    kind, dims = sig.split(":")
    return SETTINGS[setting], kind, tuple(map(int, dims.split("x")))


@pytest.fixture(scope="module")
def calls():
    """{case id: {call label: [records]}} of the cases that are one signature."""
    out = collections.defaultdict(lambda: collections.defaultdict(list))
    for cid, label, *rest in C.load_golden():
        if not cid.endswith("|group"):
            out[cid][label].append(rest)
    return out


def _in_setting(setting):
    return C.patched(C.Recorder(setting.get("built", False), setting.get("supported", True)),
                     setting)


def test_plan_fields_equal_recorded_launches(calls):
    seen = collections.Counter()
    for cid, by_label in calls.items():
        setting, kind, (M, N, K) = _parse(cid)
        if kind == "fwd" and M <= ops.GEMV_MAX_ROWS:  # the GEMV branch: no plan is made
            assert all(r[0] == "gemv_bf16" for recs in by_label.values() for r in recs[:-1])
            seen["gemv"] += 1
            continue
        with _in_setting(setting):
            chosen = P.plan(kind, M, N, K).splits
            for label, recs in by_label.items():
                if label == "helpers" or recs[0][0] == "raises":
                    continue
                want = WGRAD_SPLITS[label](chosen) if kind == "wgrad" else None
                p = P.plan(kind, M, N, K, want)
                assert (p.kind, p.M, p.N, p.K) == (kind, M, N, K)
                names = [r[0] for r in recs]
                if not p.blas:
                    assert names == ["gemm_bf16"]
                if "blas_gemm" in names:  # the launch took the library (its probe is cached)
                    assert p.blas
                    assert recs[names.index("blas_gemm")][1][-1] == p.blas_algo
                    seen["blas"] += 1
                    continue
                name, args, kw = recs[-1]
                assert name == "gemm_bf16"
                feat = C.FEATURES.get(label, {})
                la = p.launch_args(**feat)
                if la["stages"] in P.DIRECT_STAGES and (feat.get("ct") or feat.get("upd")):
                    la["stages"] = P.RP_STAGED  # gemm(): no register-direct ct / upd
                launched = ((args[BM], args[BN]), args[SPLITS], kw["stages"], kw.get("persist", 0))
                assert (la["tiles"], p.splits, la["stages"], la["persist"]) == launched, \
                    (cid, label)
                assert la["stages"] in P.STAGE_CODES
                seen[kind] += 1
    assert all(seen[k] > 20 for k in ("fwd", "dgrad", "wgrad", "blas")) and seen["xent"] > 10 and seen["gemv"]


def test_sizing_helpers_are_views_of_the_plan(calls):
    for cid, by_label in calls.items():
        setting, kind, (M, N, K) = _parse(cid)
        (_, _, got), = by_label["helpers"]
        with _in_setting(setting):
            try:
                p = P.plan(kind, M, N, K)
            except ValueError:
                assert "ValueError" in got.values()
                continue
            if kind == "wgrad":
                assert got["pick_splits"] == ops.pick_splits(M, N, K) == p.splits
                assert tuple(got["wgrad_config"]) == ops.wgrad_config(M, N, K) == \
                    (*p.tiles, p.splits)
            elif kind == "dgrad":
                assert tuple(got["dgrad_tiles"]) == ops.dgrad_tiles(M, N, K) == p.tiles
                assert tuple(got["dgrad_tiles_noN"]) == ops.dgrad_tiles(M, N) == \
                    ops.pick_tiles(M, N)
            elif kind == "xent":
                assert tuple(got["xent_tiles"]) == ops.xent_tiles(M, N) == p.tiles
            else:
                assert tuple(got["pick_tiles"]) == ops.pick_tiles(M, N)


def test_frag_mask_exactly_when_both_launches_ran_one_direct_tile(calls):
    """Over every recorded forward [M][N] and every recorded dgrad that produces an [M][N]
    gradient under the same switches: a fragment mask exists exactly when the two launches ran
    the same tile with register-direct stage codes (a tile that has the layout, whole row
    tiles, neither product planned for the library path)."""
    ran = collections.defaultdict(dict)  # (setting, M, N) -> {(kind, K): launch or None}
    for cid, by_label in calls.items():
        setting, kind, (M, N, K) = _parse(cid)
        recs = by_label.get("plain" if kind == "fwd" else "wt+cs")
        if kind in ("fwd", "dgrad") and recs and M > ops.GEMV_MAX_ROWS:
            name, args, kw = recs[-1]
            ran[(setting["id"], M, N)][(kind, K)] = \
                ((args[BM], args[BN]), kw["stages"]) if name == "gemm_bf16" else None
    pairs = collections.Counter()
    for (sid, M, N), launches in ran.items():
        for (_, K), f in ((k, v) for k, v in launches.items() if k[0] == "fwd"):
            for (_, N_next), d in ((k, v) for k, v in launches.items() if k[0] == "dgrad"):
                want = None
                with _in_setting(SETTINGS[sid]):
                    library = P.plan("fwd", M, N, K).blas or P.plan("dgrad", M, N, N_next).blas
                    if f and d and f[0] == d[0] and f[1] in P.DIRECT_STAGES and \
                            d[1] in P.DIRECT_STAGES and f[0] in P.FRAG_WAVES and \
                            M % f[0][0] == 0 and not library:
                        want = f[0]
                    assert ops.frag_mask_tiles(M, N, K, N_next) == want, (sid, M, N, K, N_next)
                pairs[want is not None] += 1
    assert pairs[True] >= 3 and pairs[False] >= 10


def test_library_warning_is_issued_once(monkeypatch):
    monkeypatch.setattr(P, "_BLAS_WARNED", [])
    with C.patched(C.Recorder(False, True), {"env": {"DNN_BLAS": "1"}}):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            assert not P.plan("fwd", 4096, 1024, 1024).blas
            assert not P.plan("wgrad", 1024, 1024, 4096).blas
    assert len(w) == 1 and "comparison build" in str(w[0].message)


# ---- the switch parser: one per switch for the all-kinds form, the per-kind form and the
# unknown kind ---------------------------------------------------------------------------------

def test_stages_switch():
    parse = lambda spec: P.parse_kinds("DNN_GEMM_STAGES", spec, P.KINDS, 0)  # noqa: E731
    assert parse("") == {"fwd": 0, "dgrad": 0, "wgrad": 0, "xent": 0}
    assert parse(" 3 ") == {"fwd": 3, "dgrad": 3, "wgrad": 3, "xent": 3}
    assert parse("fwd=9, dgrad=2") == {"fwd": 9, "dgrad": 2, "wgrad": 0, "xent": 0}
    with pytest.raises(ValueError, match="DNN_GEMM_STAGES: unknown GEMM kind"):
        parse("fwd=3,bwd=2")
    assert P.STAGES.keys() == parse("").keys()


def test_persist_switch():
    parse = lambda spec: P.parse_kinds("DNN_GEMM_PERSIST", spec, P.KINDS[:3], None)  # noqa: E731
    assert parse("") == {"fwd": None, "dgrad": None, "wgrad": None}
    assert parse("1") == {"fwd": 1, "dgrad": 1, "wgrad": 1}
    assert parse("fwd=300,wgrad=0") == {"fwd": 300, "dgrad": None, "wgrad": 0}
    with pytest.raises(ValueError, match="DNN_GEMM_PERSIST: unknown GEMM kind"):
        parse("xent=1")  # the fused cross-entropy GEMM has no persistent form
    assert P.PERSIST.keys() == parse("").keys()


def test_persist_argument(monkeypatch):
    for kind in P.PERSIST:
        monkeypatch.setitem(P.PERSIST, kind, None)
    assert P._persist("fwd", None) == 0 and P._persist("fwd", {"persist": 1}) == -1
    assert P._persist("dgrad", {"persist": 300}) == 300
    monkeypatch.setitem(P.PERSIST, "fwd", 0)
    assert P._persist("fwd", {"persist": 1}) == 0
    monkeypatch.setitem(P.PERSIST, "fwd", 1)
    assert P._persist("fwd", None) == -1


def test_blas_switch_forms(monkeypatch):
    monkeypatch.setenv("DNN_BLAS", "1")
    assert all(P._blas_requested(k, None) for k in ("fwd", "dgrad", "wgrad"))
    monkeypatch.setenv("DNN_BLAS", "table")
    assert P._blas_requested("fwd", {"blas": 1}) and not P._blas_requested("fwd", None)
    monkeypatch.setenv("DNN_BLAS", "wgrad=1,dgrad=0")
    assert P._blas_requested("wgrad", None) and not P._blas_requested("dgrad", {"blas": 1})
    assert not P._blas_requested("fwd", {"blas": 1})  # per-kind form: the others are off
    monkeypatch.setenv("DNN_BLAS", "wgrad=1,bwd=1")  # an unknown kind is accepted silently
    assert P._blas_requested("wgrad", None) and not P._blas_requested("fwd", None)
