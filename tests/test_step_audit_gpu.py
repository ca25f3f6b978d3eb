"""Whole training steps on the GPU, audited stage by stage against fp64 (tests/_step_audit.py),
under every engine path: heads, hidden activations, pipelines, executors, backward forms, update
forms and stream plans. Each case builds a Trainer, asserts that the switch under test took
effect, and audits consecutive steps (the later ones start from updated shadows, W^T and optimizer
state, at another learning rate). One STEPSTAT line per case: worst error / bound of each check."""
import time
from dataclasses import dataclass, field
from typing import Callable, Optional

import pytest
import torch

import _step_audit as sa
from docker_dist_nn_amd.engine import OptimConfig, Trainer
from docker_dist_nn_amd.engine.loss_head import DenseHead, FusedXentHead, TailHead, XentHead

pytestmark = pytest.mark.gpu

LRS = (0.05, 0.03, 0.04)  # every step at another rate than the one before
RELU = ("relu", "relu", "relu", "softmax")
MIX = ("sigmoid", "linear", "relu", "softmax")
BASE = [200, 328, 136, 72, 10]        # no hidden width a multiple of 64; fused-xent head
TAIL = [200, 328, 250, 120, 10]       # ...-256-128-64 padded: the classifier tail's geometry
ONE_SPLIT = [200, 1000, 512, 10]      # layer 1 ([512][1024] at 384 rows): one wgrad split
ONE_SPLIT_1024 = [200, 512, 2048, 10] # layer 1 ([2048][512]): one split at 1024 rows
FRAG = [512, 256, 128, 10]            # fragment-order mask of layer 0 at 65536 rows
FRAG_WIDE = [784, 1024, 1024, 10]     # ... and of a 1024-wide layer (DNN_RELU_MASK=auto)
MOM = dict(name="sgd", momentum=0.9, weight_decay=1e-3)


@dataclass
class Case:
    id: str
    widths: list = field(default_factory=lambda: BASE)
    acts: tuple = RELU
    loss: str = "softmax_ce"
    env: dict = field(default_factory=dict)
    kw: dict = field(default_factory=dict)       # Trainer arguments
    opt: dict = field(default_factory=lambda: dict(name="sgd"))
    mb: int = 128
    nm: int = 3
    steps: int = 2
    capture: bool = False
    big: bool = False                            # oracle products on the GPU (torch fp64)
    fp8: bool = False                            # two stages joined by the fp8 hop format
    expect: Optional[Callable] = None            # asserts the switch took effect


def _last(tr):
    return tr.stages[-1]


def _head(cls, **attrs):
    def check(tr):
        assert type(_last(tr).head) is cls, type(_last(tr).head)
        for k, v in attrs.items():
            assert getattr(_last(tr).head, k) == v, (k, getattr(_last(tr).head, k))
    return check


def _all(*checks):
    def check(tr):
        for c in checks:
            c(tr)
    return check


def _pipeline(pp, schedule):
    def check(tr):
        assert len(tr.stages) == pp and tr.schedule == schedule
        assert all(st.wgrad_mode == ("per_micro" if schedule == "zb" else "batched")
                   for st in tr.stages)
        # per-micro-batch weight gradients run on the Python executor
        assert (tr.executor._native_plan() is not None) == (schedule != "zb")
    return check


def _fp8(native):
    def check(tr):
        a, b = tr.stages
        assert a.boundary == b.boundary == "fp8" and a._fp8_next and b._fp8_prev
        assert all((st._prog is not None) == native for st in tr.stages)
        if native:
            assert "QF0" in a._prog.segments() and "DQF0" in b._prog.segments()
    return check


def _native(on, plan=True):
    def check(tr):
        assert tr.native_exec == on
        assert all((st._prog is not None) == on for st in tr.stages)
        assert (tr.executor._native_plan() is not None) == (on and plan)
    return check


def _masks(kind, layers):
    def check(tr):
        got = [None if m is None else type(m).__name__ for m in tr.stages[0].relu_mask]
        want = [kind if i in layers else None for i in range(len(got))]
        assert got == want, (got, want)
    return check


def _kk(tr):
    st = tr.stages[0]
    assert sorted(st.dzT) == [1, 2] and sorted(st.actT) == [0, 1], (list(st.dzT), list(st.actT))


def _wt(on):
    def check(tr):
        st = tr.stages[0]
        assert sorted(st.params.wt) == ([1, 2, 3] if on else []), list(st.params.wt)
    return check


def _per_micro(tr):
    assert tr.stages[0].wgrad_mode == "per_micro" and tr.executor._native_plan() is None


def _fused_layer(tr):
    """The overlap plan with a layer that updates in its wgrad epilogue: that wgrad is forked
    only after the dgrad that reads the layer's old W^T."""
    assert sorted(tr.stages[0].params.fused_layers) == [1]
    segs = [seg for _, seg, _ in tr.executor._native_plan()]
    assert segs.index("B0.L1") < segs.index("W1") and "@fork" in segs[segs.index("B0.L1"):], segs


def _group(on):
    """All four weight gradients of BASE at 384 rows plan the 64x64 tile with 4 / 4 / 6 / 6
    splits: one grouped launch by default, one launch per layer with DNN_WGRAD_GROUP=0."""
    def check(tr):
        st = tr.stages[0]
        launches = st._prog.segment_size("W")
        if on:
            assert launches < len(st.geoms), launches
        else:
            assert launches == len(st.geoms), launches
    return check


def _streamk(tr):
    st = tr.stages[0]
    assert st.wgrad_algo == "streamk" and st.slabs == [] and not st.fused_fin_sgd_ok()


def _segments(*names, absent=()):
    def check(tr):
        segs = tr.stages[0]._prog.segments()
        assert all(n in segs for n in names), (names, sorted(segs))
        assert not any(n in segs for n in absent), (absent, sorted(segs))
        plan = [seg for _, seg, _ in tr.executor._native_plan()]
        if "FINO" in names:
            assert "FINO" in plan and "O" not in plan, plan
        if "FINO" in absent:
            assert "FIN" in plan and "O" in plan, plan
    return check


def _fin_wt(on):
    def check(tr):
        st = tr.stages[0]
        assert st._wt_by_update_layers() == [1, 2, 3]
        # with DNN_FIN_WT the update launch writes W^T itself: no transpose launch behind it
        assert st._prog.segment_size("FINO") == st._prog.segment_size("FIN") + (0 if on else 1)
    return check


def _fused_update(on):
    def check(tr):
        st = tr.stages[0]
        assert [s == 1 for s in st.w_splits] == [False, True, False], st.w_splits
        assert sorted(st.params.fused_layers) == ([1] if on else [])
    return check


def _plan(fork, split=None, xstep=None, h0=None, mode5=False):
    def check(tr):
        st = tr.stages[0]
        plan = tr.executor._native_plan()
        segs = [seg for _, seg, _ in plan]
        assert ("@fork" in segs) == fork, segs
        if split is not None:
            assert ("FINO0-0" in segs) == split, segs
        if mode5:  # W1 and W0 on the main stream, the small wgrads on the side
            assert [e[2] for e in plan if e[1] in ("W0", "W1")] == [0, 0], plan
            assert all(e[2] == 1 for e in plan if e[1] in ("W2", "W3")), plan
        if h0 is not None:
            assert st.h0_double == h0
    return check


C = Case
CASES = [
    # ---- heads
    C("head-tail", TAIL, env={"DNN_TAIL": "1"}, expect=_head(TailHead, fwd_from=2, dgrad_from=2)),
    C("head-tail-sigmoid-out", TAIL, ("relu", "linear", "sigmoid", "softmax"),
      env={"DNN_TAIL": "1"}, opt=MOM, expect=_head(TailHead)),
    C("head-tail-sigmoid-in", TAIL, ("relu", "sigmoid", "linear", "softmax"),
      env={"DNN_TAIL": "1"}, expect=_head(TailHead)),
    C("head-fused-xent", TAIL, env={"DNN_TAIL": "0"},
      expect=_head(FusedXentHead, fwd_from=3, dgrad_from=4)),
    C("head-xent", TAIL, env={"DNN_TAIL": "0", "DNN_FUSED_XENT": "0"}, expect=_head(XentHead)),
    C("head-wide-300", [200, 136, 72, 300], ("relu", "relu", "softmax"), expect=_head(XentHead)),
    C("head-mse-linear", BASE, ("relu", "sigmoid", "relu", "linear"), "mse",
      expect=_head(DenseHead, chunks=1)),
    C("head-mse-relu", BASE, ("relu", "relu", "linear", "relu"), "mse", expect=_head(DenseHead)),
    C("head-mse-sigmoid", BASE, ("relu", "relu", "relu", "sigmoid"), "mse",
      expect=_head(DenseHead)),
    C("head-bce-300", [200, 136, 72, 300], ("relu", "sigmoid", "sigmoid"), "bce",
      opt=dict(name="adam"), expect=_head(DenseHead, chunks=2)),
    # ---- hidden activations
    C("hidden-relu", expect=_head(FusedXentHead)),
    C("hidden-mixed", acts=MIX, opt=MOM, expect=_head(FusedXentHead)),
    # ---- pipelines (loopback: every stage in this process)
    *[C(f"pp{pp}-{sch}", acts=MIX, kw=dict(pp=pp, schedule=sch), expect=_pipeline(pp, sch))
      for pp in (2, 3) for sch in ("1f1b", "gpipe", "zb")],
    C("pp2-streams0", kw=dict(pp=2), env={"DNN_LOOPBACK_STREAMS": "0"}, opt=MOM,
      expect=_pipeline(2, "1f1b")),
    C("pp2-streams1", kw=dict(pp=2), env={"DNN_LOOPBACK_STREAMS": "1"}, opt=MOM,
      expect=_pipeline(2, "1f1b")),
    C("pp2-fp8", acts=MIX, fp8=True, opt=MOM, kw=dict(native=False), expect=_fp8(False)),
    C("pp2-fp8-native", acts=MIX, fp8=True, opt=MOM, kw=dict(native=True), expect=_fp8(True)),
    # ---- executors
    C("exec-python", env={"DNN_NATIVE_EXEC": "0"}, opt=MOM, expect=_native(False)),
    C("exec-native", env={"DNN_NATIVE_EXEC": "1"}, opt=MOM, expect=_native(True)),
    C("exec-per-op-replay", env={"DNN_NATIVE_PLAN": "0"}, opt=MOM,
      expect=_native(True, plan=False)),
    C("exec-graph", acts=MIX, opt=dict(name="adam", weight_decay=1e-2), capture=True,
      expect=_native(True)),
    C("exec-graph-pp2", kw=dict(pp=2), opt=MOM, capture=True, expect=_native(True)),
    # ---- backward forms
    C("mask-0", env={"DNN_RELU_MASK": "0", "DNN_TAIL": "0"}, expect=_masks(None, ())),
    C("mask-1", env={"DNN_RELU_MASK": "1", "DNN_TAIL": "0"}, expect=_masks("Tensor", (0, 1, 2))),
    # (the stage allocates a mask for layer 2 as well; the tail kernel, which runs that layer's
    # forward and its consumer, neither writes nor reads it, and the audit does not look at it)
    C("mask-1-tail", TAIL, env={"DNN_RELU_MASK": "1"},
      expect=_all(_head(TailHead), _masks("Tensor", (0, 1, 2)))),
    C("mask-2-frag", FRAG, RELU[1:], env={"DNN_RELU_MASK": "2", "DNN_TAIL": "0"}, mb=65536, nm=1,
      big=True, expect=_masks("FragMask", (0,))),
    C("mask-auto-small", [200, 1024, 136, 10], RELU[1:], env={"DNN_RELU_MASK": "auto"},
      expect=_masks(None, ())),  # no register-direct tile at 128 rows: the activation is read
    # one audited step: 65536 rows (the fewest with a fragment tile) x 1024 columns cost 3-4 s
    # of comparisons per step; a second step from updated state under a fragment mask is what
    # mask-2-frag audits
    C("mask-auto-frag-1024", FRAG_WIDE, RELU[1:], env={"DNN_RELU_MASK": "auto"}, mb=65536, nm=1,
      steps=1, big=True, expect=_masks("FragMask", (0,))),
    C("wgrad-kk", env={"DNN_WGRAD_KK": "1", "DNN_TAIL": "0"}, expect=_kk),
    C("dgrad-wt-0", env={"DNN_DGRAD_WT": "0"}, opt=MOM, expect=_wt(False)),
    C("dgrad-wt-1", env={"DNN_DGRAD_WT": "1"}, opt=MOM, expect=_wt(True)),
    C("wgrad-streamk", env={"DNN_WGRAD_ALGO": "streamk"}, opt=MOM, expect=_streamk),
    C("wgrad-per-micro", kw=dict(wgrad="per_micro"), expect=_per_micro),
    C("wgrad-group-0", env={"DNN_WGRAD_GROUP": "0"}, expect=_group(False)),
    C("wgrad-group-1", env={"DNN_WGRAD_GROUP": "1"}, expect=_group(True)),
    # ---- updates
    C("opt-sgd", acts=MIX, opt=dict(name="sgd"), expect=_segments("FINO", "FINO1-3")),
    C("opt-sgd-momentum-wd", acts=MIX, opt=MOM, expect=_segments("FINO")),
    C("opt-adam", acts=MIX, opt=dict(name="adam", weight_decay=1e-3),
      expect=_segments("FINO", absent=("FINO1-3",))),
    C("opt-adamw", acts=MIX, opt=dict(name="adamw", weight_decay=1e-2), expect=_segments("FINO")),
    C("fuse-fin-sgd-0", env={"DNN_FUSE_FIN_SGD": "0"}, opt=MOM, expect=_segments(absent=("FINO",))),
    C("fuse-fin-sgd-0-adam", env={"DNN_FUSE_FIN_SGD": "0"}, opt=dict(name="adam"),
      expect=_segments(absent=("FINO",))),
    C("fin-wt-0", env={"DNN_FIN_WT": "0"}, opt=MOM, expect=_fin_wt(False)),
    C("fin-wt-1", env={"DNN_FIN_WT": "1"}, opt=MOM, expect=_fin_wt(True)),
    C("fused-update-1", ONE_SPLIT, RELU[1:], env={"DNN_WGRAD_FUSED_UPDATE": "1"}, opt=MOM,
      expect=_fused_update(True)),
    C("fused-update-1-plain", ONE_SPLIT, RELU[1:], env={"DNN_WGRAD_FUSED_UPDATE": "1"},
      expect=_fused_update(True)),
    C("fused-update-0", ONE_SPLIT, RELU[1:], env={"DNN_WGRAD_FUSED_UPDATE": "0"}, opt=MOM,
      expect=_fused_update(False)),
    # ---- stream plans: one micro-batch of 1024 rows, three consecutive steps
    *[C(f"overlap-{m}-split{sf}", mb=1024, nm=1, steps=3, opt=MOM,
        env={"DNN_BW_OVERLAP_MIN_ROWS": "0", "DNN_BW_OVERLAP": m, "DNN_SPLIT_FINO": sf,
             "DNN_TAIL": "0"},
        expect=_plan(fork=m != "0", split=(sf == "1" and m != "0"), mode5=m == "5"))
      for m in ("0", "1", "5") for sf in ("0", "1")],
    *[C(f"xstep{xs}-h0double{h0}", acts=MIX, opt=MOM, mb=1024, nm=1, steps=3,
        env={"DNN_BW_OVERLAP_MIN_ROWS": "0", "DNN_SPLIT_FINO": "1", "DNN_XSTEP": xs,
             "DNN_H0_DOUBLE": h0},
        expect=_plan(fork=True, split=True, h0=h0 == "1"))
      for xs in ("0", "1") for h0 in ("0", "1")],
    C("overlap-fused-update", ONE_SPLIT_1024, RELU[1:], mb=1024, nm=1, steps=3, opt=MOM,
      env={"DNN_BW_OVERLAP_MIN_ROWS": "0"}, expect=_fused_layer),
]

_T0 = [None, 0.0]


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    _T0[0] = time.time()
    yield
    print(f"\nSTEPSTAT file wall time {time.time() - _T0[0]:.1f} s, in audits {_T0[1]:.1f} s")


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_step_audit(dev, monkeypatch, case):
    try:
        _audit_case(dev, monkeypatch, case)
    except RuntimeError as e:  # a faulted device serves no further case: end the session
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"GPU fault in {case.id}: {e}", returncode=3)
        raise


def _audit_case(dev, monkeypatch, case):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    cfg = OptimConfig(lr=LRS[0], **case.opt)
    if case.fp8:
        tr = sa.Fp8Pair(sa.spec_of(case.widths, case.acts), 2, micro_batch=case.mb,
                        num_micro=case.nm, optim=cfg, device=dev, **case.kw)
    else:
        tr = Trainer(sa.spec_of(case.widths, case.acts), micro_batch=case.mb,
                     num_micro=case.nm, optim=cfg, device=dev, loss=case.loss, **case.kw)
    case.expect(tr)
    rows, dense = case.mb * case.nm, case.loss != "softmax_ce"
    kp = tr.stages[0].x_in.shape[1]

    def load(seed):
        x, y, t = sa.batch(rows, case.mb, case.widths[0], kp, case.widths[-1], seed, dense)
        tr.set_batch(x.to(dev), y.to(dev), targets=None if t is None else t.to(dev))

    if case.capture:
        load(3)
        tr.capture()
        assert tr.graph_nodes > 0
    stats = sa.new_stats()
    for k in range(case.steps):
        cfg.lr = LRS[k]
        tr.flush()
        torch.cuda.synchronize(dev)
        before = sa.snapshot(tr)
        load(5 + k)
        tr.step()
        tr.flush()
        torch.cuda.synchronize(dev)
        after = sa.collect(tr)
        t0 = time.time()
        sa.audit(before, after, cfg, stats, oracle_device=dev if case.big else None)
        _T0[1] += time.time() - t0
    if "DNN_XSTEP" in case.env:  # the cross-step form ran (it needs a primed side stream)
        assert getattr(tr.executor, "_xprimed", False) == (case.env["DNN_XSTEP"] == "1")
    if len(tr.stages) > 1 and not case.fp8 and tr.executor._native_plan() is not None \
            and not case.capture:
        streams = case.env.get("DNN_LOOPBACK_STREAMS", "1") == "1"
        assert (getattr(tr.executor, "_lb_plan", None) is not None) == streams
    print("\n" + sa.statline(case.id, stats))
    assert all(stats["checks"][k] > 0 for k in ("F", "L", "B", "G", "W", "O")), stats
    assert (stats["M"] > 0) == any(m is not None for st in tr.stages
                                   for m in st.relu_mask[:st.fwd_from])
    assert (stats["T"] > 0) == any(bool(st.actT or st.dzT or st.params.wt) for st in tr.stages)
    assert (stats["H"] > 0) == (len(tr.stages) > 1)


@pytest.mark.parametrize("opt", sa.DECAY_OPTS, ids=sa.DECAY_IDS)
def test_padding_units_stay_off_under_weight_decay(dev, opt):
    """As the CPU test of this name: 64 steps at lr * weight_decay = 0.5, on the recorded
    update segments (the pins follow every update inside them)."""
    sa.check_padding_pinned(dev, opt)
