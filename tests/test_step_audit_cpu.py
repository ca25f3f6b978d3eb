"""The step audit (tests/_step_audit.py) on the CPU path: clean steps pass every check, and each
of a list of wrong steps -- a collected dict corrupted the way a real engine defect would corrupt
it -- is rejected by the check named for it (the pattern of tests/test_wgrad_oracle.py)."""
import copy
import functools

import pytest
import torch

import _step_audit as sa
from docker_dist_nn_amd.engine import OptimConfig, Trainer

MB, NM = 64, 2
ROWS = MB * NM
LRS = (0.05, 0.03)  # the second step runs at another rate than the first
MODELS = {
    # widths that are no multiples of 64; a sigmoid layer with padding columns among them
    "softmax": ([200, 192, 136, 72, 10], ("relu", "sigmoid", "linear", "softmax"), "softmax_ce"),
    "mse": ([200, 136, 72, 10], ("sigmoid", "relu", "linear"), "mse"),
    "bce": ([200, 136, 72, 10], ("relu", "sigmoid", "sigmoid"), "bce"),
}
OPTS = {"softmax": dict(name="sgd", momentum=0.9, weight_decay=1e-3), "mse": dict(name="adamw",
        weight_decay=1e-2), "bce": dict(name="sgd")}


@functools.lru_cache(maxsize=None)
def run(model: str, pp: int):
    """Two audited steps; [(before, after)] and the optimizer configuration."""
    widths, acts, loss = MODELS[model]
    cfg = OptimConfig(lr=LRS[0], **OPTS[model])
    tr = Trainer(sa.spec_of(widths, acts), micro_batch=MB, num_micro=NM, pp=pp, optim=cfg,
                 device=torch.device("cpu"), loss=loss)
    steps = []
    for k, lr in enumerate(LRS):
        x, y, t = sa.batch(ROWS, MB, widths[0], tr.stages[0].x_in.shape[1], widths[-1], 5 + k,
                        loss != "softmax_ce")
        cfg.lr = lr
        before = sa.snapshot(tr)
        tr.set_batch(x, y, targets=t)
        tr.step()
        tr.flush()
        steps.append((before, sa.collect(tr)))
    return steps, cfg


@functools.lru_cache(maxsize=None)
def run_fp8():
    """As run("softmax", 2), the two stages joined by the fp8 hop format."""
    widths, acts, _ = MODELS["softmax"]
    cfg = OptimConfig(lr=LRS[0], **OPTS["softmax"])
    tr = sa.Fp8Pair(sa.spec_of(widths, acts), 2, micro_batch=MB, num_micro=NM, optim=cfg,
                    device=torch.device("cpu"))
    assert all(st.boundary == "fp8" for st in tr.stages)
    steps = []
    for k, lr in enumerate(LRS):
        x, y, _ = sa.batch(ROWS, MB, widths[0], tr.stages[0].x_in.shape[1], widths[-1], 5 + k,
                           False)
        cfg.lr = lr
        before = sa.snapshot(tr)
        tr.set_batch(x, y)
        tr.step()
        steps.append((before, sa.collect(tr)))
    return steps, cfg


@pytest.mark.parametrize("pp", [1, 2])
@pytest.mark.parametrize("model", list(MODELS))
def test_clean_steps_pass(model, pp):
    steps, cfg = run(model, pp)
    stats = sa.new_stats()
    for before, after in steps:
        assert len(after["stages"]) == pp
        sa.audit(before, after, cfg, stats)
    print("\n" + sa.statline(f"cpu {model} pp{pp}", stats))
    assert min(stats["checks"][k] for k in ("F", "L", "B", "G", "W", "O")) > 0  # each ran
    assert stats["H"] == (4 if pp == 2 else 0)  # two hops, two steps


# ---- wrong steps -----------------------------------------------------------------------------

def _second_step(pp=1):
    steps, cfg = run("softmax", pp)
    before, after = copy.deepcopy(steps[1])
    return before, after, cfg


def _zero_dz_block(b, a):
    a["stages"][0]["dz"][1][16:32] = 0


def _acts_read_twice(b, a):
    a["stages"][0]["acts"][0][MB:2 * MB] = a["stages"][0]["acts"][0][:MB]


def _gb_missing_micro_batch(b, a):
    a["stages"][0]["gb"][2] *= (NM - 1) / NM


def _with_wt(b, a):  # the W^T shadows of layer 1, as the GPU path keeps them
    b["stages"][0]["wt"][1] = b["stages"][0]["wbf"][1].t().contiguous()
    a["stages"][0]["wt"][1] = a["stages"][0]["wbf"][1].t().contiguous()


def _stale_wt(b, a):
    _with_wt(b, a)
    a["stages"][0]["wt"][1] = b["stages"][0]["wt"][1].clone()


def _stale_shadow(b, a):
    d = a["stages"][0]
    n = d["geoms"][2]["np_"] * d["geoms"][2]["kp"]
    off = d["w_off"][2]
    d["shadow"][off:off + n] = b["stages"][0]["shadow"][off:off + n]


def _padding_row_gradient(b, a):
    d = a["stages"][-1]
    row = int((d["labels"] < 0).nonzero()[0])
    d["dz"][-1][row, 1] = 2.0 ** -12


def _gw_row_twice(b, a):
    d = a["stages"][0]
    d["gw"][1] += torch.outer(d["dz"][1][5].float(), d["acts"][0][5].float())


def _with_mask(b, a):
    a["stages"][0]["mask_bits"][0] = a["stages"][0]["acts"][0] > 0


def _mask_bit(b, a):
    _with_mask(b, a)
    a["stages"][0]["mask_bits"][0][17, 33] ^= True


def _loss_of_padding_block(b, a):
    d = a["stages"][-1]
    own, n_part = sa._owners(d)
    valid = torch.zeros(n_part).index_add_(0, own, (d["labels"] >= 0).float())
    empty = (valid == 0).nonzero()
    assert empty.numel(), "the batch has no all-padding loss partial"
    d["loss_part"][int(empty[0])] = 1e-3


def _previous_lr(b, a):
    d, o = a["stages"][0], b["stages"][0]
    d["master"] = o["master"] - LRS[0] * d["state"][0]  # momentum SGD: p -= lr * mom
    d["shadow"] = d["master"].to(torch.bfloat16)


MUTATIONS = [("B", _zero_dz_block), ("F", _acts_read_twice), ("G", _gb_missing_micro_batch),
             ("T", _stale_wt), ("O", _stale_shadow), ("L", _padding_row_gradient),
             ("W", _gw_row_twice), ("M", _mask_bit), ("L", _loss_of_padding_block),
             ("O", _previous_lr)]


@pytest.mark.parametrize("kind,mutate", MUTATIONS, ids=[m.__name__.strip("_") for _, m in MUTATIONS])
def test_wrong_step_is_rejected(kind, mutate):
    before, after, cfg = _second_step()
    mutate(before, after)
    with pytest.raises(AssertionError, match=rf"^\[{kind}\] stage \d"):
        sa.audit(before, after, cfg)


@pytest.mark.parametrize("prepare", [_with_wt, _with_mask])
def test_synthetic_parts_pass_unmutated(prepare):
    """The W^T shadows and masks the mutations above add are right until they are corrupted."""
    before, after, cfg = _second_step()
    prepare(before, after)
    sa.audit(before, after, cfg)


def test_wrong_hop_is_rejected():
    before, after, cfg = _second_step(pp=2)
    sa.audit(before, after, cfg)
    after["stages"][1]["x_in"][MB + 1, 2] += 1.0
    with pytest.raises(AssertionError, match=r"^\[H\] stage 0"):
        sa.audit(before, after, cfg)


def test_fp8_boundary_steps_pass_and_wrong_hops_are_rejected():
    steps, cfg = run_fp8()
    stats = sa.new_stats()
    for before, after in steps:
        assert after["stages"][0]["fp8"] and after["stages"][1]["fp8"]
        sa.audit(before, after, cfg, stats)
    print("\n" + sa.statline("cpu softmax fp8 pp2", stats))
    assert stats["H"] == 12  # codes, scales and received rows of two hops, two steps
    for stage, key in ((1, "x_in"), (0, "dz")):  # a received row that is not the sent one
        before, after = copy.deepcopy(steps[1])
        t = after["stages"][stage][key]
        t = t[-1] if key == "dz" else t
        row = int(t.float().abs().sum(1).argmax())
        t[row] = t[row] * 2
        with pytest.raises(AssertionError, match=r"^\[H\] stage 0: fp8"):
            sa.audit(before, after, cfg)
    before, after = copy.deepcopy(steps[1])
    after["stages"][1]["fp8"]["s_in"][5] *= 2  # the scale of another row
    with pytest.raises(AssertionError, match=r"^\[H\] stage 0: fp8 activation scales"):
        sa.audit(before, after, cfg)


def test_sigmoid_padding_units_stay_off():
    """Regression: the padding units of a sigmoid layer whose width is no multiple of 64 used to
    output sigmoid(0) = 0.5, so the next layer's padded weight columns received a gradient and
    left 0 -- the padded model drifted from the specified one. They are held at exactly 0."""
    steps, _ = run("softmax", 1)
    for _, after in steps:
        d = after["stages"][0]
        assert d["geoms"][1]["act"] == "sigmoid" and d["geoms"][1]["out_dim"] == 136
        assert bool((d["acts"][1][:, 136:] == 0).all())
        for i, g in enumerate(d["geoms"]):
            assert bool((d["w32"][i][:, g["in_dim"]:] == 0).all()), i
            assert bool((d["w32"][i][g["out_dim"]:] == 0).all()), i
            assert bool((d["gw"][i][:, g["in_dim"]:] == 0).all()), i
        from docker_dist_nn_amd.engine.params import PAD_OFF_BIAS

        assert OPTS["softmax"]["weight_decay"] > 0  # the decay does not move the pinned bias
        assert bool((d["b32"][1][136:] == PAD_OFF_BIAS).all())


@pytest.mark.parametrize("opt", sa.DECAY_OPTS, ids=sa.DECAY_IDS)
def test_padding_units_stay_off_under_weight_decay(opt):
    """lr * weight_decay = 0.5 halves every decayed parameter per step: a bias that was only
    initialised to PAD_OFF_BIAS = -2^50 would be above the sigmoid's underflow threshold after
    50 steps and the padding units back on. They are pinned after every update: after 64 steps
    the padding bias is still bitwise PAD_OFF_BIAS, the padding units output exactly 0 and the
    next layer's padded weight columns are exactly 0."""
    sa.check_padding_pinned(torch.device("cpu"), opt)
