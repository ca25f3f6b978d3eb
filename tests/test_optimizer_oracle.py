"""The fp64 optimizer oracle (tests/_opt_oracle.py) checked without a GPU: the CPU path of
ops.sgd_update / ops.adam_update (ops/reference.py) through the same per-step checks the GPU
tests use, and a set of deliberately wrong optimizers it must reject."""
import pytest
import torch

import _opt_oracle as oo

CPU = torch.device("cpu")
ADAM_VARIANTS = [((0.9, 0.999), 0), ((0.8, 0.99), 0), ((0.9, 0.999), 999)]  # (betas, start)


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_sgd_cases_on_cpu_path(momentum, weight_decay):
    stats = oo.new_stats()
    for n in oo.SIZES:
        for shadow, lr_dev in ((True, True), (False, False), (True, False), (False, True)):
            if n == oo.BIG_N and shadow != lr_dev:
                continue
            oo.run_sgd(n, CPU, momentum=momentum, weight_decay=weight_decay, shadow=shadow,
                       lr_dev=lr_dev, stats=stats)
    print("\n" + oo.statline(f"cpu sgd mu={momentum} wd={weight_decay}", stats))


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_adam_cases_on_cpu_path(weight_decay, decoupled):
    stats = oo.new_stats()
    for n in oo.SIZES:
        for betas, start in ADAM_VARIANTS[:1] if n == oo.BIG_N else ADAM_VARIANTS:
            res = [oo.run_adam(n, CPU, weight_decay=weight_decay, decoupled=decoupled,
                               betas=betas, start=start, device_step=ds, stats=stats)
                   for ds in (False, True)]
            for k in ("p", "m", "v", "shadow"):  # host step == device step, bit for bit
                assert torch.equal(res[0][k], res[1][k]), k
    print("\n" + oo.statline(f"cpu adam wd={weight_decay} decoupled={decoupled}", stats))


# ---- the mistakes the oracle is for ---------------------------------------------------------

def _adam(old, g, *, lr, betas, eps, wd, decoupled, t, as_l2=False, t_off=0, eps_inside=False,
          stale_shadow=False, f32_beta=False):
    """Plain fp32 torch Adam / AdamW; each flag is one wrong implementation."""
    b1, b2 = betas
    p, m, v = old["p"].clone(), old["m"].clone(), old["v"].clone()
    gv = g.clone()
    if decoupled and not as_l2:
        p *= 1.0 - lr * wd
    elif wd:
        gv += wd * p
    omb1, omb2 = ((1.0 - oo.f32(b1)), (1.0 - oo.f32(b2))) if f32_beta else (1.0 - b1, 1.0 - b2)
    m = b1 * m + omb1 * gv
    v = b2 * v + omb2 * gv * gv
    bc1, bc2 = oo.adam_bc(betas, t + t_off)
    den = torch.sqrt(v * bc2 + eps) if eps_inside else torch.sqrt(v * bc2) + eps
    p -= lr * (m * bc1) / den
    return dict(p=p, m=m, v=v, shadow=(old["p"] if stale_shadow else p).to(torch.bfloat16))


def _sgd(old, g, *, lr, mu, wd, late_momentum=False, stale_shadow=False):
    p, mom = old["p"].clone(), old["mom"].clone()
    gv = g + wd * p
    new_mom = mu * mom + gv
    p -= lr * (mom if late_momentum else new_mom)
    return dict(p=p, mom=new_mom, shadow=(old["p"] if stale_shadow else p).to(torch.bfloat16))


def test_oracle_catches_the_mistakes_it_is_for():
    inp = oo.inputs(1028, seed=11)
    g = inp["gs"][0]
    old = dict(p=inp["p"], m=inp["m"], v=inp["v"], mom=inp["mom"])
    for t in (1, 3):
        cfg = dict(lr=1e-3, betas=(0.8, 0.99), eps=1e-8, wd=1e-2, decoupled=True, t=t)
        chk = dict(lr=1e-3, betas=(0.8, 0.99), eps=1e-8, weight_decay=1e-2, decoupled=True, t=t)
        oo.check_adam(old, g, _adam(old, g, **cfg), **chk)
        for mut in (dict(as_l2=True), dict(t_off=1), dict(eps_inside=True),
                    dict(stale_shadow=True), dict(f32_beta=True)):
            with pytest.raises(AssertionError):
                oo.check_adam(old, g, _adam(old, g, **cfg, **mut), **chk)
    cfg = dict(lr=0.1, mu=0.9, wd=1e-2)
    chk = dict(lr=0.1, momentum=0.9, weight_decay=1e-2)
    oo.check_sgd(old, g, _sgd(old, g, **cfg), **chk)
    for mut in (dict(late_momentum=True), dict(stale_shadow=True)):
        with pytest.raises(AssertionError):
            oo.check_sgd(old, g, _sgd(old, g, **cfg, **mut), **chk)
    # a decoupled decay of the wrong sign
    cfg = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, decoupled=True, t=2)
    with pytest.raises(AssertionError):
        oo.check_adam(old, g, _adam(old, g, wd=-1e-2, **cfg), weight_decay=1e-2, **cfg)
