"""fp64 oracle of one optimizer step, shared by the optimizer tests (CPU and GPU).

Every step is checked on its own, from the kernel's OWN stored state of the step before (and,
for the parameter, from the moment buffers the kernel has just stored, which are checked
against their own oracle first), so errors never compound over steps. The hyperparameters
enter as the caller's doubles: rounding one to fp32 moves it by 2^-25 relative, inside the
bounds -- but ``1 - beta`` must then be rounded from the double difference, as torch.optim
takes it; 1 - fp32(beta) is off by 2^-25 / (1 - beta), 1.3e-5 at beta2 = 0.999, and fails. The
Adam update is written as the kernels write it, ``m * bc1 / (sqrt(v * bc2) + eps)`` with
``bc = 1 / (1 - beta^t)``.

Bounds, per element, u = 2^-24: every quantity is a sum of two products of stored fp32
values, each product rounded once (or fused), the sum rounded once: at most 2 u relative to the
sum of the ABSOLUTE values of the terms. With 2x slack for the fp32 roundings of the
coefficients (lr * wd, 1 - lr * wd, the bias corrections, sqrt, the division):
  * p:            |got - want| <= 2^-22 * (|p_old| + |lr * update|)
  * m, v, mom:    |got - want| <= 2^-22 * (sum of the absolute values of their terms)
    where an L2 term is folded into the gradient (g + wd * p) the gradient's own two terms
    count separately, |g| + |wd * p|: their sum is rounded too, and may cancel. In Adam that
    g' is then multiplied on: it carries up to 2^-23 relative to |g| + |wd * p| itself (wd, the
    product, the sum: three roundings), which m's gradient term passes on once and v's, being
    g'^2, twice -- so with L2 those terms are allowed 2^-22 + 2^-23 (m) and 2^-22 + 2^-22 (v).
  * shadow:       bitwise got_p.to(bfloat16).
Adam's parameter does not fit the first bound where p_old is 0 or tiny: lr * update alone takes
six roundings (m * bc1, v * bc2, sqrt, + eps, lr *, /), about 5 u against the 4 u the bound
allows. The CPU reference path (ops/reference.py, the same operations in fp32) exceeds it by up
to 1.08 x on these inputs. There, as tests/test_mlp_tail_gpu.py::_assert_dgrad_fp64 does, the
bound is scaled by 4 x the worst ratio the CPU reference reaches on the SAME inputs, never
below 1 (``adam_p_slack``).
"""
from __future__ import annotations

import torch

from docker_dist_nn_amd import ops

CPU = torch.device("cpu")
U22 = 2.0 ** -22
SENT = 5.0
BIG_N = 2_097_152 + 3076  # past the 2048-block grid cap of sgd_kernel / adam_kernel
SIZES = [4, 1028, BIG_N]


def f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float32))


def new_stats() -> dict:
    return dict(p=0.0, mom=0.0, m=0.0, v=0.0, p_cpu=0.0)


def statline(name: str, stats: dict) -> str:
    return "OPTSTAT " + name + " worst/bound " + " ".join(
        f"{k} {v:.3f}" for k, v in stats.items() if v > 0.0)


def _close(name, got, want, bound, stats, what, slack=1.0):
    """|got - want| <= slack * bound per element; the figure kept in ``stats`` is the worst
    ratio to the bound itself, before the slack."""
    got = got.detach().to(CPU).double().reshape(-1)
    assert not torch.isnan(got).any(), f"{what}: NaN in {name}"
    err = (got - want.reshape(-1)).abs()
    bound = bound.reshape(-1)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    if stats is not None:
        stats[name] = max(stats[name], ratio)
    assert bool((err <= slack * bound).all()), (
        f"{what}: {name} off by {ratio:.2f} x the bound (allowed {slack:.2f} x) at "
        f"{(err > slack * bound).nonzero()[:4].flatten().tolist()}")


def _shadow(shadow, got_p, what):
    if shadow is not None:
        assert torch.equal(shadow.detach().to(CPU).reshape(-1),
                           got_p.detach().to(CPU).reshape(-1).to(torch.bfloat16)), \
            f"{what}: shadow is not bf16(p)"


def check_sgd(old, g, got, *, lr, momentum=0.0, weight_decay=0.0, stats=None, what="sgd"):
    """old / got: dicts p, mom (None without momentum), shadow (got only); torch.optim.SGD
    semantics: g' = g + wd * p; mom = mu * mom + g'; p -= lr * (mom or g')."""
    lr, mu, wd = float(lr), float(momentum), float(weight_decay)
    p0, g = old["p"].to(CPU).double().reshape(-1), g.to(CPU).double().reshape(-1)
    l2 = wd * p0
    if mu:
        m0 = old["mom"].to(CPU).double().reshape(-1)
        _close("mom", got["mom"], mu * m0 + (g + l2), U22 * ((mu * m0).abs() + g.abs() + l2.abs()),
               stats, what)
        upd = got["mom"].detach().to(CPU).double().reshape(-1)
    else:
        upd = g + l2
    _close("p", got["p"], p0 - lr * upd, U22 * (p0.abs() + (lr * upd).abs()), stats, what)
    _shadow(got.get("shadow"), got["p"], what)


def adam_bc(betas, t: int) -> tuple[float, float]:
    return 1.0 / (1.0 - betas[0] ** t), 1.0 / (1.0 - betas[1] ** t)


def check_adam(old, g, got, *, lr, betas, eps, weight_decay, decoupled, t, stats=None,
               what="adam"):
    """old / got: dicts p, m, v (+ shadow). torch.optim.Adam / AdamW semantics at 1-based
    step ``t``."""
    lr, eps, wd = float(lr), float(eps), float(weight_decay)
    b1, b2 = betas
    bc1, bc2 = adam_bc(betas, t)
    p0, m0, v0 = (old[k].to(CPU).double().reshape(-1) for k in ("p", "m", "v"))
    g = g.to(CPU).double().reshape(-1)
    if decoupled:
        pd, gv, gmag = p0 * (1.0 - lr * wd), g, g.abs()
    else:
        pd, gv, gmag = p0, g + wd * p0, g.abs() + (wd * p0).abs()
    l2 = 2.0 ** -23 if (wd and not decoupled) else 0.0  # the rounding of g' = g + wd * p itself
    _close("m", got["m"], b1 * m0 + (1.0 - b1) * gv,
           U22 * (b1 * m0).abs() + (U22 + l2) * (1.0 - b1) * gmag, stats, what)
    _close("v", got["v"], b2 * v0 + (1.0 - b2) * gv * gv,
           U22 * (b2 * v0).abs() + (U22 + 2 * l2) * (1.0 - b2) * gmag * gmag, stats, what)
    def p_oracle(state):  # from the moments that ``state`` itself stores
        m1, v1 = (state[k].detach().to(CPU).double().reshape(-1) for k in ("m", "v"))
        upd = lr * (m1 * bc1) / (torch.sqrt(v1 * bc2) + eps)
        return pd - upd, U22 * (p0.abs() + upd.abs())

    cpu = {k: old[k].detach().to(CPU).clone() for k in ("p", "m", "v")}
    ops.adam_update(cpu["p"], g.float(), cpu["m"], cpu["v"], None, lr=lr, betas=betas, eps=eps,
                    weight_decay=wd, decoupled=decoupled, step=t)
    want, bound = p_oracle(cpu)
    worst = float(((cpu["p"].double().reshape(-1) - want).abs() / bound.clamp_min(1e-300)).max())
    if stats is not None:
        stats["p_cpu"] = max(stats["p_cpu"], worst)
    want, bound = p_oracle(got)
    _close("p", got["p"], want, bound, stats, what, slack=max(1.0, 4.0 * worst))
    _shadow(got.get("shadow"), got["p"], what)


# ---- inputs ---------------------------------------------------------------------------------

def inputs(n: int, seed: int, steps: int = 5) -> dict:
    """fp32 state and ``steps`` gradients. p: zeros, +-1e4 (where lr * update is tiny against
    p) and N(0, 1); g: zeros and N(0, 0.1); v of order eps^2 = 1e-16 and of order 1."""
    gen = torch.Generator().manual_seed(seed)
    i = torch.arange(n)
    p = torch.randn(n, generator=gen)
    p[i % 5 == 1] = 0.0
    p[i % 7 == 2] = 1e4
    p[i % 7 == 3] = -1e4
    gs = []
    for _ in range(steps):
        g = torch.randn(n, generator=gen) * 0.1
        g[torch.rand(n, generator=gen) < 0.25] = 0.0
        gs.append(g)
    v = torch.rand(n, generator=gen)
    v[i % 2 == 0] *= 1e-16
    return dict(p=p, gs=gs, mom=torch.randn(n, generator=gen) * 0.1,
                m=torch.randn(n, generator=gen) * 0.01, v=v)


def guarded(data: torch.Tensor, dev, dtype=None):
    """(buffer, slice): ``data`` as a slice at a 16-byte offset of a larger sentinel-filled
    buffer."""
    dtype = dtype or data.dtype
    off = 16 // torch.empty(0, dtype=dtype).element_size()
    big = torch.full((data.numel() + 2 * off,), SENT, dtype=dtype)
    big[off:off + data.numel()] = data.to(dtype)
    big = big.to(dev)
    return big, big[off:off + data.numel()]


def assert_guards(big, n, what=""):
    off = (big.numel() - n) // 2
    b = big.detach().to(CPU)
    assert bool((b[:off] == SENT).all()) and bool((b[off + n:] == SENT).all()), \
        f"{what}: wrote outside the slice"


def snap(state: dict) -> dict:
    return {k: (t.detach().to(CPU).clone() if t is not None else None) for k, t in state.items()}


# ---- stand-alone kernels --------------------------------------------------------------------

def run_sgd(n, dev, *, momentum, weight_decay, shadow, lr_dev, stats=None, steps=5, seed=0):
    """``steps`` consecutive ops.sgd_update calls on guarded slices, each checked against the
    oracle from the stored state of the step before; the learning rate changes every step."""
    inp = inputs(n, seed or n, steps)
    bufs = {k: guarded(inp[k], dev) for k in ("p", "mom")}
    bufs["shadow"] = guarded(torch.zeros(n), dev, torch.bfloat16) if shadow else (None, None)
    st = {k: v[1] for k, v in bufs.items()}
    lrd = torch.zeros(1, device=dev) if lr_dev else None
    what = f"sgd n={n} mu={momentum} wd={weight_decay} shadow={shadow} lr_dev={lr_dev}"
    for k, g in enumerate(inp["gs"]):
        lr = 0.1 / (k + 1)
        old = snap(st)
        if lr_dev:
            lrd.fill_(lr)
        ops.sgd_update(st["p"], g.to(dev), st["mom"], st["shadow"], lr=-1.0 if lr_dev else lr,
                       momentum=momentum, weight_decay=weight_decay, lr_dev=lrd)
        got = dict(st, mom=st["mom"] if momentum else None)
        check_sgd(old, g, got, lr=lr, momentum=momentum, weight_decay=weight_decay,
                  stats=stats, what=f"{what} step {k + 1}")
        if not momentum:  # a momentum buffer that is not used is not touched
            assert torch.equal(st["mom"].to(CPU), old["mom"])
    for k, (big, _) in bufs.items():
        if big is not None:
            assert_guards(big, n, f"{what} {k}")
    return snap(st)


def run_adam(n, dev, *, weight_decay, decoupled, betas, start, device_step, stats=None,
             steps=5, seed=0, shadow=True):
    """``steps`` consecutive ops.adam_update calls, steps start+1 .. start+steps, with the step
    and learning rate from the host or (``device_step``) from device memory + ops.step_advance.
    Returns the final state for the bitwise comparison of the two paths."""
    inp = inputs(n, seed or n, steps)
    bufs = {k: guarded(inp[k], dev) for k in ("p", "m", "v")}
    bufs["shadow"] = guarded(torch.zeros(n), dev, torch.bfloat16) if shadow else (None, None)
    st = {k: v[1] for k, v in bufs.items()}
    sd = torch.full((1,), start, dtype=torch.int32, device=dev) if device_step else None
    lrd = torch.zeros(1, device=dev) if device_step else None
    what = f"adam n={n} wd={weight_decay} decoupled={decoupled} betas={betas} start={start} " \
           f"dev={device_step}"
    for k, g in enumerate(inp["gs"]):
        t, lr = start + k + 1, 1e-3 * (1 + k % 2)
        old = snap(st)
        if device_step:
            lrd.fill_(lr)
            assert int(sd[0]) == t - 1
        ops.adam_update(st["p"], g.to(dev), st["m"], st["v"], st["shadow"],
                        lr=-1.0 if device_step else lr, betas=betas, eps=1e-8,
                        weight_decay=weight_decay, decoupled=decoupled,
                        step=1 if device_step else t, lr_dev=lrd, step_dev=sd)
        if device_step:
            ops.step_advance(sd)
        check_adam(old, g, st, lr=lr, betas=betas, eps=1e-8, weight_decay=weight_decay,
                   decoupled=decoupled, t=t, stats=stats, what=f"{what} step {t}")
    for k, (big, _) in bufs.items():
        if big is not None:
            assert_guards(big, n, f"{what} {k}")
    return snap(st)
