"""sgd4 / adam4 in the three places they run -- ops.sgd_update / ops.adam_update (including the
grid-stride loop on the capped grid), fused into ops.reduce_multi, and sgd4 in the weight-gradient
GEMM epilogue (``upd=`` of ops.linear_wgrad) -- each step against the fp64 oracle of
tests/_opt_oracle.py, on slices of sentinel-filled buffers."""
import pytest
import torch

import _act_oracle as ao
import _opt_oracle as oo
from docker_dist_nn_amd import ops

pytestmark = pytest.mark.gpu
CPU = torch.device("cpu")
ADAM_VARIANTS = [((0.9, 0.999), 0), ((0.8, 0.99), 0), ((0.9, 0.999), 999)]  # (betas, start)


@pytest.mark.parametrize("n", oo.SIZES)
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_sgd_update_fp64(dev, n, momentum, weight_decay):
    stats = oo.new_stats()
    for shadow, lr_dev in ((True, True), (False, False), (True, False), (False, True)):
        if n == oo.BIG_N and shadow != lr_dev:
            continue
        oo.run_sgd(n, dev, momentum=momentum, weight_decay=weight_decay, shadow=shadow,
                   lr_dev=lr_dev, stats=stats)
    print("\n" + oo.statline(f"gpu sgd n={n} mu={momentum} wd={weight_decay}", stats))


@pytest.mark.parametrize("n", oo.SIZES)
@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_adam_update_fp64(dev, n, weight_decay, decoupled):
    """Steps 1..5 and 1000..1004, default and non-default betas; the host-step and the
    device-step (step_dev + ops.step_advance, lr_dev) paths must agree bit for bit."""
    stats = oo.new_stats()
    for betas, start in ADAM_VARIANTS[1:2] if n == oo.BIG_N else ADAM_VARIANTS:
        res = [oo.run_adam(n, dev, weight_decay=weight_decay, decoupled=decoupled, betas=betas,
                           start=start, device_step=ds, stats=stats) for ds in (False, True)]
        for k in ("p", "m", "v", "shadow"):
            assert torch.equal(res[0][k], res[1][k]), (k, betas, start)
    print("\n" + oo.statline(f"gpu adam n={n} wd={weight_decay} decoupled={decoupled}", stats))


# ---- fused into reduce_multi ----------------------------------------------------------------

W_ROWS, W_COLS, GAP, N2 = 96, 64, 64, 1028  # job 1 = a [96][64] weight (with W^T), job 2 flat


@pytest.mark.parametrize("max_blocks", [0, 3])
@pytest.mark.parametrize("opt", [dict(momentum=0.0, weight_decay=0.0),
                                 dict(momentum=0.9, weight_decay=1e-2),
                                 dict(adam=True, weight_decay=0.0, decoupled=False),
                                 dict(adam=True, weight_decay=1e-2, decoupled=False),
                                 dict(adam=True, weight_decay=1e-2, decoupled=True)])
def test_reduce_multi_fused_update_fp64(dev, opt, max_blocks):
    """Two jobs in one flat gradient with a gap no job covers, one job with a W^T output: the
    reduced gradient against the fp64 sum of the slabs, the update against the oracle evaluated
    from the kernel's own stored gradient, everything outside the jobs untouched."""
    stats = oo.new_stats()
    n1 = W_ROWS * W_COLS
    total = n1 + GAP + N2
    adam = bool(opt.get("adam"))
    inp = oo.inputs(total, seed=17, steps=2)
    gen = torch.Generator().manual_seed(3)
    keys = ("p", "m", "v") if adam else ("p", "mom")
    bufs = {k: oo.guarded(inp[k], dev) for k in keys}
    bufs["shadow"] = oo.guarded(torch.zeros(total), dev, torch.bfloat16)
    bufs["grad"] = oo.guarded(torch.full((total,), 0.25), dev)
    st = {k: v[1] for k, v in bufs.items()}
    wt = torch.full((W_COLS, W_ROWS), oo.SENT, dtype=torch.bfloat16, device=dev)
    sd = torch.zeros(1, dtype=torch.int32, device=dev)
    lrd = torch.zeros(1, device=dev)
    covered = torch.ones(total, dtype=torch.bool)
    covered[n1:n1 + GAP] = False
    for k in range(2):
        lr = (1e-3 if adam else 0.1) * (k + 1)
        lrd.fill_(lr)
        src1 = torch.randn(5, n1, generator=gen)
        src2 = torch.randn(3, N2, generator=gen)
        old = oo.snap(st)
        jobs = [(src1.to(dev), 5, n1, n1, st["grad"][:n1], 0.5, False, wt),
                (src2.to(dev), 3, N2, N2, st["grad"][n1 + GAP:], 2.0, False)]
        sgd = dict(grad=st["grad"], master=st["p"], shadow=st["shadow"], lr=-1.0, lr_dev=lrd,
                   weight_decay=opt["weight_decay"])
        if adam:
            sgd.update(adam=True, mom=st["m"], v=st["v"], betas=(0.8, 0.99), eps=1e-8,
                       decoupled=opt["decoupled"], step_dev=sd)
        else:
            sgd.update(mom=st["mom"] if opt["momentum"] else None, momentum=opt["momentum"])
        ops.reduce_multi(jobs, sgd=sgd, max_blocks=max_blocks)
        if adam:
            ops.step_advance(sd)
        got = oo.snap(st)
        # the reduction itself: (n_src - 1) additions and the scaling, relative to sum |terms|
        want = torch.cat([src1.double().sum(0) * 0.5, torch.full((GAP,), 0.25).double(),
                          src2.double().sum(0) * 2.0])
        mag = torch.cat([src1.double().abs().sum(0) * 0.5, torch.zeros(GAP).double(),
                         src2.double().abs().sum(0) * 2.0])
        assert bool(((got["grad"].double() - want).abs() <= 6 * 2.0 ** -24 * mag).all())
        sel = lambda d: {k: (t[covered] if t is not None else None) for k, t in d.items()}  # noqa: E731
        g = got["grad"][covered]
        what = f"reduce_multi {opt} max_blocks={max_blocks} step {k + 1}"
        if adam:
            oo.check_adam(sel(old), g, sel(got), lr=lr, betas=(0.8, 0.99), eps=1e-8,
                          weight_decay=opt["weight_decay"], decoupled=opt["decoupled"], t=k + 1,
                          stats=stats, what=what)
        else:
            gs = sel(got)
            if not opt["momentum"]:
                gs["mom"] = None
                assert torch.equal(got["mom"], old["mom"])
            oo.check_sgd(sel(old), g, gs, lr=lr, momentum=opt["momentum"],
                         weight_decay=opt["weight_decay"], stats=stats, what=what)
        for key in keys + ("shadow",):  # nothing outside the jobs' outputs moves
            assert torch.equal(got[key][~covered], old[key][~covered]), key
        assert torch.equal(wt.to(CPU), got["shadow"][:n1].view(W_ROWS, W_COLS).t())
    for key, (big, _) in bufs.items():
        oo.assert_guards(big, total, key)
    print("\n" + oo.statline(f"gpu reduce_multi {opt} max_blocks={max_blocks}", stats))


# ---- the weight-gradient GEMM epilogue ------------------------------------------------------

@pytest.mark.parametrize("R,N,K", [(128, 64, 64), (256, 128, 832), (128, 1024, 192)])
@pytest.mark.parametrize("momentum,weight_decay,shadow", [(0.0, 0.0, False), (0.9, 1e-2, True)])
def test_wgrad_epilogue_update_fp64(dev, monkeypatch, R, N, K, momentum, weight_decay, shadow):
    """ops.linear_wgrad(..., upd=, wt=): dz and x are small integers, so the gradient dz^T.x is
    exact and the fused sgd4 is checked against the oracle alone. master / mom / shadow / W^T
    are views (the output's row stride) inside sentinel buffers. The GPU epilogue does NOT
    store the gradient: ``slabs`` comes back untouched."""
    monkeypatch.setenv("DNN_BLAS", "0")
    stats = oo.new_stats()
    gen = torch.Generator().manual_seed(R + N + K)
    dz = torch.randint(-2, 3, (R, N), generator=gen).to(torch.bfloat16)
    x = torch.randint(-1, 2, (R, K), generator=gen).to(torch.bfloat16)
    grad = dz.double().t() @ x.double()
    inp = oo.inputs(N * K, seed=N + K, steps=1)
    sbuf, slabs = ao.padded(N, K, torch.float32, ao.SENTINEL, dev)
    pbuf, master = ao.padded(N, K, torch.float32, ao.SENTINEL, dev, inp["p"].view(N, K))
    mbuf, mom = ao.padded(N, K, torch.float32, ao.SENTINEL, dev, inp["mom"].view(N, K))
    hbuf, sh = ao.padded(N, K, torch.bfloat16, ao.SENTINEL, dev)
    tbuf, wt = ao.padded(K, N, torch.bfloat16, ao.SENTINEL, dev)
    lrd = torch.full((1,), 0.05, device=dev)
    upd = dict(master=master, mom=mom if momentum else None, shadow=sh if shadow else None,
               lr_dev=lrd, momentum=momentum, weight_decay=weight_decay)
    ops.linear_wgrad(dz.to(dev), x.to(dev), slabs, splits=1, upd=upd,
                     wt=wt if shadow else None)
    old = dict(p=inp["p"], mom=inp["mom"])
    got = dict(p=master.to(CPU).contiguous(), mom=mom.to(CPU).contiguous() if momentum else None,
               shadow=sh.to(CPU).contiguous() if shadow else None)
    what = f"wgrad upd {R}x{N}x{K} mu={momentum} wd={weight_decay}"
    oo.check_sgd(old, grad, got, lr=0.05, momentum=momentum, weight_decay=weight_decay,
                 stats=stats, what=what)
    assert bool((sbuf == ao.SENTINEL).all()), f"{what}: the gradient was stored to slabs"
    ao.assert_padding_untouched(pbuf, N, K, what=f"{what} master")
    ao.assert_padding_untouched(mbuf, N, K, what=f"{what} mom")
    if not momentum:
        assert torch.equal(mom.to(CPU), inp["mom"].view(N, K))
    if shadow:
        ao.assert_padding_untouched(hbuf, N, K, what=f"{what} shadow")
        ao.assert_padding_untouched(tbuf, K, N, what=f"{what} wt")
        assert torch.equal(wt, sh.t()), f"{what}: W^T is not the transposed shadow"
    else:
        assert bool((hbuf == ao.SENTINEL).all()) and bool((tbuf == ao.SENTINEL).all())
    print("\n" + oo.statline(what, stats))
