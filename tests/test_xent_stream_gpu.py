"""ops.linear_xent_stream (csrc/kernels/xent_stream.hip) against the fp64 oracle of
tests/_loss_oracle.py on exact-logit operands, at the tight bounds of
tests/_wide_softmax_oracle.py with the kernel's documented chain D = 4 ceil(n_cls / 128) + 19;
its argument checks; and StreamXentHead inside a Trainer."""
import numpy as np
import pytest
import torch

import _loss_oracle as lo
import _wide_softmax_oracle as wo
from _act_oracle import CPU, PAD, SENTINEL
from docker_dist_nn_amd import MLPSpec, ops
from docker_dist_nn_amd.engine import OptimConfig, Trainer
from docker_dist_nn_amd.engine.loss_head import StreamXentHead, XentHead

pytestmark = pytest.mark.gpu

CASES = [(64, 64, 10, 64), (192, 192, 130, 128), (192, 320, 257, 192), (128, 1088, 1025, 64),
         (64, 128, 100, ops.XENT_STREAM_MAX_K)]  # M, Np, n_cls, K


def depth(n_cls):
    return 4 * -(-n_cls // 128) + 19


def exact_case(M, Np, n_cls, K, seed):
    """lo.gemm_case; beyond its 128 features, more of the same recipe: x in multiples of 1/16,
    w in {-1, 0, 1} * 2^s, s in -2 .. 0 (every product a multiple of 2^-6, every sum below 2^12:
    exact in fp32 in any order), the four edge rows left as they are, padding weights non-zero."""
    case = lo.gemm_case(M, Np, min(K, 128), n_cls, seed)
    if K > 128:
        g = torch.Generator().manual_seed(seed + 1)
        xe = torch.randint(-16, 17, (M, K - 128), generator=g).double() / 16
        xe[:4] = 0.0
        we = lo._pow2((Np, K - 128), g, -2, 0)
        we[n_cls:] = lo._pow2((Np - n_cls, K - 128), g, -2, 7, zeros=False)
        x = torch.cat([case["x"].double(), xe], 1)
        w = torch.cat([case["w"].double(), we], 1)
        z = x @ w[:n_cls].t() + case["bias"][:n_cls].double()
        z32 = x.float() @ w[:n_cls].float().t() + case["bias"][:n_cls]
        assert torch.equal(z32.double(), z), "logits not exact in fp32 (test bug)"
        assert torch.equal(z[:4], case["z"][:4])
        case.update(K=K, x=x.to(torch.bfloat16), w=w.to(torch.bfloat16), z=z)
    return case


def _view(rows, cols, dtype, fill, dev, shift):
    """(buffer, strided [rows][cols] view), 16-byte aligned or (``shift``) off every boundary."""
    buf = torch.full((rows + 2, cols + PAD + shift + 3), fill, dtype=dtype, device=dev)
    return buf, buf[1:1 + rows, PAD + shift:PAD + shift + cols]


def _untouched(buf, view, c0, fill, what):
    o = buf.to(CPU).clone()
    r, c = view.shape
    o[1:1 + r, c0:c0 + c] = fill
    assert bool((o == fill).all()), f"{what}: wrote outside its view"


def _launch(case, scale, dev, shift):
    M, Np, nb = case["M"], case["Np"], case["M"] // 64
    out = dict(zip(("dzbuf", "dz"), _view(M, Np, torch.bfloat16, SENTINEL, dev, shift)))
    out["csbuf"], out["cs"] = _view(nb, Np, torch.float32, SENTINEL, dev, shift)
    out["lp"] = torch.full((nb + 1,), SENTINEL, dtype=torch.float32, device=dev)
    out["co"] = torch.full((nb + 1,), lo.ISENT, dtype=torch.int32, device=dev)
    ops.linear_xent_stream(case["x"].to(dev), case["w"].to(dev), case["bias"].to(dev), out["dz"],
                           case["labels"].to(dev), case["n_cls"], scale, out["lp"], out["co"],
                           colsum=out["cs"])
    return {k: v.to(CPU) for k, v in out.items()}


@pytest.mark.parametrize("idx", range(len(CASES)), ids=["x".join(map(str, c)) for c in CASES])
def test_linear_xent_stream_exact_logits(dev, idx):
    M, Np, n_cls, K = CASES[idx]
    case, scale, nb, shift = exact_case(M, Np, n_cls, K, 40 + idx), 1.0 / M, M // 64, idx % 2
    what = f"linear_xent_stream {M}x{Np}x{K} cls={n_cls} shift={shift}"
    out = _launch(case, scale, dev, shift)
    ref = lo.xent_ref(case["z"], case["labels"], scale)
    own, d, stats = lo.owners(M, 64), depth(n_cls), lo.new_stats()
    wo.assert_dz_tight(out["dz"], ref, Np, stats, what, d)
    assert bool((out["dz"][case["labels"] < 0] == 0).all()), f"{what}: padding rows not zero"
    wo.assert_loss_partials_tight(out["lp"], ref, own, nb, stats, what, d)
    lo.assert_correct_partials(out["co"], ref, own, nb, what=what)
    lo.assert_colsum_partials(out["cs"], out["dz"], own, nb, stats, what)
    print(lo.statline(what, stats))
    assert float(out["lp"][nb]) == SENTINEL and int(out["co"][nb]) == lo.ISENT
    _untouched(out["dzbuf"], out["dz"], PAD + shift, SENTINEL, what + " dz")
    _untouched(out["csbuf"], out["cs"], PAD + shift, SENTINEL, what + " colsum")
    again = _launch(case, scale, dev, shift)
    for k in ("dzbuf", "csbuf", "lp", "co"):
        assert torch.equal(out[k], again[k]), f"{what}: {k} differs between two launches"


def test_linear_xent_stream_argument_errors(dev):
    bf, f32, i32 = torch.bfloat16, torch.float32, torch.int32
    z = lambda *s, dt=bf: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
    ok = dict(x=z(64, 64), w=z(128, 64), bias=z(128, dt=f32), dz=z(64, 128),
              labels=z(64, dt=i32), n_cls=100, scale=1.0, loss_part=z(1, dt=f32),
              correct=z(1, dt=i32), colsum=z(1, 128, dt=f32))
    ops.linear_xent_stream(**ok)
    kmax = ops.XENT_STREAM_MAX_K
    bad = [(TypeError, dict(x=z(64, 64, dt=f32))), (TypeError, dict(dz=z(64, 128, dt=f32))),
           (ValueError, dict(x=z(96, 64), dz=z(96, 128), labels=z(96, dt=i32))),
           (ValueError, dict(x=z(64, kmax + 64), w=z(128, kmax + 64))),
           (ValueError, dict(x=z(64, 96), w=z(128, 96))), (ValueError, dict(n_cls=129)),
           (ValueError, dict(bias=None)), (ValueError, dict(labels=z(64, dt=torch.int64))),
           (ValueError, dict(x=z(128, 64), dz=z(128, 128), labels=z(128, dt=i32))),  # partials
           (ValueError, dict(correct=z(1, dt=f32))), (ValueError, dict(colsum=z(1, 64, dt=f32)))]
    for exc, kw in bad:
        with pytest.raises(exc):
            ops.linear_xent_stream(**{**ok, **kw})


ROWS, LR = 128, 0.5
SPEC = MLPSpec.from_widths([200, 136, 72, 300])


def _train(monkeypatch, dev, stream, native, x, y, steps=3):
    monkeypatch.setenv("DNN_XENT_STREAM", stream)
    monkeypatch.setenv("DNN_NATIVE_EXEC", native)
    tr = Trainer(SPEC, device=dev, micro_batch=64, num_micro=2, optim=OptimConfig(lr=LR))
    w0, first = tr.local_weights(), None
    for _ in range(steps):
        tr.set_batch(x, y)
        tr.step()
        first = first or (tr.loss() * ROWS, tr.correct())
    return tr, w0, first


def _logits(ps, x):  # (input of the last layer, logits) in fp64
    h = x.double()
    for w, b in ps[:-1]:
        h = torch.relu(h @ w.t() + b)
    return h, h @ ps[-1][0].t() + ps[-1][1]


def _oracle(w0, x, y, steps):
    """(max |h| . |w| + |b| at the start, parameters after ``steps`` fp64 autograd SGD steps)."""
    ps = [[torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=True) for a in w0[k]]
          for k in sorted(w0)]
    valid = y >= 0
    with torch.no_grad():
        h = _logits(ps, x)[0]
        mag = float((h.abs() @ ps[-1][0].abs().t() + ps[-1][1].abs()).max())
    for _ in range(steps):
        z = _logits(ps, x)[1]
        loss = torch.nn.functional.cross_entropy(z[valid], y[valid].long(), reduction="sum") / ROWS
        grads = torch.autograd.grad(loss, [p for wb in ps for p in wb])
        with torch.no_grad():
            for p, gr in zip([p for wb in ps for p in wb], grads):
                p -= LR * gr
    return mag, ps


def test_trainer_on_stream_xent_head(dev, monkeypatch):
    assert [l.activation for l in SPEC.layers] == ["relu", "relu", "softmax"]
    g = torch.Generator().manual_seed(3)
    x = torch.rand(ROWS, 200, generator=g).to(torch.bfloat16)
    y = torch.randint(0, 300, (ROWS,), generator=g, dtype=torch.int32)
    y[[5, 77, ROWS - 1]] = -1
    xd, yd = torch.nn.functional.pad(x, (0, 56)).to(dev), y.to(dev)  # Kp = 256 columns
    new, w0, (ln, cn) = _train(monkeypatch, dev, "1", "1", xd, yd)
    py, _, (lpy, cpy) = _train(monkeypatch, dev, "1", "0", xd, yd)
    old, w0o, (lold, cold) = _train(monkeypatch, dev, "0", "1", xd, yd)
    st = new.last
    assert type(st.head) is StreamXentHead and type(old.last.head) is XentHead
    assert st.acts[-1].shape[0] == 0 and old.last.acts[-1].shape[0] == ROWS
    assert new.native_exec and not py.native_exec and (ln, cn) == (lpy, cpy)
    wn, wp, wold = new.local_weights(), py.local_weights(), old.local_weights()
    for k in wn:  # native replay == the Python executor, bit for bit
        assert np.array_equal(wn[k][0], wp[k][0]) and np.array_equal(wn[k][1], wp[k][1])
        assert np.array_equal(w0[k][0], w0o[k][0])
    # Step-1 loss: each head within the tight bound of its own chain (test 1; the wide kernel's
    # chain for XentHead) of the loss of ITS logits; the two logit sets are fp32 sums of the
    # same Kp = 128 products in different orders, each within (Kp + 1) u (|h| . |w| + |b|) = d
    # of the exact one, and a row's loss moves by at most 2 d with it (tests/_step_audit.py).
    mag, want = _oracle(w0, x, y, 3)
    nval, u = int((y >= 0).sum()), lo.U
    d = 129 * u * mag
    bound = sum(18 * u * lold + nval * wo.loss_terms(300, dd) * u
                for dd in (depth(300), None)) + nval * 2 * 2 * d
    print(f"XENTSTREAM step-1 loss sums new {ln:.6f} old {lold:.6f} bound {bound:.2e}")
    assert abs(ln - lold) <= bound and cn == cold
    dist = [max(float((torch.tensor(np.asarray(a)).double() - p.detach()).abs().max())
                for k, wb in enumerate(want) for a, p in zip(ws[k], wb)) for ws in (wn, wold)]
    print(f"XENTSTREAM master distance to the fp64 oracle: new {dist[0]:.3e} old {dist[1]:.3e}")
    assert dist[0] <= 2 * dist[1]
