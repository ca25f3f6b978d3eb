"""Training with the dense-target losses on the GPU (csrc/kernels/dense_loss.hip inside the
step), modelled on tests/test_engine_gpu.py and with its tolerances: parity with the CPU
reference path, 2-stage loopback pipeline == 1 stage, native replay == the Python executor bit
for bit (zero-copy targets relocated without re-recording), HIP-graph replay == eager, two runs
bitwise equal, and an output wider than 256 columns (two column chunks of the loss kernel)."""
import numpy as np
import pytest
import torch

from docker_dist_nn_amd import MLPSpec
from docker_dist_nn_amd.engine import OptimConfig, Trainer

pytestmark = pytest.mark.gpu

MB, NM = 64, 2
ROWS = MB * NM
AE = MLPSpec.from_widths([192, 128, 192], hidden_act="relu", out_act="sigmoid")  # autoencoder
WIDE = MLPSpec.from_widths([128, 64, 300], hidden_act="relu", out_act="linear")  # Np = 320


def _batch(spec, dev, seed=1):
    """Inputs [ROWS][Kp] in [0, 1), targets [ROWS][Np] (the inputs for the autoencoder), and a
    validity vector with a few padding rows."""
    g = torch.Generator().manual_seed(seed)
    kp, np_ = (spec.in_dim + 63) // 64 * 64, (spec.out_dim + 63) // 64 * 64
    x = torch.zeros(ROWS, kp, dtype=torch.bfloat16)
    x[:, :spec.in_dim] = torch.rand(ROWS, spec.in_dim, generator=g).to(torch.bfloat16)
    if spec.out_dim == spec.in_dim:
        t = x.clone()
    else:
        t = torch.zeros(ROWS, np_, dtype=torch.bfloat16)
        t[:, :spec.out_dim] = torch.randn(ROWS, spec.out_dim, generator=g).to(torch.bfloat16)
    ok = torch.zeros(ROWS, dtype=torch.int32)
    ok[[5, ROWS - 1]] = -1
    return x.to(dev), t.to(dev), ok.to(dev)


def _run(spec, loss, dev, steps, lr=30.0, **kw):
    tr = Trainer(spec, device=dev, micro_batch=MB, num_micro=NM, optim=OptimConfig(lr=lr),
                 loss=loss, **kw)
    x, t, ok = _batch(spec, dev)
    losses = []
    for _ in range(steps):
        tr.set_batch(x, ok, targets=t)
        tr.step()
        losses.append(tr.loss())
    return tr, losses


@pytest.mark.parametrize("spec,loss", [(AE, "bce"), (AE, "mse"), (WIDE, "mse")])
def test_gpu_dense_training_matches_cpu_reference(dev, spec, loss):
    lr = 30.0 if spec is AE else 5.0
    tg, lg = _run(spec, loss, dev, 8, lr=lr)
    _, lc = _run(spec, loss, torch.device("cpu"), 8, lr=lr)
    assert lg[-1] < lg[0]
    np.testing.assert_allclose(lg, lc, rtol=2e-2, atol=2e-3)
    assert tg.correct() is None and not tg.last.fused_xent and not tg.last.tail


def test_gpu_wide_output_trains(dev):
    """320 padded output columns: more than the 256 the stand-alone cross-entropy kernel takes."""
    tr, losses = _run(WIDE, "mse", dev, 6, lr=5.0)
    st = tr.last
    assert st.dz[-1].shape[1] == 320 and st.head.chunks == 2
    assert st.loss_part.numel() == st.head.blocks * 2 * NM
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_gpu_dense_pipeline_equals_single_stage(dev):
    t1, l1 = _run(AE, "bce", dev, 4)
    tp, lp = _run(AE, "bce", dev, 4, pp=2)
    np.testing.assert_allclose(lp, l1, rtol=1e-3, atol=1e-4)
    w1, wp = t1.local_weights(), tp.local_weights()
    for k in w1:
        np.testing.assert_allclose(wp[k][0], w1[k][0], rtol=1e-3, atol=1e-5)


def test_gpu_dense_graph_replay_equals_eager(dev):
    x, t, ok = _batch(AE, dev)
    ta = Trainer(AE, device=dev, micro_batch=MB, num_micro=NM, optim=OptimConfig(lr=30.0),
                 loss="bce")
    tb = Trainer(AE, device=dev, micro_batch=MB, num_micro=NM, optim=OptimConfig(lr=30.0),
                 loss="bce")
    ta.set_batch(x, ok, targets=t)
    tb.set_batch(x, ok, targets=t)
    tb.last.bind_targets(t)  # targets read in place before the capture ...
    tb.capture(warmup=0)  # capture executes one real step
    assert tb.last.targets.data_ptr() == tb.last.targets_buf.data_ptr()  # ... fixed after it
    ta.step()
    la, lb = [ta.loss()], [tb.loss()]
    for k in range(4):
        xs = x.roll(k + 1, 0).contiguous()
        ta.set_batch(xs, ok, targets=xs)
        ta.step()
        tb.set_batch(xs, ok, targets=xs)
        tb.step()
        la.append(ta.loss())
        lb.append(tb.loss())
    assert la == lb
    wa, wb = ta.local_weights(), tb.local_weights()
    for k in wa:
        assert np.array_equal(wa[k][0], wb[k][0])


def test_gpu_dense_bitwise_deterministic(dev):
    ta, la = _run(WIDE, "mse", dev, 3, lr=5.0)
    tb, lb = _run(WIDE, "mse", dev, 3, lr=5.0)
    assert la == lb
    wa, wb = ta.local_weights(), tb.local_weights()
    for k in wa:
        assert np.array_equal(wa[k][0], wb[k][0]) and np.array_equal(wa[k][1], wb[k][1])


@pytest.mark.parametrize("pp", [1, 2])
def test_dense_native_executor_equals_python(dev, pp):
    """Recorded-launch replay == the Python op-by-op path, bit for bit, with the targets bound
    zero-copy to a different buffer each step (relocated inside the recorded program)."""
    x, _, ok = _batch(AE, dev)
    out = []
    for native_exec in (False, True):
        tr = Trainer(AE, device=dev, micro_batch=MB, num_micro=NM, pp=pp,
                     optim=OptimConfig(lr=5.0, momentum=0.9), native_exec=native_exec,
                     loss="bce")
        assert tr.native_exec == native_exec
        prog = tr.last._prog
        losses = []
        for k in range(4):
            xs = x.roll(k * 8, 0).contiguous()  # a different buffer each step
            ts = xs.clone()
            oks = ok.roll(k, 0).contiguous()
            tr.set_batch(xs, oks, zero_copy=True, targets=ts)
            assert tr.last.targets.data_ptr() == ts.data_ptr()
            tr.step()
            losses.append(tr.loss())
        assert tr.last._prog is prog  # nothing was re-recorded
        out.append((losses, tr.local_weights()))
    (l0, w0), (l1, w1) = out
    assert l0 == l1 and len(set(l0)) == 4
    for k in w0:
        assert np.array_equal(w0[k][0], w1[k][0]) and np.array_equal(w0[k][1], w1[k][1])
