"""Training with the dense-target losses (Trainer(loss="mse" | "bce")) on the CPU path: one
step's loss and gradients against fp32 torch autograd from the same bf16-rounded weights (with
the softmax-CE step of the same model as a control), the loss/activation pairs that must be
refused, the untouched default, and the ``--loss mse --targets input`` command line.

Tolerances are the ones the cross-entropy step already has: losses rtol 2e-2 / atol 2e-3
(tests/test_engine_gpu.py), gradients rtol 2e-2 / atol 5e-2 on the UNNORMALISED gradient
(tests/test_kernels_gpu.py compares weight gradients of a unit-scale dz, so the engine's
gradient is multiplied back by its 1 / global_batch -- and 1 / n_out for the dense losses)."""
import json

import numpy as np
import pytest
import torch

from docker_dist_nn_amd import MLPSpec
from docker_dist_nn_amd.engine import OptimConfig, Trainer
from docker_dist_nn_amd.engine.stage import Stage

CPU = torch.device("cpu")
MB, NM = 64, 2
ROWS = MB * NM
ACT = {"linear": lambda v: v, "relu": torch.relu, "sigmoid": torch.sigmoid}


def _spec(widths, out_act):
    return MLPSpec.from_widths(widths, hidden_act="relu", out_act=out_act)


def _data(spec, seed=0):
    g = torch.Generator().manual_seed(seed)
    kp = (spec.in_dim + 63) // 64 * 64
    x = torch.zeros(ROWS, kp, dtype=torch.bfloat16)
    x[:, :spec.in_dim] = torch.rand(ROWS, spec.in_dim, generator=g).to(torch.bfloat16)
    return x, g


def _step(spec, loss, x, labels, targets, **kw):
    """One engine step from seed-3 weights; the step's loss and unpadded gradients, and the
    bf16-rounded initial weights the engine's GEMMs read."""
    tr = Trainer(spec, micro_batch=MB, num_micro=NM, device=CPU, optim=OptimConfig(lr=0.1),
                 seed=3, **({} if loss is None else {"loss": loss}), **kw)
    ww = tr.local_weights()
    w0 = [torch.from_numpy(ww[i][0]).to(torch.bfloat16).float() for i in range(len(spec.layers))]
    b0 = [torch.from_numpy(ww[i][1]) for i in range(len(spec.layers))]
    if targets is None:
        tr.set_batch(x, labels)
    else:
        tr.set_batch(x, labels, targets=targets)
    tr.step()
    grads = []
    for st in tr.stages:
        for i, gm in enumerate(st.geoms):
            o, k = gm.spec.out_dim, gm.spec.in_dim
            grads.append((st.params.gw(i).view(gm.np_, gm.kp)[:o, :k].clone(),
                          st.params.gb(i)[:o].clone()))
    return tr, grads, w0, b0


def _torch_forward(spec, w0, b0, x):
    ws = [w.clone().requires_grad_() for w in w0]
    bs = [b.clone().requires_grad_() for b in b0]
    h = x[:, :spec.in_dim].float()
    for i, (w, b) in enumerate(zip(ws, bs)):
        h = h @ w.t() + b
        if i < len(ws) - 1:
            h = torch.relu(h)
    return h, ws, bs


def _assert_grads(grads, ws, bs, unscale):
    for (gw, gb), w, b in zip(grads, ws, bs):
        torch.testing.assert_close(gw * unscale, w.grad * unscale, rtol=2e-2, atol=5e-2)
        torch.testing.assert_close(gb * unscale, b.grad * unscale, rtol=2e-2, atol=5e-2)
        assert float(w.grad.abs().max()) * unscale > 0.5  # the tolerance is not vacuous


@pytest.mark.parametrize("pp", [1, 2])
def test_bce_autoencoder_step_matches_autograd(pp):
    spec = _spec([96, 64, 96], "sigmoid")
    x, _ = _data(spec)
    t = x[:, :96].clone()
    tr, grads, w0, b0 = _step(spec, "bce", x, None, t, pp=pp)
    z, ws, bs = _torch_forward(spec, w0, b0, x)
    want = torch.nn.BCEWithLogitsLoss()(z, t.float())
    want.backward()
    np.testing.assert_allclose(tr.loss(), float(want.detach()), rtol=2e-2, atol=2e-3)
    _assert_grads(grads, ws, bs, ROWS * 96)
    assert tr.correct() is None


def test_mse_regressor_step_matches_autograd():
    spec = _spec([96, 64, 32], "linear")
    x, g = _data(spec)
    t = torch.randn(ROWS, 32, generator=g).to(torch.bfloat16)
    ok = torch.zeros(ROWS, dtype=torch.int32)
    ok[-5:] = -1  # padding rows: no loss, no gradient
    ok[7] = -1
    tr, grads, w0, b0 = _step(spec, "mse", x, ok, t)
    z, ws, bs = _torch_forward(spec, w0, b0, x)
    valid = (ok >= 0).float()
    want = (((z - t.float()) ** 2).mean(1) * valid).sum() / ROWS
    want.backward()
    np.testing.assert_allclose(tr.loss(), float(want.detach()), rtol=2e-2, atol=2e-3)
    _assert_grads(grads, ws, bs, ROWS * 32)
    # no padding rows: Trainer.loss() is nn.MSELoss (mean reduction)
    tr2, _, _, _ = _step(spec, "mse", x, None, t)
    np.testing.assert_allclose(tr2.loss(), float(torch.nn.MSELoss()(z.detach(), t.float())),
                               rtol=2e-2, atol=2e-3)


@pytest.mark.parametrize("act", ["relu", "sigmoid"])
def test_mse_other_activations_match_autograd(act):
    spec = _spec([96, 64, 32], act)
    x, g = _data(spec, seed=4)
    t = torch.rand(ROWS, 32, generator=g).to(torch.bfloat16)
    tr, grads, w0, b0 = _step(spec, "mse", x, None, t)
    z, ws, bs = _torch_forward(spec, w0, b0, x)
    want = torch.nn.MSELoss()(ACT[act](z), t.float())
    want.backward()
    np.testing.assert_allclose(tr.loss(), float(want.detach()), rtol=2e-2, atol=2e-3)
    _assert_grads(grads, ws, bs, ROWS * 32)


def test_softmax_ce_control_matches_autograd():
    """The same comparison on the existing loss: the harness and its tolerances are sound."""
    spec = _spec([96, 64, 32], "softmax")
    x, g = _data(spec)
    y = torch.randint(0, 32, (ROWS,), generator=g, dtype=torch.int32)
    tr, grads, w0, b0 = _step(spec, "softmax_ce", x, y, None)
    z, ws, bs = _torch_forward(spec, w0, b0, x)
    want = torch.nn.CrossEntropyLoss()(z, y.long())
    want.backward()
    np.testing.assert_allclose(tr.loss(), float(want.detach()), rtol=2e-2, atol=2e-3)
    _assert_grads(grads, ws, bs, ROWS)
    assert tr.correct() is not None


@pytest.mark.parametrize("loss,act", [("mse", "softmax"), ("bce", "softmax"), ("bce", "linear"),
                                      ("bce", "relu"), ("l1", "linear")])
def test_invalid_pairs_raise(loss, act):
    spec = _spec([96, 64, 32], act)
    with pytest.raises(ValueError, match="sigmoid|allowed"):
        Trainer(spec, micro_batch=MB, device=CPU, loss=loss)
    with pytest.raises(ValueError, match="sigmoid|allowed"):
        Stage(spec, 0, 2, micro_batch=MB, num_micro=1, device=CPU, loss=loss)


def test_other_trainers_refuse_dense_losses():
    from docker_dist_nn_amd.engine.fan_trainer import FanTrainer
    from docker_dist_nn_amd.parallel.tensor import TensorParallelMLP

    spec = _spec([96, 64, 32], "linear")
    with pytest.raises(ValueError, match="softmax_ce"):
        FanTrainer(spec, None, None, micro_batch=MB, num_micro=1, device=CPU, loss="mse")
    with pytest.raises(ValueError, match="softmax_ce"):
        TensorParallelMLP(spec, rows=64, tp=1, rank=0, device=CPU, loss="mse")


def test_batch_arguments():
    spec = _spec([96, 64, 32], "linear")
    x, g = _data(spec)
    t = torch.randn(ROWS, 32, generator=g).to(torch.bfloat16)
    tr = Trainer(spec, micro_batch=MB, num_micro=NM, device=CPU, loss="mse")
    with pytest.raises(ValueError, match="targets"):
        tr.set_batch(x, None)
    ce = Trainer(_spec([96, 64, 32], "softmax"), micro_batch=MB, num_micro=NM, device=CPU)
    with pytest.raises(ValueError, match="loss"):
        ce.set_batch(x, torch.zeros(ROWS, dtype=torch.int32), targets=t)
    # zero-copy: a full-width target buffer is read in place, a narrow one is copied
    full = torch.zeros(ROWS, 64, dtype=torch.bfloat16)
    full[:, :32] = t
    tr.set_batch(x, None, zero_copy=True, targets=full)
    assert tr.last.targets.data_ptr() == full.data_ptr()
    tr.step()
    l_zero_copy = tr.loss()
    tr2 = Trainer(spec, micro_batch=MB, num_micro=NM, device=CPU, loss="mse")
    tr2.set_batch(x, None, zero_copy=True, targets=t)
    assert tr2.last.targets.data_ptr() == tr2.last.targets_buf.data_ptr()
    tr2.step()
    assert tr2.loss() == l_zero_copy


def test_default_loss_is_bit_identical():
    spec = MLPSpec.parse("96-64-32")
    x, g = _data(spec)
    y = torch.randint(0, 32, (ROWS,), generator=g, dtype=torch.int32)
    out = []
    for loss in (None, "softmax_ce"):
        tr, _, _, _ = _step(spec, loss, x, y, None)
        for _ in range(2):
            tr.set_batch(x, y)
            tr.step()
        out.append((tr.loss(), tr.correct(), tr.local_weights()))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    for k in out[0][2]:
        assert np.array_equal(out[0][2][k][0], out[1][2][k][0])
        assert np.array_equal(out[0][2][k][1], out[1][2][k][1])


@pytest.mark.parametrize("args", [["--loss", "mse", "--targets", "input"],
                                  ["--loss", "bce", "--targets", "input"]])
def test_cli_autoencoder_smoke(capsys, args):
    from docker_dist_nn_amd.cli import train

    rc = train.main(["--model", "64-16-64", "--device", "cpu", "--synthetic", "512",
                     "--micro-batch", "64", "--epochs", "4", "--lr", "0.5", "--check-every", "0",
                     *args])
    assert rc == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep["loss_name"] == args[1] and rep["targets"] == "input" and rep["steps"] == 32
    assert np.isfinite(rep["loss"]) and rep["loss"] < rep["first_loss"], rep


def test_cli_onehot_and_evaluate(capsys):
    from docker_dist_nn_amd.cli import train

    rc = train.main(["--model", "64-16-10", "--device", "cpu", "--synthetic", "256",
                     "--micro-batch", "64", "--epochs", "3", "--lr", "0.5", "--check-every", "0",
                     "--loss", "bce", "--targets", "onehot"])
    assert rc == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep["loss"] < rep["first_loss"], rep
    with pytest.raises(ValueError, match="out_dim == in_dim"):
        train.main(["--model", "64-16-10", "--device", "cpu", "--synthetic", "64",
                    "--micro-batch", "64", "--loss", "mse", "--targets", "input"])
    # evaluate under a dense loss reports the mean loss of the served outputs
    rng = np.random.default_rng(0)
    x = rng.random((32, 8), dtype=np.float32)
    w, b = np.eye(8, dtype=np.float32), np.zeros(8, dtype=np.float32)
    rep = train.evaluate([w], [b], ["linear"], x, None, CPU, loss="mse", targets=x + 0.5)
    assert abs(rep["loss"] - 0.25) < 1e-2 and rep["loss_name"] == "mse"
