"""Softmax classifiers wider than 256 classes on the GPU, end to end (the wide cross-entropy
kernel inside the step, the wide row softmax inside the serving engine), modelled on
tests/test_dense_engine_gpu.py and with its tolerances: parity with the CPU reference path,
2-stage loopback pipeline == 1 stage, native replay == the Python executor bit for bit,
HIP-graph replay == eager, two runs bitwise equal, serving against the fp64 oracle, and the
training CLI."""
import json
import math

import numpy as np
import pytest
import torch

import _loss_oracle as lo
import _wide_softmax_oracle as wo
from docker_dist_nn_amd import MLPSpec
from docker_dist_nn_amd.config import LayerWeights, load_model_config
from docker_dist_nn_amd.cpu_ref import model_forward
from docker_dist_nn_amd.engine import OptimConfig, Trainer
from docker_dist_nn_amd.engine.inference import InferenceEngine

pytestmark = pytest.mark.gpu

MB, NM = 64, 2
ROWS = MB * NM
C300 = MLPSpec.from_widths([128, 64, 300])    # Np = 320: the narrowest wide output
C1000 = MLPSpec.from_widths([128, 64, 1000])  # Np = 1024: one full sweep


def _batch(spec, dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(ROWS, spec.in_dim, generator=g).to(torch.bfloat16)
    y = torch.randint(0, spec.out_dim, (ROWS,), generator=g, dtype=torch.int32)
    y[[5, 77, ROWS - 1]] = -1  # padding rows
    return x.to(dev), y.to(dev)


def _run(spec, dev, steps, lr=0.5, **kw):
    tr = Trainer(spec, device=dev, micro_batch=MB, num_micro=NM, optim=OptimConfig(lr=lr), **kw)
    x, y = _batch(spec, dev)
    losses, correct = [], []
    for _ in range(steps):
        tr.set_batch(x, y)
        tr.step()
        losses.append(tr.loss())
        correct.append(tr.correct())
    return tr, losses, correct


def _same_weights(ta, tb):
    wa, wb = ta.local_weights(), tb.local_weights()
    for k in wa:
        assert np.array_equal(wa[k][0], wb[k][0]) and np.array_equal(wa[k][1], wb[k][1])


@pytest.mark.parametrize("spec", [C300, C1000])
def test_gpu_wide_classifier_matches_cpu_reference(dev, spec):
    assert spec.layers[-1].activation == "softmax"
    tg, lg, cg = _run(spec, dev, 8)
    _, lc, cc = _run(spec, torch.device("cpu"), 8)
    assert lg[-1] < lg[0]
    np.testing.assert_allclose(lg, lc, rtol=2e-2, atol=2e-3)
    assert cg[0] == cc[0]
    st = tg.last
    assert not st.fused_xent and not st.tail and not st.dense
    assert st.dz[-1].shape[1] == (spec.out_dim + 63) // 64 * 64 > 256


def test_gpu_wide_classifier_pipeline_equals_single_stage(dev):
    t1, l1, c1 = _run(C300, dev, 4)
    tp, lp, cp = _run(C300, dev, 4, pp=2)
    np.testing.assert_allclose(lp, l1, rtol=1e-3, atol=1e-4)
    assert cp[0] == c1[0]
    w1, wp = t1.local_weights(), tp.local_weights()
    for k in w1:
        np.testing.assert_allclose(wp[k][0], w1[k][0], rtol=1e-3, atol=1e-5)


@pytest.mark.parametrize("pp", [1, 2])
def test_wide_classifier_native_executor_equals_python(dev, pp):
    out = []
    for native_exec in (False, True):
        tr, losses, correct = _run(C300, dev, 4, pp=pp, native_exec=native_exec)
        assert tr.native_exec == native_exec
        out.append((tr, losses, correct))
    (t0, l0, c0), (t1, l1, c1) = out
    assert l0 == l1 and c0 == c1 and len(set(l0)) == 4
    _same_weights(t0, t1)


def test_gpu_wide_classifier_graph_replay_equals_eager(dev):
    x, y = _batch(C1000, dev)
    ta = Trainer(C1000, device=dev, micro_batch=MB, num_micro=NM, optim=OptimConfig(lr=0.5))
    tb = Trainer(C1000, device=dev, micro_batch=MB, num_micro=NM, optim=OptimConfig(lr=0.5))
    ta.set_batch(x, y)
    tb.set_batch(x, y)
    tb.capture(warmup=0)  # capture executes one real step
    ta.step()
    la, lb = [ta.loss()], [tb.loss()]
    for k in range(4):
        xs, ys = x.roll(k + 1, 0).contiguous(), y.roll(k + 1, 0).contiguous()
        ta.set_batch(xs, ys)
        ta.step()
        tb.set_batch(xs, ys)
        tb.step()
        la.append(ta.loss())
        lb.append(tb.loss())
    assert la == lb and ta.correct() == tb.correct()
    _same_weights(ta, tb)


def test_gpu_wide_classifier_bitwise_deterministic(dev):
    ta, la, ca = _run(C1000, dev, 3)
    tb, lb, cb = _run(C1000, dev, 3)
    assert la == lb and ca == cb
    _same_weights(ta, tb)


def test_engine_serves_a_trained_1000_way_model(dev):
    """The served probabilities against the fp64 softmax of the engine's OWN fp32 logits (a
    second engine over the same weights with a linear output: the same GEMM launch). These
    logits are no multiples of 1/4, so x - mx rounds: one more u relative per unit of t in
    e_c, ln(n_cls) + 1 more terms by the argument of the oracle's docstring."""
    tr, _, _ = _run(C1000, dev, 8)
    ww = tr.local_weights()
    acts = [l.activation for l in C1000.layers]
    layers = [LayerWeights(ww[i][0], ww[i][1], a) for i, a in enumerate(acts)]
    logit_layers = [LayerWeights(ww[i][0], ww[i][1], "linear" if a == "softmax" else a)
                    for i, a in enumerate(acts)]
    eng = InferenceEngine([layers], dev, expected_input=128)
    eng_z = InferenceEngine([logit_layers], dev, expected_input=128)
    for rows in (70, 2):  # MFMA path and the serving-size GEMV path
        x = np.random.default_rng(rows).random((rows, 128))
        p, z = np.asarray(eng.predict(x)), np.asarray(eng_z.predict(x))
        assert p.shape == z.shape == (rows, 1000)
        zt = torch.from_numpy(z.astype(np.float32))
        assert torch.equal(zt.double(), torch.from_numpy(z).double())  # fp32 values, unrounded
        ref = lo.xent_ref(zt.double(), torch.zeros(rows, dtype=torch.int32), 1.0)
        wo.assert_probs_tight(torch.from_numpy(p), ref, what=f"engine 1000-way rows={rows}",
                              depth=wo.kernel_depth(1000) + math.log(1000) + 1)
        np.testing.assert_allclose(p.sum(1), 1.0, atol=1e-5)
        np.testing.assert_allclose(p, model_forward(layers, x), atol=1e-2)


def test_hidden_wide_softmax_and_linear_output(dev):
    rng = np.random.default_rng(0)
    dims, acts = [100, 320, 32], ["softmax", "linear"]
    L = [LayerWeights(rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i]),
                      rng.standard_normal(dims[i + 1]) * 0.1, acts[i]) for i in range(2)]
    eng = InferenceEngine([L], dev, expected_input=100)
    for rows in (70, 2):
        x = np.random.default_rng(rows).random((rows, 100))
        np.testing.assert_allclose(eng.predict(x), model_forward(L, x), rtol=2e-2, atol=2e-2)


def test_cli_trains_a_300_way_classifier(capsys, tmp_path):
    from docker_dist_nn_amd.cli import train
    from docker_dist_nn_amd.data import synthetic_mnist

    out = tmp_path / "wide.json"
    rc = train.main(["--model", "128-64-300", "--synthetic", "1024", "--micro-batch", "128",
                     "--epochs", "1", "--lr", "0.2", "--check-every", "0", "--save", str(out)])
    assert rc == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep["steps"] == 8 and np.isfinite(rep["loss"]) and 0.0 < rep["loss"] < 10.0, rep
    mc = load_model_config(str(out))
    assert [L.activation for L in mc.layers][-1] == "softmax" and mc.layers[-1].out_dim == 300
    x, y = synthetic_mnist(256, seed=3, dim=128)
    ev = train.evaluate([L.weight for L in mc.layers], [L.bias for L in mc.layers],
                        [L.activation for L in mc.layers], x, y, torch.device("cuda", 0))
    assert np.isfinite(ev["accuracy"]) and 0.0 <= ev["accuracy"] <= 1.0, ev
