"""One training step of a model with sigmoid / linear hidden layers against the fp64 oracle
(cpu_ref.train_step), on the CPU path and on the GPU kernels.

The model is 784-256-128-64-10 with explicit per-layer activations; at pp = 2 and 4 a sigmoid or
linear layer ends a pipeline stage, so the next stage applies its derivative (Stage.prev_act).
Gradients are recovered from one SGD step without momentum, (W_before - W_after) / lr, and
compared per layer by relative L2 error with the oracle started from the same bf16-rounded
weights and inputs. A wrong derivative in one hidden layer gives ~0.75 in every layer below it;
the CPU path measures <= 2.2e-2 (weights), <= 1.0e-2 (biases), 1.3e-5 (loss)."""
import functools

import numpy as np
import pytest
import torch

from docker_dist_nn_amd import MLPSpec
from docker_dist_nn_amd.cpu_ref import train_step
from docker_dist_nn_amd.data import synthetic_mnist
from docker_dist_nn_amd.engine import OptimConfig, Trainer
from docker_dist_nn_amd.models.mlp import LayerSpec

WIDTHS = [784, 256, 128, 64, 10]
HIDDEN = [("sigmoid", "relu", "linear"), ("relu", "sigmoid", "sigmoid"),
          ("linear", "linear", "relu"), ("relu", "relu", "relu")]
LR, MICRO, NUM_MICRO = 0.2, 128, 2
CAP, LOSS_CAP = 5e-2, 1e-3

gpu = pytest.mark.gpu
CONFIGS = [pytest.param("cpu", pp, {}, id=f"cpu-pp{pp}") for pp in (1, 2, 4)] + [
    pytest.param("cuda", 1, {"DNN_TAIL": "0"}, marks=gpu, id="gpu-pp1-tail0"),
    pytest.param("cuda", 1, {"DNN_TAIL": "1"}, marks=gpu, id="gpu-pp1-tail1"),
    pytest.param("cuda", 2, {"DNN_NATIVE_EXEC": "0"}, marks=gpu, id="gpu-pp2-native0"),
    pytest.param("cuda", 2, {"DNN_NATIVE_EXEC": "1"}, marks=gpu, id="gpu-pp2-native1"),
    pytest.param("cuda", 4, {}, marks=gpu, id="gpu-pp4")]


def _spec(hidden):
    acts = list(hidden) + ["softmax"]
    return MLPSpec(tuple(LayerSpec(WIDTHS[i], WIDTHS[i + 1], acts[i],
                                   "output" if i == len(acts) - 1 else "hidden")
                         for i in range(len(acts))), "-".join(hidden))


@functools.lru_cache(maxsize=None)
def _batch():
    n = MICRO * NUM_MICRO
    x, y = synthetic_mnist(n, seed=11)
    xt = torch.zeros(n, 832, dtype=torch.bfloat16)
    xt[:, :784] = torch.from_numpy(x).to(torch.bfloat16)
    return xt, torch.from_numpy(y), y


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _errors(hidden, device, pp, check=None):
    """One engine step on ``device``; (loss error, per-layer weight-gradient errors, per-layer
    bias-gradient errors) against the fp64 oracle, all relative."""
    xt, yt, y = _batch()
    dev = torch.device(device)
    tr = Trainer(_spec(hidden), micro_batch=MICRO, num_micro=NUM_MICRO, pp=pp,
                 optim=OptimConfig(lr=LR), device=dev)
    if check is not None:
        check(tr)
    before = tr.local_weights()
    L = len(WIDTHS) - 1
    # the engine multiplies bf16 weights (fp32 masters, fp32 biases) with bf16 inputs
    W = [torch.from_numpy(before[i][0]).to(torch.bfloat16).double().numpy() for i in range(L)]
    B = [before[i][1].astype(np.float64) for i in range(L)]
    W0, B0 = [w.copy() for w in W], [b.copy() for b in B]
    ref_loss = train_step(W, B, list(hidden) + ["softmax"],
                          xt[:, :784].double().numpy(), y.astype(np.int64), LR)
    tr.set_batch(xt.to(dev), yt.to(dev))
    tr.step()
    loss = tr.loss()
    after = tr.local_weights()
    ew = [_rel((before[i][0].astype(np.float64) - after[i][0]) / LR, (W0[i] - W[i]) / LR)
          for i in range(L)]
    eb = [_rel((before[i][1].astype(np.float64) - after[i][1]) / LR, (B0[i] - B[i]) / LR)
          for i in range(L)]
    return abs(loss - ref_loss) / abs(ref_loss), ew, eb


@functools.lru_cache(maxsize=None)
def _cpu_errors(hidden, pp):
    return _errors(hidden, "cpu", pp)


@pytest.mark.parametrize("hidden", HIDDEN, ids="-".join)
@pytest.mark.parametrize("device,pp,env", CONFIGS)
def test_one_step_matches_fp64_oracle(monkeypatch, hidden, device, pp, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)

    def check(tr):  # the switch under test took effect
        if "DNN_TAIL" in env:
            assert tr.stages[-1].tail == (env["DNN_TAIL"] == "1")
        if "DNN_NATIVE_EXEC" in env:
            assert tr.native_exec == (env["DNN_NATIVE_EXEC"] == "1")

    el, ew, eb = _cpu_errors(hidden, pp) if device == "cpu" else _errors(hidden, device, pp, check)
    print(f"\nACTSTAT train {'-'.join(hidden)} {device} pp{pp} {env} loss {el:.2e} "
          f"dW {' '.join(f'{e:.2e}' for e in ew)} db {' '.join(f'{e:.2e}' for e in eb)}")
    assert el <= LOSS_CAP, el
    assert max(ew + eb) <= CAP, (ew, eb)
    if device != "cpu":
        # same rounding points as the CPU path, another accumulation order: factor 2
        _, cw, cb = _cpu_errors(hidden, pp)
        for i, (g, c) in enumerate(zip(ew + eb, cw + cb)):
            assert g <= 2.0 * c + 1e-3, (i, g, c)
