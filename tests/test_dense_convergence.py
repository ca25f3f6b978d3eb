"""Convergence parity of a dense-loss model with a plain fp32 ``torch.nn`` trainer, in the form
of tests/test_convergence_cpu.py and with its margins (per-epoch mean losses within
0.05 * b + 0.01): a 64-16-64 sigmoid / binary-cross-entropy autoencoder on low-rank synthetic
data, same initial weights, same batches, same optimizer (Adam, lr 1e-3, batch 64). The CPU
run uses the engine's reference path, the GPU run (marked gpu) the gfx950 kernels."""
import numpy as np
import pytest
import torch

from docker_dist_nn_amd import MLPSpec
from docker_dist_nn_amd.engine import OptimConfig, Trainer

SPEC = MLPSpec.from_widths([64, 16, 64], hidden_act="relu", out_act="sigmoid")
EPOCHS, BATCH, N = 3, 64, 4096


def _data():
    """Rank-4 data in (0, 1), rounded to bf16 so that both trainers see the same numbers."""
    g = torch.Generator().manual_seed(11)
    lat = torch.randn(N, 4, generator=g)
    basis = torch.randn(4, 64, generator=g)
    return torch.sigmoid(lat @ basis).to(torch.bfloat16)


def _run(device):
    x = _data()
    tr = Trainer(SPEC, micro_batch=BATCH, num_micro=1, device=device, seed=5,
                 optim=OptimConfig(name="adam", lr=1e-3), loss="bce")
    ww = tr.local_weights()
    l1, l2 = torch.nn.Linear(64, 16), torch.nn.Linear(16, 64)
    with torch.no_grad():
        for lin, (w, b) in zip((l1, l2), (ww[0], ww[1])):
            lin.weight.copy_(torch.from_numpy(w))
            lin.bias.copy_(torch.from_numpy(b))
    ref = torch.nn.Sequential(l1, torch.nn.ReLU(), l2)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    lossf = torch.nn.BCEWithLogitsLoss()
    xd = x.to(device)
    ours_ep, ref_ep = [], []
    for ep in range(EPOCHS):
        order = torch.from_numpy(np.random.default_rng(100 + ep).permutation(N))
        lo, lr_ = [], []
        for s in range(0, N, BATCH):
            idx = order[s:s + BATCH]
            xb = xd[idx.to(device)].contiguous()
            tr.set_batch(xb, None, targets=xb)
            tr.step()
            lo.append(tr.loss())
            opt.zero_grad()
            xf = x[idx].float()
            loss = lossf(ref(xf), xf)
            loss.backward()
            opt.step()
            lr_.append(float(loss.detach()))
        ours_ep.append(float(np.mean(lo)))
        ref_ep.append(float(np.mean(lr_)))
    return ours_ep, ref_ep


def _check(ours_ep, ref_ep):
    for a, b in zip(ours_ep, ref_ep):  # bf16 operands: a few % of the epoch-mean loss
        assert abs(a - b) <= 0.05 * b + 0.01, (ours_ep, ref_ep)
    assert ours_ep[-1] < ours_ep[0] and ref_ep[-1] < ref_ep[0], (ours_ep, ref_ep)
    print(f"\ndense convergence: ours {ours_ep} torch {ref_ep}")


def test_bce_autoencoder_convergence_parity_cpu():
    _check(*_run(torch.device("cpu")))


@pytest.mark.gpu
def test_bce_autoencoder_convergence_parity_gpu(dev):
    _check(*_run(dev))
