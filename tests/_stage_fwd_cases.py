"""Operands and fp64 oracles of the fused stage forward (ops.stage_fwd), CPU and GPU tests."""
import numpy as np
import torch

from docker_dist_nn_amd.config import LayerWeights

HEADLINE = [832, 512, 256, 128, 64]  # padded 784-512-256-128-10
REFUSED = [  # (padded widths, activations, n_cls, what): stage_fwd_supported is false for each
    ([64, 576, 64], ["relu", "linear"], 0, "width 576"),
    ([64] * 10, ["relu"] * 9, 0, "9 layers"),
    ([64, 64, 64], ["softmax", "linear"], 10, "hidden softmax"),
    ([64, 64, 128], ["relu", "softmax"], 65, "softmax wider than 64 classes")]


def exact_case(M, widths, seed, bias=True):
    """x in {-1, 0, 1}, nz weights of +-1 per weight row (3, or 1 for more than 4 layers), biases
    in {-1, 0, 1}: every pre-activation is an integer, exact in fp32 in any order."""
    g = np.random.default_rng(seed)
    nz = 3 if len(widths) <= 5 else 1
    x = g.integers(-1, 2, (M, widths[0])).astype(np.float64)
    ws, bs = [], []
    for k, n in zip(widths, widths[1:]):
        w = np.zeros((n, k))
        for r in range(n):
            w[r, g.choice(k, nz, replace=False)] = g.choice([-1.0, 1.0], nz)
        ws.append(w)
        bs.append(g.integers(-1, 2, n).astype(np.float64) if bias else None)
    return x, ws, bs


def chain64(x, ws, bs, acts, out_bf16=False, exact=False):
    """fp64 chain and the running forward bound e of the kernel's error beside it: e_out = |W|
    e_in + K 2^-24 |W||h_in|, through the activation (Lipschitz 1, sigmoid 1/4 plus its own
    (|z| + 8) 2^-23 of _act_oracle.check_fwd), plus 2^-9 (|h| + e) wherever the kernel rounds
    to bf16. ``exact``: asserts every pre-activation an integer <= 256 instead (e is then 0)."""
    h, e = x, np.zeros_like(x)
    for l, (w, b, a) in enumerate(zip(ws, bs, acts)):
        z = h @ w.T + (0 if b is None else b)
        if exact:
            assert np.abs(z).max() <= 256 and (z == np.round(z)).all() and a != "sigmoid"
        else:
            e = e @ np.abs(w).T + w.shape[1] * 2.0 ** -24 * (np.abs(h) @ np.abs(w).T)
            if a == "sigmoid":
                e = e / 4 + (np.abs(z) + e + 8) * 2.0 ** -23
        h = np.maximum(z, 0) if a == "relu" else 1 / (1 + np.exp(-z)) if a == "sigmoid" else z
        if not exact and (l < len(ws) - 1 or out_bf16):
            e = e + 2.0 ** -9 * (np.abs(h) + e)
    return h, e


def random_case(M, widths, seed):
    g = torch.Generator().manual_seed(seed)
    bf = lambda t: t.to(torch.bfloat16).double().numpy()  # noqa: E731 (bf16 values, as fp64)
    x = bf(torch.randn(M, widths[0], generator=g))
    ws = [bf(torch.randn(n, k, generator=g) / k ** 0.5) for k, n in zip(widths, widths[1:])]
    bs = [torch.randn(n, generator=g).float().double().numpy() * 0.5 for n in widths[1:]]
    return x, ws, bs


def model_layers(dims, acts, seed):
    g = np.random.default_rng(seed)
    return [LayerWeights(weight=g.standard_normal((n, k)) / np.sqrt(k),
                         bias=g.standard_normal(n) * 0.1, activation=a)
            for k, n, a in zip(dims, dims[1:], acts)]
