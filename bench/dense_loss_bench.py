"""Dense-target loss micro-benchmark: ops.dense_loss (csrc/kernels/dense_loss.hip) against the
same loss written as torch eager ops, on the same GPU in the same process, plus the step time of
a 784-512-128-512-784 bce autoencoder. One JSON line per case.

Both contenders produce the same outputs -- the loss sum, dz in bf16 and the bias gradient
(column sums of dz) -- from random data, and every call works on the next of several buffer
sets that together exceed the 256-MiB Infinity Cache, so each pass streams from HBM. The two
are timed in alternating rounds with device events; median and minimum over the rounds are
reported. Effective bytes/s counts 8 B per element (4 B z + 2 B t read, 2 B dz written)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from docker_dist_nn_amd import MLPSpec, ops  # noqa: E402
from docker_dist_nn_amd.engine import OptimConfig, Trainer  # noqa: E402

CACHE_BYTES = 256 << 20
SHAPES = [(65536, 832, 784), (16384, 8192, 8192)]  # rows, padded width, n_out


def _time(fn, n_sets, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(iters):
        fn(i % n_sets)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters  # ms


def _torch_loss(z, t, n_out, loss, coef):
    """The composite: a library loss (sum reduction), its gradient rounded to bf16, and the
    column sums of the rounded gradient."""
    zz, tt = z[:, :n_out], t[:, :n_out].float()
    if loss == "bce":
        total = F.binary_cross_entropy_with_logits(zz, tt, reduction="sum")
        dz = ((torch.sigmoid(zz) - tt) * coef).to(torch.bfloat16)
    else:
        d = zz - tt
        total = (d * d).sum()
        dz = (d * coef).to(torch.bfloat16)
    return total, dz, dz.float().sum(0)


def run(rows, width, n_out, loss, act, iters, rounds):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    set_bytes = rows * width * 8
    n_sets = max(2, -(-3 * CACHE_BYTES // set_bytes))
    sets = []
    for _ in range(n_sets):
        z = torch.randn(rows, width, device=dev, generator=g) * 2
        t = torch.rand(rows, width, device=dev, generator=g).to(torch.bfloat16)
        sets.append((z, t, torch.empty(rows, width, device=dev, dtype=torch.bfloat16)))
    nb, nc = ops.dense_loss_row_blocks(rows), ops.dense_loss_col_chunks(width)
    lp = torch.zeros(nb * nc, device=dev)
    cs = torch.zeros(nb, width, device=dev)
    scale = 1.0 / rows
    coef = (2.0 if loss == "mse" else 1.0) * scale / n_out

    def ours(k):
        z, t, dz = sets[k]
        ops.dense_loss(z, t, dz, n_out, scale, loss, act, loss_part=lp, colsum=cs)

    def theirs(k):
        z, t, _ = sets[k]
        return _torch_loss(z, t, n_out, loss, coef)

    # same results first (section "When results must not change" of any timing comparison)
    ours(0)
    total, dz_t, cs_t = theirs(0)
    got = float(lp.double().sum()) * n_out
    assert abs(got - float(total)) <= 1e-3 * abs(float(total)), (got, float(total))
    torch.testing.assert_close(sets[0][2][:, :n_out].float(), dz_t.float(), rtol=2 ** -7,
                               atol=1e-4 * coef)
    torch.testing.assert_close(cs.sum(0)[:n_out], cs_t, rtol=1e-2, atol=coef)
    for k in range(n_sets):  # warm-up over every buffer set
        ours(k)
        theirs(k)
    t_ours, t_ref = [], []
    for _ in range(rounds):
        t_ours.append(_time(ours, n_sets, iters))
        t_ref.append(_time(theirs, n_sets, iters))
    elems = rows * n_out
    med = statistics.median(t_ours)
    return {"case": "dense_loss", "loss": loss, "act": act, "rows": rows, "width": width,
            "n_out": n_out, "buffer_sets": n_sets, "set_MiB": round(set_bytes / 2 ** 20, 1),
            "ours_ms_median": round(med, 4), "ours_ms_min": round(min(t_ours), 4),
            "torch_ms_median": round(statistics.median(t_ref), 4),
            "torch_ms_min": round(min(t_ref), 4),
            "ours_TBps_8B_per_elem": round(elems * 8 / med / 1e9, 3),
            "speedup_median": round(statistics.median(t_ref) / med, 2)}


def step_time(rows, iters, rounds):
    """Eager (native-executor) step time of the 784-512-128-512-784 sigmoid / bce autoencoder,
    the targets bound zero-copy to the input batch, rotating over resident batches."""
    dev = torch.device("cuda")
    spec = MLPSpec.from_widths([784, 512, 128, 512, 784], hidden_act="relu", out_act="sigmoid")
    tr = Trainer(spec, micro_batch=rows, num_micro=1, device=dev, optim=OptimConfig(lr=0.05),
                 loss="bce")
    g = torch.Generator(device=dev).manual_seed(1)
    batches = []
    for _ in range(4):
        x = torch.zeros(rows, 832, device=dev, dtype=torch.bfloat16)
        x[:, :784] = torch.rand(rows, 784, device=dev, generator=g).to(torch.bfloat16)
        batches.append(x)

    def step(k):
        tr.set_batch(batches[k], None, zero_copy=True, targets=batches[k])
        tr.step()

    for k in range(4):
        step(k)
    first = tr.loss()
    ts = [_time(step, 4, iters) for _ in range(rounds)]
    tr.flush()
    torch.cuda.synchronize()
    return {"case": "autoencoder_step", "model": spec.describe(), "loss": "bce", "rows": rows,
            "step_ms_median": round(statistics.median(ts), 4), "step_ms_min": round(min(ts), 4),
            "loss_first": first, "loss_last": tr.loss()}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dense_loss_bench needs a GPU: nothing is measured without one")
    for rows, width, n_out in SHAPES:
        for loss, act in (("bce", "sigmoid"), ("mse", "linear")):
            print(json.dumps(run(rows, width, n_out, loss, act, a.iters, a.rounds)), flush=True)
    if not a.no_step:
        print(json.dumps(step_time(65536, a.iters, a.rounds)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
