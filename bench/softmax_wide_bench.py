"""Wide softmax micro-benchmark: ops.softmax_xent and ops.softmax_rows beyond 256 columns
(csrc/kernels/softmax_wide.hip) against (a) the same results written as torch eager ops and
(b) ops.dense_loss bce at the same rows x width, on the same GPU in the same process. One JSON
line per case.

Every contender works on the next of several buffer sets that together exceed the 256-MiB
Infinity Cache, so each call starts from HBM. The contenders are timed in alternating rounds
with device events; median and minimum over the rounds are reported. Effective bytes/s of the
cross-entropy counts 6 B per element (4 B logit read, 2 B dz written; the kernel's second and
third sweep of a row block are not counted: they are the price of the algorithm, not useful
traffic), of dense_loss 8 B (it also reads a 2-B target), of softmax_rows 8 B (4 read, 4
written). Run one shape per process (``--shape``) so that each gets its own time limit."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from docker_dist_nn_amd import ops  # noqa: E402

CACHE_BYTES = 256 << 20
SHAPES = [(65536, 1024, 1000), (16384, 8192, 8192), (16384, 32768, 32768)]  # rows, width, n_cls


def _time(fn, n_sets, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(iters):
        fn(i % n_sets)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters  # ms


def _rounds(fns, n_sets, iters, rounds):
    """Alternating rounds over the contenders; returns {name: [ms per round]}."""
    for k in range(n_sets):  # warm-up over every buffer set
        for fn in fns.values():
            fn(k)
    out = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            out[name].append(_time(fn, n_sets, iters))
    return out


def _torch_xent(z, labels, n_cls, scale):
    """The composite: a library loss (sum reduction), softmax - onehot rounded to bf16, and the
    column sums of the rounded gradient."""
    zz = z[:, :n_cls]
    total = F.cross_entropy(zz, labels, reduction="sum")
    p = torch.softmax(zz, 1)
    p[torch.arange(z.shape[0], device=z.device), labels] -= 1.0
    dz = (p * scale).to(torch.bfloat16)
    return total, dz, dz.float().sum(0)


def run_xent(rows, width, n_cls, iters, rounds):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    set_bytes = rows * width * 8  # logits + dz + the dense-loss target
    n_sets = max(2, -(-3 * CACHE_BYTES // set_bytes))
    sets = []
    for _ in range(n_sets):
        z = torch.randn(rows, width, device=dev, generator=g) * 2
        t = torch.rand(rows, width, device=dev, generator=g).to(torch.bfloat16)
        lab = torch.randint(0, n_cls, (rows,), device=dev, generator=g, dtype=torch.int32)
        sets.append((z, t, lab, lab.long(),
                     torch.empty(rows, width, device=dev, dtype=torch.bfloat16)))
    nb = ops.xent_blocks(rows)
    lp = torch.zeros(nb, device=dev)
    co = torch.zeros(nb, device=dev, dtype=torch.int32)
    cs = torch.zeros(nb, width, device=dev)
    dense = width % 64 == 0
    lpd = torch.zeros(nb * ops.dense_loss_col_chunks(width), device=dev)
    scale = 1.0 / rows

    def ours(k):
        z, _, lab, _, dz = sets[k]
        ops.softmax_xent(z, lab, dz, n_cls, scale, lp, co, colsum=cs)

    def theirs(k):
        z, _, _, lab64, _ = sets[k]
        return _torch_xent(z, lab64, n_cls, scale)

    def dense_bce(k):
        z, t, _, _, dz = sets[k]
        ops.dense_loss(z, t, dz, n_cls, scale, "bce", "sigmoid", loss_part=lpd, colsum=cs)

    # same results first (section "When results must not change" of any timing comparison)
    ours(0)
    total, dz_t, cs_t = theirs(0)
    got = float(lp.double().sum())
    assert abs(got - float(total)) <= 1e-4 * abs(float(total)), (got, float(total))
    torch.testing.assert_close(sets[0][4][:, :n_cls].float(), dz_t.float(), rtol=2 ** -7,
                               atol=1e-4 * scale)
    torch.testing.assert_close(cs.sum(0)[:n_cls], cs_t, rtol=1e-2, atol=scale)
    assert int(co.sum()) == int((torch.argmax(sets[0][0][:, :n_cls], 1) == sets[0][3]).sum())
    fns = {"ours": ours, "torch": theirs}
    if dense:
        fns["dense_bce"] = dense_bce
    ts = _rounds(fns, n_sets, iters, rounds)
    elems = rows * n_cls
    med = statistics.median(ts["ours"])
    rep = {"case": "softmax_xent", "rows": rows, "width": width, "n_cls": n_cls,
           "buffer_sets": n_sets, "set_MiB": round(set_bytes / 2 ** 20, 1), "iters": iters,
           "rounds": rounds, "ours_ms_median": round(med, 4),
           "ours_ms_min": round(min(ts["ours"]), 4),
           "torch_ms_median": round(statistics.median(ts["torch"]), 4),
           "torch_ms_min": round(min(ts["torch"]), 4),
           "ours_TBps_6B_per_elem": round(elems * 6 / med / 1e9, 3),
           "speedup_vs_torch_median": round(statistics.median(ts["torch"]) / med, 2)}
    if dense:
        dmed = statistics.median(ts["dense_bce"])
        rep.update(dense_bce_ms_median=round(dmed, 4),
                   dense_bce_ms_min=round(min(ts["dense_bce"]), 4),
                   dense_bce_TBps_8B_per_elem=round(elems * 8 / dmed / 1e9, 3),
                   ours_over_dense_bce_median=round(med / dmed, 2))
    return rep


def run_rows(rows, width, n_cls, iters, rounds):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    set_bytes = rows * width * 8  # logits + probabilities
    n_sets = max(2, -(-3 * CACHE_BYTES // set_bytes))
    sets = []
    for _ in range(n_sets):
        z = torch.randn(rows, width, device=dev, generator=g) * 2
        lab = torch.randint(0, n_cls, (rows,), device=dev, generator=g, dtype=torch.int32)
        sets.append((z, lab, lab.long(), torch.empty(rows, width, device=dev)))
    pred = torch.zeros(rows, device=dev, dtype=torch.int32)
    co = torch.zeros(1, device=dev, dtype=torch.int32)

    def ours(k):
        z, lab, _, out = sets[k]
        ops.softmax_rows(z, out, n_cls, lab, pred, co)

    def theirs(k):
        z, _, lab64, _ = sets[k]
        zz = z[:, :n_cls]
        p = torch.softmax(zz, 1)
        am = torch.argmax(zz, 1)
        return p, am, (am == lab64).sum()

    ours(0)
    p, am, hits = theirs(0)
    torch.testing.assert_close(sets[0][3][:, :n_cls], p, rtol=1e-5, atol=1e-7)
    assert torch.equal(pred.long(), am) and int(co[0]) == int(hits)
    ts = _rounds({"ours": ours, "torch": theirs}, n_sets, iters, rounds)
    med = statistics.median(ts["ours"])
    return {"case": "softmax_rows", "rows": rows, "width": width, "n_cls": n_cls,
            "buffer_sets": n_sets, "set_MiB": round(set_bytes / 2 ** 20, 1), "iters": iters,
            "rounds": rounds, "ours_ms_median": round(med, 4),
            "ours_ms_min": round(min(ts["ours"]), 4),
            "torch_ms_median": round(statistics.median(ts["torch"]), 4),
            "torch_ms_min": round(min(ts["torch"]), 4),
            "ours_TBps_8B_per_elem": round(rows * n_cls * 8 / med / 1e9, 3),
            "speedup_vs_torch_median": round(statistics.median(ts["torch"]) / med, 2)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shape", type=int, default=-1,
                    help=f"index into {SHAPES} (rows, width, n_cls); default: all")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("softmax_wide_bench needs a GPU: nothing is measured without one")
    for rows, width, n_cls in (SHAPES if a.shape < 0 else [SHAPES[a.shape]]):
        print(json.dumps(run_xent(rows, width, n_cls, a.iters, a.rounds)), flush=True)
        torch.cuda.empty_cache()
        print(json.dumps(run_rows(rows, width, n_cls, a.iters, a.rounds)), flush=True)
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
