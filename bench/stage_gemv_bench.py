"""A whole serving stage per launch against one launch per layer at 1..8 rows, by the method of
bench/stage_fwd_bench.py: one ``InferenceStage`` per model holding all of its layers, with

  layers     stage_gemv="layers": ops.gemv per layer + ops.softmax_rows (the default);
  fused      stage_gemv="fused": one ops.stage_gemv (csrc/kernels/stage_gemv.hip).

Models mnist-fcnn, pytorch-recipe and notebook (relu hidden layers, softmax last) at 1, 2, 4 and
8 rows. The two are timed in alternating rounds, back to back in one job, two ways:

  replay     device events around ``--iters`` forwards captured once in a HIP graph and replayed;
  eager      a host clock around ``--eager-iters`` forwards launched from Python, ended by a
             stream synchronise (the launches are host-bound: this is the time per request of
             a caller that does not replay).

Per case: the median over the rounds, each contender's run-to-run spread (max - min over the
median), and a verdict per way: fused wins / loses only when the gap of the medians exceeds the
larger of the two spreads, otherwise it ties. The answers are checked equal bit for bit first.
One JSON line per case, printed and appended to ``--out``."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from docker_dist_nn_amd.config import LayerWeights  # noqa: E402
from docker_dist_nn_amd.engine.inference import InferenceStage  # noqa: E402
from docker_dist_nn_amd.models.mlp import NAMED_MODELS  # noqa: E402
from docker_dist_nn_amd.utils.native import native  # noqa: E402

MODELS = ("mnist-fcnn", "pytorch-recipe", "notebook")
ROWS = (1, 2, 4, 8)
OUT_DEFAULT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                           "profiles", "stage_gemv", "stage_gemv_bench.jsonl")


def _capture(fn, iters, stream):
    g = native().GraphExec()
    with torch.cuda.stream(stream):
        g.begin_capture(stream.cuda_stream)
        try:
            for _ in range(iters):
                fn()
        finally:
            g.end_capture()
    return g


def _replay(graph, iters, stream):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        s.record()
        graph.replay(stream.cuda_stream)
        e.record()
    stream.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us per forward


def _eager(fn, iters, stream):
    with torch.cuda.stream(stream):
        stream.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        stream.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6  # us per forward


def _spread(ts):
    return (max(ts) - min(ts)) / statistics.median(ts)


def stage(name, mode, dev):
    dims = list(NAMED_MODELS[name].widths)
    g = np.random.default_rng(len(dims))
    acts = ["relu"] * (len(dims) - 2) + ["softmax"]
    layers = [LayerWeights(weight=g.standard_normal((n, k)) / np.sqrt(k),
                           bias=g.standard_normal(n) * 0.1, activation=a)
              for k, n, a in zip(dims, dims[1:], acts)]
    return InferenceStage(layers, dev, expected_input=dims[0], stage_gemv=mode)


def run(name, M, iters, eager_iters, rounds, dev):
    st = {m: stage(name, m, dev) for m in ("layers", "fused")}
    pads, n_cls = st["fused"].pads, st["fused"].dims[-1]
    x = torch.randn(M, pads[0], device=dev).to(torch.bfloat16)
    for s in st.values():
        s.buffers(M)["x"].copy_(x)
    assert st["fused"].buffers(M)["gemv_fused"] and not st["layers"].buffers(M)["gemv_fused"]
    fns = {"layers": lambda: st["layers"].forward(M), "fused": lambda: st["fused"].forward(M)}
    # same answers first: the fused stage is bit for bit the per-layer one
    assert torch.equal(fns["fused"]()[:, :n_cls], fns["layers"]()[:, :n_cls])

    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for fn in fns.values():  # warm-up
            for _ in range(20):
                fn()
    stream.synchronize()
    graphs = {k: _capture(fn, iters, stream) for k, fn in fns.items()}
    ts = {(k, way): [] for k in fns for way in ("replay", "eager")}
    for k in fns:  # first replay uploads the graph: not timed
        _replay(graphs[k], iters, stream)
    for _ in range(rounds):
        for k in fns:
            ts[k, "replay"].append(_replay(graphs[k], iters, stream))
        for k in fns:
            ts[k, "eager"].append(_eager(fns[k], eager_iters, stream))
    assert torch.equal(fns["fused"]()[:, :n_cls], fns["layers"]()[:, :n_cls])
    med = {k: statistics.median(t) for k, t in ts.items()}
    params = sum(a * b for a, b in zip(pads, pads[1:]))
    res = {"case": "stage_gemv", "model": name, "M": M, "pads": pads, "iters": iters,
           "eager_iters": eager_iters, "rounds": rounds,
           "bytes": 2 * M * pads[0] + 2 * params + 4 * sum(pads[1:]) + 4 * M * n_cls,
           "launches_layers": len(pads), "launches_fused": 1}
    for way in ("replay", "eager"):
        a, b = ("fused", way), ("layers", way)
        for k in (a, b):
            res[f"{k[0]}_{way}_us_median"] = round(med[k], 3)
            res[f"{k[0]}_{way}_spread"] = round(_spread(ts[k]), 3)
        gap = max(_spread(ts[a]) * med[a], _spread(ts[b]) * med[b])
        res[f"fused_over_layers_{way}"] = round(med[a] / med[b], 3)
        res[f"fused_vs_layers_{way}"] = ("wins" if med[b] - med[a] > gap else
                                         "loses" if med[a] - med[b] > gap else "ties")
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--rows", default=",".join(map(str, ROWS)))
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--eager-iters", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=OUT_DEFAULT)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("stage_gemv_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for name in a.models.split(","):
            for M in map(int, a.rows.split(",")):
                line = json.dumps(run(name, M, a.iters, a.eager_iters, a.rounds, dev))
                print(line, flush=True)
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
