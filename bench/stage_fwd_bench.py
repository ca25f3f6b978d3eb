"""A whole serving stage per launch against one launch per layer, by the method of
bench/linear_w4a8_bench.py: one ``InferenceStage`` per model holding all of its layers, with

  layers     stage_gemm="layers": ops.linear_fwd per layer + ops.softmax_rows (the default);
  fused      stage_gemm="fused": one ops.stage_fwd (csrc/kernels/stage_fwd.hip), tile chosen by
             the launcher;
  fused_tN   ops.stage_fwd on the same operands with tile N forced (stage_fwd.hpp).

Models mnist-fcnn, pytorch-recipe and notebook (relu hidden layers, softmax last) at buckets of
64 .. 65536 rows. The contenders are timed in alternating rounds, back to back in one job, with
device events around ``--iters`` forwards captured once in a HIP graph and replayed. Per case:
the median over the rounds, each contender's run-to-run spread (max - min over the median), and
a verdict: fused wins / loses only when the gap of the medians exceeds the larger of the two
spreads, otherwise it ties. Bytes (x in, all weights and biases once, probabilities out) and
flops come from the shapes; the rates are those over the median. One JSON line per case, printed
and appended to ``--out``. Past 4096 rows the forwards per timed loop shrink with the rows."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from docker_dist_nn_amd import ops  # noqa: E402
from docker_dist_nn_amd.config import LayerWeights  # noqa: E402
from docker_dist_nn_amd.engine.inference import InferenceStage  # noqa: E402
from docker_dist_nn_amd.models.mlp import NAMED_MODELS  # noqa: E402
from docker_dist_nn_amd.utils.native import native  # noqa: E402

MODELS = ("mnist-fcnn", "pytorch-recipe", "notebook")
BUCKETS = (64, 256, 1024, 4096, 16384, 65536)
OUT_DEFAULT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                           "profiles", "stage_fwd", "stage_fwd_bench.jsonl")


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


def _time(graph, iters, stream):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        s.record()
        graph.replay(stream.cuda_stream)
        e.record()
    stream.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us per forward


def _spread(ts):
    return (max(ts) - min(ts)) / statistics.median(ts)


def stage(name, mode, dev):
    dims = list(NAMED_MODELS[name].widths)
    g = np.random.default_rng(len(dims))
    acts = ["relu"] * (len(dims) - 2) + ["softmax"]
    layers = [LayerWeights(weight=g.standard_normal((n, k)) / np.sqrt(k),
                           bias=g.standard_normal(n) * 0.1, activation=a)
              for k, n, a in zip(dims, dims[1:], acts)]
    return InferenceStage(layers, dev, expected_input=dims[0], stage_gemm=mode)


def run(name, M, iters, rounds, dev):
    st = {m: stage(name, m, dev) for m in ("layers", "fused")}
    pads, n_cls = st["fused"].pads, st["fused"].dims[-1]
    x = torch.randn(M, pads[0], device=dev).to(torch.bfloat16)
    for s in st.values():
        s.buffers(M)["x"].copy_(x)
    assert st["fused"].buffers(M)["fused"] and not st["layers"].buffers(M)["fused"]
    outs = {t: torch.zeros(M, pads[-1], device=dev) for t in range(1, ops.STAGE_FWD_TILES + 1)}
    fns = {"layers": lambda: st["layers"].forward(M), "fused": lambda: st["fused"].forward(M)}
    for t, y in outs.items():
        fns[f"fused_t{t}"] = (lambda t=t, y=y: ops.stage_fwd(
            x, st["fused"].w, st["fused"].b, st["fused"].acts, y, n_cls=n_cls, tile=t))
    # same answers first: every tile bit for bit the fused stage, fused within 1e-3 of layers
    want = st["layers"].forward(M)[:, :n_cls].clone()
    got = st["fused"].forward(M)[:, :n_cls].clone()
    torch.testing.assert_close(got, want, rtol=0, atol=1e-3)
    for f in list(fns.values())[2:]:
        assert torch.equal(f()[:, :n_cls], got)

    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for fn in fns.values():  # warm-up of every shape
            for _ in range(10):
                fn()
    stream.synchronize()
    graphs = {k: _capture(fn, iters, stream) for k, fn in fns.items()}
    ts = {k: [] for k in fns}
    for k in fns:  # first replay uploads the graph: not timed
        _time(graphs[k], iters, stream)
    for _ in range(rounds):
        for k in fns:
            ts[k].append(_time(graphs[k], iters, stream))
    med = {k: statistics.median(t) for k, t in ts.items()}
    params = sum(a * b for a, b in zip(pads, pads[1:]))
    nbytes = 2 * M * pads[0] + 2 * params + 4 * sum(pads[1:]) + 4 * M * n_cls
    flops = 2 * M * params
    res = {"case": "stage_fwd", "model": name, "M": M, "pads": pads, "iters": iters,
           "rounds": rounds, "bytes": nbytes, "flops": flops}
    for k in fns:
        res[f"{k}_us_median"] = round(med[k], 3)
        res[f"{k}_spread"] = round(_spread(ts[k]), 3)
        res[f"{k}_TFLOPs"] = round(flops / med[k] / 1e6, 3)
        res[f"{k}_GBps"] = round(nbytes / med[k] / 1e3, 2)

    def verdict(a, b):  # a against b: the gap must exceed the larger of the two spreads
        gap = max(_spread(ts[a]) * med[a], _spread(ts[b]) * med[b])
        return "wins" if med[b] - med[a] > gap else "loses" if med[a] - med[b] > gap else "ties"

    for k in list(fns)[1:]:
        res[f"{k}_over_layers"] = round(med[k] / med["layers"], 3)
        res[f"{k}_vs_layers"] = verdict(k, "layers")
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--buckets", default=",".join(map(str, BUCKETS)))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=OUT_DEFAULT)
    a = ap.parse_args(argv)
    dev = torch.device("cuda")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for name in a.models.split(","):
            for M in map(int, a.buckets.split(",")):
                iters = max(4, a.iters * 4096 // max(M, 4096))
                line = json.dumps(run(name, M, iters, a.rounds, dev))
                print(line, flush=True)
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
