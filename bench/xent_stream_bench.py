"""Last layer + softmax cross-entropy of a wide classifier: the two ways to run it on the same GPU
in the same process, by the method of bench/linear_stream_bench.py.

  pair     ops.linear_fwd to fp32 logits [M][Np] + ops.softmax_xent (XentHead: 8 bytes of traffic
           and 4 bytes of residency per logit);
  stream   ops.linear_xent_stream (csrc/kernels/xent_stream.hip, StreamXentHead): no logits
           matrix, the last layer's forward computed twice.

Both write the same outputs (bf16 dz, loss and correct partials, bias-gradient partials) and are
checked against each other first. They are timed back to back in alternating rounds with device
events around ``--iters`` calls captured once in a HIP graph and replayed (how the engine runs a
step). Per shape: the median over the rounds, each contender's run-to-run spread (max - min over
the median), the ratio of the medians, a verdict -- "wins" / "loses" only beyond the larger of the
two spreads, else "ties" -- and the bytes of the logits buffer that the stream form does not
allocate. One JSON line per shape, printed and appended to ``--out``."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from docker_dist_nn_amd import ops  # noqa: E402
from docker_dist_nn_amd.utils.native import native  # noqa: E402

SHAPES = [(65536, 1024, 512), (16384, 1024, 1024), (16384, 8192, 1024), (8192, 32768, 512)]
OUT_DEFAULT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                           "profiles", "xent_stream", "xent_stream_bench.jsonl")


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
    return s.elapsed_time(e) / iters * 1e3  # us per call


def _spread(ts):
    return (max(ts) - min(ts)) / statistics.median(ts)


def run(M, Np, Kp, iters, rounds, dev):
    n_cls, nb, scale = Np - 3, ops.xent_blocks(M), 1.0 / M
    g = torch.Generator(device=dev).manual_seed(Np + M)
    x = torch.randn(M, Kp, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(Np, Kp, device=dev, generator=g) / Kp ** 0.5).to(torch.bfloat16)
    bias = torch.randn(Np, device=dev, generator=g)
    labels = torch.randint(0, n_cls, (M,), device=dev, generator=g, dtype=torch.int32)
    labels[::97] = -1
    logits = torch.empty(M, Np, dtype=torch.float32, device=dev)
    outs = {name: dict(dz=torch.empty(M, Np, dtype=torch.bfloat16, device=dev),
                       lp=torch.empty(nb, dtype=torch.float32, device=dev),
                       co=torch.empty(nb, dtype=torch.int32, device=dev),
                       cs=torch.empty(nb, Np, dtype=torch.float32, device=dev))
            for name in ("pair", "stream")}

    def pair():
        o = outs["pair"]
        ops.linear_fwd(x, w, bias, logits, act="linear")
        ops.softmax_xent(logits, labels, o["dz"], n_cls, scale, o["lp"], o["co"], colsum=o["cs"])

    def stream_():
        o = outs["stream"]
        ops.linear_xent_stream(x, w, bias, o["dz"], labels, n_cls, scale, o["lp"], o["co"],
                               colsum=o["cs"])

    fns = {"pair": pair, "stream": stream_}
    for fn in fns.values():
        fn()
    a, b = outs["pair"], outs["stream"]  # same results: one bf16 rounding of dz, fp32 sums
    torch.testing.assert_close(b["dz"].float(), a["dz"].float(), rtol=2.0 ** -7, atol=scale * 1e-4)
    torch.testing.assert_close(b["lp"], a["lp"], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(b["cs"], a["cs"], rtol=0, atol=64 * scale * 2.0 ** -8)
    assert int((b["co"] - a["co"]).abs().sum()) <= max(2, M // 4096), "correct counts differ"

    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for fn in fns.values():
            for _ in range(3):
                fn()
    stream.synchronize()
    graphs = {name: _capture(fn, iters, stream) for name, fn in fns.items()}
    ts = {name: [] for name in fns}
    for name in fns:  # first replay uploads the graph: not timed
        _time(graphs[name], iters, stream)
    for _ in range(rounds):
        for name in fns:
            ts[name].append(_time(graphs[name], iters, stream))
    med = {name: statistics.median(t) for name, t in ts.items()}
    margin = max(_spread(ts[n]) * med[n] for n in fns)
    res = {"case": "xent_stream", "M": M, "Np": Np, "Kp": Kp, "n_cls": n_cls, "iters": iters,
           "rounds": rounds, "logits_bytes_not_allocated": M * Np * 4}
    for name in fns:
        res[f"{name}_us_median"] = round(med[name], 2)
        res[f"{name}_us_min"] = round(min(ts[name]), 2)
        res[f"{name}_spread"] = round(_spread(ts[name]), 3)
    res["stream_over_pair"] = round(med["stream"] / med["pair"], 3)
    res["stream_vs_pair"] = "wins" if med["pair"] - med["stream"] > margin else \
        "loses" if med["stream"] - med["pair"] > margin else "ties"
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=0,
                    help="calls per timed replay (default: 3 .. 50 by the shape's size)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", type=str, default="",
                    help="MxNpxKp, comma-separated (default: the four shapes of the README)")
    ap.add_argument("--out", type=str, default=OUT_DEFAULT)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("xent_stream_bench needs a GPU: nothing is measured without one")
    shapes = [tuple(map(int, s.split("x"))) for s in a.shapes.split(",") if s] or SHAPES
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    dev = torch.device("cuda")
    with open(a.out, "a") as f:
        for M, Np, Kp in shapes:
            iters = a.iters or max(3, min(50, (1 << 35) // (M * Np * Kp)))
            line = json.dumps(run(M, Np, Kp, iters, a.rounds, dev))
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
