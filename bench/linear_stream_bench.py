"""bf16 forward layer at serving buckets of 64 .. 4096 rows: the ways to run one layer on the same
GPU in the same process, by the method of bench/linear_fp8_bench.py.

  tiled    ops.linear_fwd on bf16 weights (the training GEMM; --bf16-gemm tiled, the default);
  stream   ops.linear_fwd_stream on the same weights (csrc/kernels/linear_stream.hip;
           --bf16-gemm stream);
  fp8      ops.linear_fwd_fp8 on the e4m3 codes of those weights (csrc/kernels/linear_fp8.hip;
           --weights fp8 --fp8-gemm direct): the structure's precedent, at half the bytes.

Two layers: 1024 x 1024 on ONE weight buffer (cache-resident: launch and latency) and 8192 x
8192, where each contender rotates through enough distinct weight buffers (>= 3 x the 256-MiB
Infinity Cache in total) that no call finds its weights in a cache. The contenders are timed back
to back in alternating rounds with device events around ``--iters`` calls captured once in a HIP
graph and replayed (how the engine serves; no host work between kernels). Per case: the median
over the rounds, each contender's run-to-run spread (max - min over the median), the ratios of
the medians, the effective weight bytes/s, and a verdict per pair: "wins" / "loses" only beyond
the larger of the two spreads, else "ties". One JSON line per case, printed and appended to
``--out``. ``--tiles 1,2,3`` adds stream contenders with a forced tile (linear_stream.hpp) next to
the launcher's choice."""
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

CACHE_BYTES = 256 << 20
CASES = [(1024, 1024, False), (8192, 8192, True)]  # N, K, cold
OUT_DEFAULT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                           "profiles", "linear_stream", "linear_stream_bench.jsonl")


def _capture(fn, n_sets, iters, stream):
    """``iters`` calls (rotating through the buffer sets) as one HIP graph."""
    g = native().GraphExec()
    with torch.cuda.stream(stream):
        g.begin_capture(stream.cuda_stream)
        try:
            for i in range(iters):
                fn(i % n_sets)
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


def layer(N, K, cold, dev):
    """The weight sets: bf16, and the e4m3 codes + row scales of the same weights (cycled)."""
    g = torch.Generator(device=dev).manual_seed(N)
    n_bf16 = max(1, -(-3 * CACHE_BYTES // (N * K * 2))) if cold else 1
    n_fp8 = max(1, -(-3 * CACHE_BYTES // (N * K))) if cold else 1
    ws = [(torch.randn(N, K, device=dev, generator=g) / K ** 0.5).to(torch.bfloat16)
          for _ in range(n_bf16)]
    qs = []
    for k in range(n_fp8):
        q = torch.empty(N, K, dtype=torch.uint8, device=dev)
        s = torch.empty(N, dtype=torch.float32, device=dev)
        ops.quant_rows_fp8(ws[k % n_bf16], q, s)
        qs.append((q, s))
    return ws, qs


def run(N, K, cold, M, ws, qs, iters, rounds, tiles):
    dev = ws[0].device
    n_bf16, n_fp8 = len(ws), len(qs)
    g = torch.Generator(device=dev).manual_seed(N + M)
    x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
    bias = torch.randn(N, device=dev, generator=g)
    ys = {}

    def out(name):
        ys[name] = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        return ys[name]

    def make_stream(tile, y):
        return lambda k: ops.linear_fwd_stream(x, ws[k % n_bf16], bias, y, "relu", tile=tile)

    yt, y8 = out("tiled"), out("fp8")
    fns = {"tiled": (lambda k: ops.linear_fwd(x, ws[k % n_bf16], bias, yt, act="relu"), n_bf16),
           "fp8": (lambda k: ops.linear_fwd_fp8(x, qs[k % n_fp8][0], qs[k % n_fp8][1], bias, y8,
                                                "relu"), n_fp8),
           "stream": (make_stream(0, out("stream")), n_bf16)}
    for t in tiles:
        fns[f"stream_t{t}"] = (make_stream(t, out(f"stream_t{t}")), n_bf16)

    # same results first (rows up to 1024, first 256 neurons against fp64; every stream
    # contender against the tiled layer everywhere, within one bf16 rounding of the output)
    for fn, _ in fns.values():
        fn(0)
    R = min(M, 1024)
    want = torch.relu(x[:R].double() @ ws[0][:256].double().t() + bias[:256].double())
    for name, y in ys.items():
        if name != "fp8":
            torch.testing.assert_close(y[:R, :256].double(), want, rtol=2.0 ** -7, atol=1e-3)
            torch.testing.assert_close(y.float(), yt.float(), rtol=2.0 ** -7, atol=1e-3)
    del want

    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for fn, n in fns.values():  # warm-up over every buffer set
            for k in range(max(n, 10)):
                fn(k)
    stream.synchronize()
    graphs = {name: _capture(fn, n, iters, stream) for name, (fn, n) in fns.items()}
    ts = {name: [] for name in fns}
    for name in fns:  # first replay uploads the graph: not timed
        _time(graphs[name], iters, stream)
    for _ in range(rounds):
        for name in fns:
            ts[name].append(_time(graphs[name], iters, stream))
    med = {name: statistics.median(t) for name, t in ts.items()}
    res = {"case": "linear_stream", "M": M, "N": N, "K": K, "cold": cold,
           "weight_buffers_bf16": n_bf16, "weight_buffers_fp8": n_fp8, "iters": iters,
           "rounds": rounds}
    for name in fns:
        res[f"{name}_us_median"] = round(med[name], 3)
        res[f"{name}_us_min"] = round(min(ts[name]), 3)
        res[f"{name}_spread"] = round(_spread(ts[name]), 3)
        res[f"{name}_weight_TBps"] = round(N * K * (1 if name == "fp8" else 2) / med[name] / 1e6,
                                           3)

    def verdict(a, b):  # a against b: beyond the larger of the two spreads, or a tie
        margin = max(_spread(ts[a]) * med[a], _spread(ts[b]) * med[b])
        return "wins" if med[b] - med[a] > margin else "loses" if med[a] - med[b] > margin \
            else "ties"

    for other in ("tiled", "fp8"):
        res[f"stream_over_{other}"] = round(med["stream"] / med[other], 3)
        res[f"stream_vs_{other}"] = verdict("stream", other)
    for t in tiles:
        res[f"stream_t{t}_vs_stream"] = verdict(f"stream_t{t}", "stream")
    res["max_spread"] = round(max(_spread(t) for t in ts.values()), 3)
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=0,
                    help="calls per timed loop (default: 1000 cache-resident, 120 cold)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=str, default="64,128,256,512,1024,2048,4096",
                    help="input row counts, comma-separated")
    ap.add_argument("--tiles", type=str, default="",
                    help="forced stream tiles to add, e.g. 1,2,3")
    ap.add_argument("--out", type=str, default=OUT_DEFAULT)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("linear_stream_bench needs a GPU: nothing is measured without one")
    tiles = [int(t) for t in a.tiles.split(",") if t]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    dev = torch.device("cuda")
    with open(a.out, "a") as f:
        for N, K, cold in CASES:
            ws, qs = layer(N, K, cold, dev)
            for M in map(int, a.rows.split(",")):
                iters = a.iters or max(8, (120 if cold else 1000) * 1024 // max(M, 1024))
                line = json.dumps(run(N, K, cold, M, ws, qs, iters, a.rounds, tiles))
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
            del ws, qs
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
