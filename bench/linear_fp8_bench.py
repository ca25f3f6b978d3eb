"""fp8-weight forward layer at serving buckets of 64 .. 65536 rows: the ways to run one layer
on the same GPU in the same process, by the method of bench/gemv_fp8_bench.py.

  bf16       ops.linear_fwd on bf16 weights (what --weights bf16 serves with);
  scratch    ops.dequant_rows_fp8 of the whole layer into a bf16 buffer + ops.linear_fwd on it
             (--weights fp8 --fp8-gemm scratch: the yardstick for FP8_DIRECT_MAX_ROWS);
  direct     ops.linear_fwd_fp8 on the codes (csrc/kernels/linear_fp8.hip; --fp8-gemm direct);
  w8a8       ops.linear_fwd_w8a8: ops.quant_rows_fp8 of the rows + ops.linear_w8a8 on codes x
             codes (csrc/kernels/linear_w8a8.hip; --fp8-gemm w8a8) -- what a layer costs;
  w8a8_gemm  ops.linear_w8a8 alone, on rows quantised beforehand.

Two layers: 1024 x 1024 on ONE weight buffer (cache-resident: launch and latency) and 8192 x
8192, where each contender rotates through enough distinct weight buffers (>= 3 x the 256-MiB
Infinity Cache in total) that no call finds its weights in a cache. The contenders are timed in
alternating rounds with device events around ``--iters`` calls captured once in a HIP graph and
replayed (how the engine serves; no host work between kernels). Per case: the median over the
rounds, each contender's run-to-run spread (max - min over the median), the ratios of the
medians and the effective weight bytes/s (bytes of the resident weight format per call). One
JSON line per case, printed and appended to ``--out``. ``--tiles 1,2`` adds direct contenders
with a forced tile (linear_fp8.hpp) and ``--w8a8-tiles 1,2`` w8a8_gemm contenders with a forced
tile (linear_w8a8.hpp) to compare against the launchers' choices. Past 1024 rows the calls per
timed loop shrink with the rows (a call then takes milliseconds) and the result check looks at
the first 1024 rows."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from docker_dist_nn_amd import ops  # noqa: E402
from docker_dist_nn_amd.ops import reference as ref  # noqa: E402
from docker_dist_nn_amd.utils.native import native  # noqa: E402

CACHE_BYTES = 256 << 20
CASES = [(1024, 1024, False), (8192, 8192, True)]  # N, K, cold
OUT_DEFAULT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                           "profiles", "linear_fp8", "linear_fp8_bench.jsonl")


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
    g = torch.Generator(device=dev).manual_seed(N)
    n_bf16 = max(1, -(-3 * CACHE_BYTES // (N * K * 2))) if cold else 1
    n_fp8 = max(1, -(-3 * CACHE_BYTES // (N * K))) if cold else 1
    ws = [(torch.randn(N, K, device=dev, generator=g) / K ** 0.5).to(torch.bfloat16)
          for _ in range(n_bf16)]
    qs = []
    for k in range(n_fp8):  # the fp8 sets quantise the bf16 ones (cycled)
        q = torch.empty(N, K, dtype=torch.uint8, device=dev)
        s = torch.empty(N, dtype=torch.float32, device=dev)
        ops.quant_rows_fp8(ws[k % n_bf16], q, s)
        qs.append((q, s))
    return ws, qs, torch.empty(N, K, dtype=torch.bfloat16, device=dev)


def run(N, K, cold, M, ws, qs, scratch, iters, rounds, tiles, w8a8_tiles=()):
    dev = ws[0].device
    n_bf16, n_fp8 = len(ws), len(qs)
    g = torch.Generator(device=dev).manual_seed(N + M)
    x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
    bias = torch.randn(N, device=dev, generator=g)
    ys = {}

    def out(name):
        ys[name] = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        return ys[name]

    def make_direct(tile, y):
        return lambda k: ops.linear_fwd_fp8(x, qs[k % n_fp8][0], qs[k % n_fp8][1], bias, y,
                                            "relu", tile=tile)

    xq = torch.empty(M, K, dtype=torch.uint8, device=dev)
    sx = torch.empty(M, dtype=torch.float32, device=dev)
    xq0, sx0 = torch.empty_like(xq), torch.empty_like(sx)  # quantised once, for w8a8_gemm
    ops.quant_rows_fp8(x, xq0, sx0)

    def make_w8a8(y):
        return lambda k: ops.linear_fwd_w8a8(x, qs[k % n_fp8][0], qs[k % n_fp8][1], bias, y,
                                             "relu", xq=xq, sx=sx)

    def make_w8a8_gemm(tile, y):
        return lambda k: ops.linear_w8a8(xq0, sx0, qs[k % n_fp8][0], qs[k % n_fp8][1], bias, y,
                                         "relu", tile=tile)

    yb, ysc = out("bf16"), out("scratch")

    def bf16(k):
        ops.linear_fwd(x, ws[k % n_bf16], bias, yb, act="relu")

    def scratch_path(k):
        ops.dequant_rows_fp8(qs[k % n_fp8][0], qs[k % n_fp8][1], scratch)
        ops.linear_fwd(x, scratch, bias, ysc, act="relu")

    fns = {"bf16": (bf16, n_bf16), "scratch": (scratch_path, n_fp8),
           "direct": (make_direct(0, out("direct")), n_fp8)}
    for t in tiles:
        fns[f"direct_t{t}"] = (make_direct(t, out(f"direct_t{t}")), n_fp8)
    fns["w8a8"] = (make_w8a8(out("w8a8")), n_fp8)
    fns["w8a8_gemm"] = (make_w8a8_gemm(0, out("w8a8_gemm")), n_fp8)
    for t in w8a8_tiles:
        fns[f"w8a8_gemm_t{t}"] = (make_w8a8_gemm(t, out(f"w8a8_gemm_t{t}")), n_fp8)

    # same results first (rows up to 1024): direct against fp64 over the decoded codes (first
    # 256 neurons), w8a8 against fp64 over the decoded codes of both operands, and every fp8
    # contender against the bf16 layer within the format's 2^-4 per weight (w8a8: per weight
    # and per activation)
    for fn, _ in fns.values():
        fn(0)
    q, s = qs[0]
    R = min(M, 1024)
    table = ref.e4m3_table().to(dev)
    dec = table[q[:256].long()] * s[:256, None].double()
    want = torch.relu(x[:R].double() @ dec.t() + bias[:256].double())
    want8 = torch.relu((table[xq0[:R].long()] * sx0[:R, None].double()) @ dec.t()
                       + bias[:256].double())
    mag = x[:R].float().abs() @ ws[0].float().abs().t()
    for name, y in ys.items():
        if name.startswith("direct"):
            torch.testing.assert_close(y[:R, :256].double(), want, rtol=2.0 ** -7, atol=1e-3)
        if name.startswith("w8a8"):
            torch.testing.assert_close(y[:R, :256].double(), want8, rtol=2.0 ** -7, atol=1e-3)
        tol = 2.0 ** -2 if name.startswith("w8a8") else 2.0 ** -3
        assert bool(((y[:R].float() - yb[:R].float()).abs() <= tol * mag + 1e-2).all()), name
    del want, want8, mag, dec

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
    res = {"case": "linear_fp8", "M": M, "N": N, "K": K, "cold": cold,
           "weight_buffers_bf16": n_bf16, "weight_buffers_fp8": n_fp8, "iters": iters,
           "rounds": rounds}
    for name in fns:
        res[f"{name}_us_median"] = round(med[name], 3)
        res[f"{name}_us_min"] = round(min(ts[name]), 3)
        res[f"{name}_spread"] = round(_spread(ts[name]), 3)
        res[f"{name}_weight_TBps"] = round(N * K * (2 if name == "bf16" else 1) / med[name] / 1e6,
                                           3)
    def beats(a, b):  # a beats b by more than the larger of the two spreads
        return bool(med[b] - med[a] >
                    max(_spread(ts[a]) * med[a], _spread(ts[b]) * med[b]))

    for other in ("bf16", "scratch", "direct"):
        res[f"w8a8_over_{other}"] = round(med["w8a8"] / med[other], 3)
        res[f"w8a8_beats_{other}"] = beats("w8a8", other)
        res[f"{other}_beats_w8a8"] = beats(other, "w8a8")
    res["w8a8_gemm_over_bf16"] = round(med["w8a8_gemm"] / med["bf16"], 3)
    res["direct_over_scratch"] = round(med["direct"] / med["scratch"], 3)
    res["direct_over_bf16"] = round(med["direct"] / med["bf16"], 3)
    res["scratch_over_bf16"] = round(med["scratch"] / med["bf16"], 3)
    # direct beats scratch by more than the larger of the two spreads (FP8_DIRECT_MAX_ROWS)
    res["direct_beats_scratch"] = bool(
        med["scratch"] - med["direct"] >
        max(_spread(ts["direct"]) * med["direct"], _spread(ts["scratch"]) * med["scratch"]))
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=0,
                    help="calls per timed loop (default: 1000 cache-resident, 120 cold)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=str, default="64,128,256,512,1024,2048,4096,16384,65536",
                    help="input row counts, comma-separated")
    ap.add_argument("--tiles", type=str, default="", help="forced direct tiles to add, e.g. 1,2")
    ap.add_argument("--w8a8-tiles", type=str, default="",
                    help="forced w8a8_gemm tiles to add, e.g. 1,2")
    ap.add_argument("--out", type=str, default=OUT_DEFAULT)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("linear_fp8_bench needs a GPU: nothing is measured without one")
    tiles = [int(t) for t in a.tiles.split(",") if t]
    w8a8_tiles = [int(t) for t in a.w8a8_tiles.split(",") if t]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    dev = torch.device("cuda")
    with open(a.out, "a") as f:
        for N, K, cold in CASES:
            ws, qs, scratch = layer(N, K, cold, dev)
            for M in map(int, a.rows.split(",")):
                iters = a.iters or max(8, (120 if cold else 1000) * 1024 // max(M, 1024))
                line = json.dumps(run(N, K, cold, M, ws, qs, scratch, iters, a.rounds, tiles,
                                      w8a8_tiles))
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
            del ws, qs, scratch
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
