"""MXFP4-weight forward layer at serving buckets of 64 .. 16384 rows: the ways to run one layer
on the same GPU in the same process, by the method of bench/linear_fp8_bench.py.

  bf16       ops.linear_fwd on bf16 weights (what --weights bf16 serves with);
  scratch    ops.dequant_rows_mxfp4 of the whole layer into a bf16 buffer + ops.linear_fwd on it
             (--weights mxfp4 --mxfp4-gemm scratch, the default);
  w8a8       ops.linear_fwd_w8a8: ops.quant_rows_fp8 of the rows + ops.linear_w8a8 on fp8 weight
             codes (--weights fp8 --fp8-gemm w8a8);
  w4a8       ops.linear_fwd_w4a8: ops.quant_rows_fp8 of the rows + ops.linear_w4a8 on the mxfp4
             codes and block scales (csrc/kernels/linear_w4a8.hip; --mxfp4-gemm w4a8) -- what a
             layer costs;
  w4a8_gemm  ops.linear_w4a8 alone, on rows quantised beforehand (w8a8_gemm likewise: the two
             MFMA forms side by side without the shared quantiser).

Two layers: 1024 x 1024 on ONE weight buffer (cache-resident: launch and latency) and 8192 x
8192, where each contender rotates through enough distinct weight buffers (>= 3 x the 256-MiB
Infinity Cache in total) that no call finds its weights in a cache. The contenders are timed in
alternating rounds with device events around ``--iters`` calls captured once in a HIP graph and
replayed (how the engine serves; no host work between kernels). Per case: the median over the
rounds, each contender's run-to-run spread (max - min over the median), the ratios of the
medians and the effective weight bytes/s (bytes of the resident weight format per call). A
contender beats another only when the gap of the medians exceeds the larger of the two spreads;
otherwise they tie. One JSON line per case, printed and appended to ``--out``. ``--w4a8-tiles
1,2`` adds w4a8_gemm contenders with a forced tile (linear_w4a8.hpp) to compare against the
launcher's choice. Past 1024 rows the calls per timed loop shrink with the rows and the result
check looks at the first 1024 rows."""
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
WEIGHT_BYTES = {"bf16": 2.0, "scratch": 17 / 32, "w8a8": 1.0, "w4a8": 17 / 32}
OUT_DEFAULT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                           "profiles", "linear_w4a8", "linear_w4a8_bench.jsonl")


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

    def sets(bytes_per_weight):
        return max(1, -(-3 * CACHE_BYTES // int(N * K * bytes_per_weight))) if cold else 1

    n_bf16, n_fp8, n_mx = sets(2), sets(1), sets(17 / 32)
    ws = [(torch.randn(N, K, device=dev, generator=g) / K ** 0.5).to(torch.bfloat16)
          for _ in range(n_bf16)]
    q8, q4 = [], []
    for k in range(n_fp8):  # the quantised sets quantise the bf16 ones (cycled)
        q = torch.empty(N, K, dtype=torch.uint8, device=dev)
        s = torch.empty(N, dtype=torch.float32, device=dev)
        ops.quant_rows_fp8(ws[k % n_bf16], q, s)
        q8.append((q, s))
    for k in range(n_mx):
        q = torch.empty(N, K // 2, dtype=torch.uint8, device=dev)
        e = torch.empty(N, K // 32, dtype=torch.uint8, device=dev)
        ops.quant_rows_mxfp4(ws[k % n_bf16], q, e)
        q4.append((q, e))
    return ws, q8, q4, torch.empty(N, K, dtype=torch.bfloat16, device=dev)


def run(N, K, cold, M, ws, q8, q4, scratch, iters, rounds, w4a8_tiles=()):
    dev = ws[0].device
    n_bf16, n_fp8, n_mx = len(ws), len(q8), len(q4)
    g = torch.Generator(device=dev).manual_seed(N + M)
    x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
    bias = torch.randn(N, device=dev, generator=g)
    ys = {}

    def out(name):
        ys[name] = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        return ys[name]

    xq = torch.empty(M, K, dtype=torch.uint8, device=dev)
    sx = torch.empty(M, dtype=torch.float32, device=dev)
    xq0, sx0 = torch.empty_like(xq), torch.empty_like(sx)  # quantised once, for the GEMMs alone
    ops.quant_rows_fp8(x, xq0, sx0)
    yb, ysc, y8, y8g, y4 = out("bf16"), out("scratch"), out("w8a8"), out("w8a8_gemm"), out("w4a8")

    def bf16(k):
        ops.linear_fwd(x, ws[k % n_bf16], bias, yb, act="relu")

    def scratch_path(k):
        ops.dequant_rows_mxfp4(q4[k % n_mx][0], q4[k % n_mx][1], scratch)
        ops.linear_fwd(x, scratch, bias, ysc, act="relu")

    def w8a8(k):
        ops.linear_fwd_w8a8(x, q8[k % n_fp8][0], q8[k % n_fp8][1], bias, y8, "relu", xq=xq, sx=sx)

    def w8a8_gemm(k):
        ops.linear_w8a8(xq0, sx0, q8[k % n_fp8][0], q8[k % n_fp8][1], bias, y8g, "relu")

    def w4a8(k):
        ops.linear_fwd_w4a8(x, q4[k % n_mx][0], q4[k % n_mx][1], bias, y4, "relu", xq=xq, sx=sx)

    def make_w4a8_gemm(tile, y):
        return lambda k: ops.linear_w4a8(xq0, sx0, q4[k % n_mx][0], q4[k % n_mx][1], bias, y,
                                         "relu", tile=tile)

    fns = {"bf16": (bf16, n_bf16), "scratch": (scratch_path, n_mx), "w8a8": (w8a8, n_fp8),
           "w8a8_gemm": (w8a8_gemm, n_fp8), "w4a8": (w4a8, n_mx),
           "w4a8_gemm": (make_w4a8_gemm(0, out("w4a8_gemm")), n_mx)}
    for t in w4a8_tiles:
        fns[f"w4a8_gemm_t{t}"] = (make_w4a8_gemm(t, out(f"w4a8_gemm_t{t}")), n_mx)

    # same results first (rows up to 1024, first 256 neurons): every w4a8 contender against fp64
    # over the decoded codes of both operands, the scratch path against fp64 over the decoded
    # weights, and both within the formats' per-element bounds of the bf16 layer
    for fn, _ in fns.values():
        fn(0)
    R = min(M, 1024)
    q, e = q4[0]
    dec = ref.mxfp4_values(q[:256].cpu(), e[:256].cpu(), 256, K).to(dev)
    table = ref.e4m3_table().to(dev)
    want4 = torch.relu((table[xq0[:R].long()] * sx0[:R, None].double()) @ dec.t()
                       + bias[:256].double())
    wants = torch.relu(x[:R].double() @ dec.t() + bias[:256].double())
    mag = x[:R].float().abs() @ ws[0].float().abs().t()
    for name, y in ys.items():
        if name.startswith("w4a8"):
            torch.testing.assert_close(y[:R, :256].double(), want4, rtol=2.0 ** -7, atol=1e-3)
        if name == "scratch":
            torch.testing.assert_close(y[:R, :256].double(), wants, rtol=2.0 ** -7, atol=1e-3)
        if name.startswith("w4a8") or name == "scratch":  # a quarter per weight, 2^-4 per x
            assert bool(((y[:R].float() - yb[:R].float()).abs() <= 0.5 * mag + 1e-2).all()), name
    del want4, wants, mag, dec

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
    res = {"case": "linear_w4a8", "M": M, "N": N, "K": K, "cold": cold,
           "weight_buffers_bf16": n_bf16, "weight_buffers_fp8": n_fp8,
           "weight_buffers_mxfp4": n_mx, "iters": iters, "rounds": rounds}
    for name in fns:
        res[f"{name}_us_median"] = round(med[name], 3)
        res[f"{name}_us_min"] = round(min(ts[name]), 3)
        res[f"{name}_spread"] = round(_spread(ts[name]), 3)
        per_weight = WEIGHT_BYTES[name.split("_")[0]]
        res[f"{name}_weight_TBps"] = round(N * K * per_weight / med[name] / 1e6, 3)

    def verdict(a, b):  # a against b: the gap must exceed the larger of the two spreads
        gap = max(_spread(ts[a]) * med[a], _spread(ts[b]) * med[b])
        return "wins" if med[b] - med[a] > gap else "loses" if med[a] - med[b] > gap else "ties"

    for other in ("bf16", "scratch", "w8a8"):
        res[f"w4a8_over_{other}"] = round(med["w4a8"] / med[other], 3)
        res[f"w4a8_vs_{other}"] = verdict("w4a8", other)
    res["w4a8_gemm_over_w8a8_gemm"] = round(med["w4a8_gemm"] / med["w8a8_gemm"], 3)
    res["w4a8_gemm_vs_w8a8_gemm"] = verdict("w4a8_gemm", "w8a8_gemm")
    for t in w4a8_tiles:
        res[f"w4a8_gemm_vs_t{t}"] = verdict("w4a8_gemm", f"w4a8_gemm_t{t}")
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=0,
                    help="calls per timed loop (default: 1000 cache-resident, 120 cold)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=str, default="64,128,256,512,1024,2048,4096,16384",
                    help="input row counts, comma-separated")
    ap.add_argument("--w4a8-tiles", type=str, default="",
                    help="forced w4a8_gemm tiles to add, e.g. 1,2")
    ap.add_argument("--out", type=str, default=OUT_DEFAULT)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("linear_w4a8_bench needs a GPU: nothing is measured without one")
    w4a8_tiles = [int(t) for t in a.w4a8_tiles.split(",") if t]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    dev = torch.device("cuda")
    with open(a.out, "a") as f:
        for N, K, cold in CASES:
            ws, q8, q4, scratch = layer(N, K, cold, dev)
            for M in map(int, a.rows.split(",")):
                iters = a.iters or max(8, (120 if cold else 1000) * 1024 // max(M, 1024))
                line = json.dumps(run(N, K, cold, M, ws, q8, q4, scratch, iters, a.rounds,
                                      w4a8_tiles))
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
            del ws, q8, q4, scratch
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
