"""Serving GEMV micro-benchmark over three weight formats: ops.gemv (bf16 rows, gemv.hip),
ops.gemv_fp8 (e4m3 rows + one scale per row, gemv_fp8.hip) and ops.gemv_mxfp4 (e2m1 codes + one
e8m0 scale per 32 columns, gemv_mxfp4.hip) at 1, 2, 4 and 8 input rows, back to back on the same
GPU in the same process; and ops.dequant_rows_mxfp4 alone, which is what a bucket of more than 8
rows pays per layer on top of the bf16 GEMM. One JSON line per case, also appended to ``--out``.

The method is bench/gemv_fp8_bench.py's. Two layer sizes: 1024 x 1024 on ONE weight buffer
(cache-resident: the time is launch and latency) and 8192 x 8192, where each contender rotates
through enough distinct weight buffers (>= 3 x the 256-MiB Infinity Cache in total) that no call
can find its weights in a cache: the cold, large-layer case in which the weight bytes are the
time (2, 1 and 17/32 bytes per weight). The contenders are timed in alternating rounds with
device events around ``--iters`` calls captured once in a HIP graph and replayed (how the
engine serves; no host work between kernels). Reported: the median over the rounds, each
contender's run-to-run spread (max - min over the median), the ratios of the medians and the
effective weight bytes/s."""
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
BYTES_PER_WEIGHT = {"bf16": 2.0, "fp8": 1.0, "mxfp4": 17.0 / 32.0}


def _capture(fn, iters, stream):
    """``iters`` calls (each given its index, to rotate buffer sets) as one HIP graph."""
    g = native().GraphExec()
    with torch.cuda.stream(stream):
        g.begin_capture(stream.cuda_stream)
        try:
            for i in range(iters):
                fn(i)
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


def _sets(cold, nbytes):
    return max(1, -(-3 * CACHE_BYTES // int(nbytes))) if cold else 1


def _alternate(fns, iters, rounds, stream):
    """{name: [us per call, one per round]}: warm-up, capture, one untimed replay (the graph's
    upload), then ``rounds`` rounds that time every contender once, in turn."""
    with torch.cuda.stream(stream):
        for fn in fns.values():
            for k in range(32):
                fn(k)
    stream.synchronize()
    graphs = {name: _capture(fn, iters, stream) for name, fn in fns.items()}
    for name in fns:
        _time(graphs[name], iters, stream)
    ts = {name: [] for name in fns}
    for _ in range(rounds):
        for name in fns:
            ts[name].append(_time(graphs[name], iters, stream))
    return ts


def make_layer(N, K, cold, dev, seed):
    """bf16 / fp8 / mxfp4 weight-buffer sets of one N x K layer (the quantised sets cycle
    through the bf16 ones)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    n = {f: _sets(cold, N * K * b) for f, b in BYTES_PER_WEIGHT.items()}
    ws = [(torch.randn(N, K, device=dev, generator=g) / K ** 0.5).to(torch.bfloat16)
          for _ in range(n["bf16"])]
    q8, q4 = [], []
    for k in range(n["fp8"]):
        q = torch.empty(N, K, dtype=torch.uint8, device=dev)
        s = torch.empty(N, dtype=torch.float32, device=dev)
        ops.quant_rows_fp8(ws[k % len(ws)], q, s)
        q8.append((q, s))
    for k in range(n["mxfp4"]):
        q = torch.empty(N, K // 2, dtype=torch.uint8, device=dev)
        e = torch.empty(N, K // 32, dtype=torch.uint8, device=dev)
        ops.quant_rows_mxfp4(ws[k % len(ws)], q, e)
        q4.append((q, e))
    return ws, q8, q4


def run_gemv(layer, N, K, cold, M, iters, rounds):
    ws, q8, q4 = layer
    dev = ws[0].device
    g = torch.Generator(device=dev).manual_seed(N + M)
    x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
    bias = torch.randn(N, device=dev, generator=g)
    y = {f: torch.empty(M, N, dtype=torch.bfloat16, device=dev) for f in BYTES_PER_WEIGHT}
    fns = {"bf16": lambda k: ops.gemv(x, ws[k % len(ws)], bias, y["bf16"], "relu"),
           "fp8": lambda k: ops.gemv_fp8(x, *q8[k % len(q8)], bias, y["fp8"], "relu"),
           "mxfp4": lambda k: ops.gemv_mxfp4(x, *q4[k % len(q4)], bias, y["mxfp4"], "relu")}
    # same results first: mxfp4 against fp64 over the decoded codes (first 256 neurons), and
    # against the bf16 layer within the format's quarter of a weight or of a block's scale
    for fn in fns.values():
        fn(0)
    q, e = q4[0]
    dec = ref.mxfp4_values(q[:256].cpu(), e[:256].cpu(), 256, K).to(dev)
    want = torch.relu(x.double() @ dec.t() + bias[:256].double())
    torch.testing.assert_close(y["mxfp4"][:, :256].double(), want, rtol=2.0 ** -7, atol=1e-3)
    amax = ws[0].float().abs().view(N, K // 32, 32).amax(2).repeat_interleave(32, dim=1)
    fmt = torch.maximum(ws[0].float().abs() / 4, amax / 16)  # scale / 4 <= amax / 16
    assert bool(((y["mxfp4"].float() - y["bf16"].float()).abs()
                 <= x.float().abs() @ fmt.t() + 2.0 ** -4).all())  # + bf16 outputs
    ts = _alternate(fns, iters, rounds, torch.cuda.Stream(dev))
    med = {f: statistics.median(t) for f, t in ts.items()}
    out = {"case": "gemv_mxfp4_vs_fp8_vs_bf16", "M": M, "N": N, "K": K, "cold": cold,
           "iters": iters, "rounds": rounds}
    for f in fns:
        out[f"weight_buffers_{f}"] = len({"bf16": ws, "fp8": q8, "mxfp4": q4}[f])
        out[f"{f}_us_median"] = round(med[f], 3)
        out[f"{f}_us_min"] = round(min(ts[f]), 3)
        out[f"{f}_spread"] = round(_spread(ts[f]), 3)
        out[f"{f}_weight_TBps"] = round(N * K * BYTES_PER_WEIGHT[f] / med[f] / 1e6, 3)
    out["mxfp4_over_fp8"] = round(med["mxfp4"] / med["fp8"], 3)
    out["mxfp4_over_bf16"] = round(med["mxfp4"] / med["bf16"], 3)
    out["fp8_over_bf16"] = round(med["fp8"] / med["bf16"], 3)
    return out


def run_dequant(layer, N, K, cold, iters, rounds):
    """ops.dequant_rows_mxfp4 of one layer into ONE bf16 scratch (as the stage does), against
    ops.dequant_rows_fp8 into the same scratch."""
    ws, q8, q4 = layer
    dev = ws[0].device
    w = torch.empty(N, K, dtype=torch.bfloat16, device=dev)
    fns = {"fp8": lambda k: ops.dequant_rows_fp8(*q8[k % len(q8)], w),
           "mxfp4": lambda k: ops.dequant_rows_mxfp4(*q4[k % len(q4)], w)}
    fns["mxfp4"](0)
    q, e = q4[0]
    assert torch.equal(w[:64].cpu().double(), ref.mxfp4_values(q[:64].cpu(), e[:64].cpu(), 64, K))
    ts = _alternate(fns, iters, rounds, torch.cuda.Stream(dev))
    out = {"case": "dequant_rows_mxfp4_vs_fp8", "N": N, "K": K, "cold": cold, "iters": iters,
           "rounds": rounds}
    for f in fns:
        med = statistics.median(ts[f])
        out[f"{f}_us_median"] = round(med, 3)
        out[f"{f}_us_min"] = round(min(ts[f]), 3)
        out[f"{f}_spread"] = round(_spread(ts[f]), 3)
        # bytes moved: the codes and scales read, the bf16 layer written
        out[f"{f}_moved_TBps"] = round(N * K * (BYTES_PER_WEIGHT[f] + 2.0) / med / 1e6, 3)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=0,
                    help="calls per timed loop (default: 2000 cache-resident, 300 cold)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=str, default="1,2,4,8", help="input row counts")
    ap.add_argument("--out", type=str, default=None, help="also append the JSON lines here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemv_mxfp4_bench needs a GPU: nothing is measured without one")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    dev = torch.device("cuda")
    for N, K, cold in CASES:
        iters = a.iters or (300 if cold else 2000)
        layer = make_layer(N, K, cold, dev, seed=N)
        for M in map(int, a.rows.split(",")):
            emit(run_gemv(layer, N, K, cold, M, iters, a.rounds))
        emit(run_dequant(layer, N, K, cold, iters, a.rounds))
        del layer
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
