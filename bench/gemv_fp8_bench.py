"""Serving GEMV micro-benchmark: ops.gemv (bf16 weight rows, csrc/kernels/gemv.hip) against
ops.gemv_fp8 (e4m3 weight rows + one scale per row, csrc/kernels/gemv_fp8.hip) at 1 and 8 input
rows, on the same GPU in the same process. One JSON line per case.

Two layer sizes: 1024 x 1024 on ONE weight buffer (2 MiB / 1 MiB: cache-resident, the time is
launch and latency) and 8192 x 8192 (128 MiB / 64 MiB), where each contender rotates through
enough distinct weight buffers (>= 3 x the 256-MiB Infinity Cache in total) that no call can
find its weights in a cache: the cold, large-layer case in which the weight bytes are the
time. The contenders are timed in alternating rounds with device events around ``--iters``
calls (a few milliseconds at least), in two forms: the calls captured once in a HIP graph and
replayed (the headline figures: how the engine serves, and no host work between kernels) and
the same calls launched from Python (``*_eager_*``: at small layers that loop is bound by the
host's ~8 us per launch, not by the kernel). The median over the rounds, the ratio of the
medians and each contender's run-to-run spread (max - min over the median) are reported, with
the effective weight bytes/s of the replayed form."""
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


def _time(fn, n_sets, iters, stream, graph=None):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        s.record()
        if graph is not None:
            graph.replay(stream.cuda_stream)
        else:
            for i in range(iters):
                fn(i % n_sets)
        e.record()
    stream.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us per call


def _spread(ts):
    return (max(ts) - min(ts)) / statistics.median(ts)


def run(N, K, cold, M, iters, rounds):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(N + M)
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
    x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
    bias = torch.randn(N, device=dev, generator=g)
    y = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    y8 = torch.empty(M, N, dtype=torch.bfloat16, device=dev)

    def bf16(k):
        ops.gemv(x, ws[k % n_bf16], bias, y, "relu")

    def fp8(k):
        ops.gemv_fp8(x, qs[k % n_fp8][0], qs[k % n_fp8][1], bias, y8, "relu")

    # same results first: fp8 against fp64 over the decoded codes (first 256 neurons), and
    # against the bf16 layer within the format's 2^-4 per weight
    bf16(0)
    fp8(0)
    q, s = qs[0]
    dec = ref.e4m3_table().to(dev)[q[:256].long()] * s[:256, None].double()
    want = torch.relu(x.double() @ dec.t() + bias[:256].double())
    torch.testing.assert_close(y8[:, :256].double(), want, rtol=2.0 ** -7, atol=1e-3)
    mag = x.float().abs() @ ws[0].float().abs().t()
    assert bool(((y8.float() - y.float()).abs() <= 2.0 ** -3 * mag + 1e-2).all())

    fns = {"bf16": (bf16, n_bf16), "fp8": (fp8, n_fp8)}
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for fn, n in fns.values():  # warm-up over every buffer set
            for k in range(max(n, 10)):
                fn(k)
    stream.synchronize()
    graphs = {name: _capture(fn, n, iters, stream) for name, (fn, n) in fns.items()}
    ts = {name: [] for name in fns}
    eager = {name: [] for name in fns}
    for name, (fn, n) in fns.items():  # first replay uploads the graph: not timed
        _time(fn, n, iters, stream, graphs[name])
    for _ in range(rounds):
        for name, (fn, n) in fns.items():
            ts[name].append(_time(fn, n, iters, stream, graphs[name]))
        for name, (fn, n) in fns.items():
            eager[name].append(_time(fn, n, iters, stream))
    mb, m8 = statistics.median(ts["bf16"]), statistics.median(ts["fp8"])
    eb, e8 = statistics.median(eager["bf16"]), statistics.median(eager["fp8"])
    return {"case": "gemv_fp8_vs_bf16", "M": M, "N": N, "K": K, "cold": cold,
            "weight_buffers_bf16": n_bf16, "weight_buffers_fp8": n_fp8, "iters": iters,
            "rounds": rounds, "bf16_us_median": round(mb, 3), "fp8_us_median": round(m8, 3),
            "bf16_us_min": round(min(ts["bf16"]), 3), "fp8_us_min": round(min(ts["fp8"]), 3),
            "fp8_over_bf16": round(m8 / mb, 3),
            "bf16_spread": round(_spread(ts["bf16"]), 3), "fp8_spread": round(_spread(ts["fp8"]), 3),
            "bf16_weight_TBps": round(N * K * 2 / mb / 1e6, 3),
            "fp8_weight_TBps": round(N * K / m8 / 1e6, 3),
            "bf16_eager_us_median": round(eb, 3), "fp8_eager_us_median": round(e8, 3),
            "fp8_over_bf16_eager": round(e8 / eb, 3),
            "bf16_eager_spread": round(_spread(eager["bf16"]), 3),
            "fp8_eager_spread": round(_spread(eager["fp8"]), 3)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iters", type=int, default=0,
                    help="calls per timed loop (default: 2000 cache-resident, 300 cold)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=str, default="1,8", help="input row counts, comma-separated")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemv_fp8_bench needs a GPU: nothing is measured without one")
    for N, K, cold in CASES:
        for M in map(int, a.rows.split(",")):
            iters = a.iters or (300 if cold else 2000)
            print(json.dumps(run(N, K, cold, M, iters, a.rounds)), flush=True)
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
