"""The weight-streaming bf16 GEMM (csrc/kernels/linear_stream.hip, ops.linear_fwd_stream) and the
engine's bf16_gemm="stream" path on the GPU, against fp64 on the exact-sum operands of
_linear_fp8_cases.py (x integers in [-2, 2], w multiples of 1/4, all bf16 values; its codes and
scales are not used) and the activation oracle _act_oracle.py.

A wave owns 16 neurons; a k-step is 32 columns; a wave keeps 8 k-steps in flight = one trip of its
loop: 256 columns unsplit, 512 2-way, 1024 4-way. ``tile`` = 1 .. 6 forces 64 x 64, 64 x 32 2-way,
64 x 32 4-way, 128 x 128, 128 x 64 2-way, 128 x 32 4-way; 0 is the launcher's choice."""
import numpy as np
import pytest
import torch

import _act_oracle as ao
import _gemv_fp8_cases as gc
import _linear_fp8_cases as lc
from test_gemv_gpu import SIGMOID_F32_MAX_ULP
from test_linear_fp8_gpu import MODELS, _layers
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.engine.inference import InferenceEngine

pytestmark = pytest.mark.gpu

# (M, N, K, tile). Which edge each value hits:
#   M  9 first past the GEMV; 63 / 64 / 65 below, at, past the 64-row tile (65 and 70: a second
#      row tile); 127 / 128 / 129 / 130 below, at, past the 128-row tile (tiles 4 .. 6).
#   N  1; 15 / 16 / 17 around a wave's 16 neurons; 31 / 32 / 33 around the 32-neuron workgroups
#      (tiles 2, 3, 6); 63 / 64 / 65 around the 64-neuron ones (1, 5); 127 / 128 / 129 around
#      tile 4. Where the launcher's rule changes tile: 16385 at 9 rows (257 workgroups of 64 x
#      64: tile 1, below it tile 2), 8193 at 65 rows (258 > 256 workgroups of 64 rows: the
#      128-row tiles, 4-way), 32641 at 65 rows (256 workgroups of 128 x 128: unsplit).
#   K  32 one k-step (every other ring slot past K); 96 one k-step past a 64-column boundary;
#      256 / 288, 512 / 544, 1024 / 1056 the ring depth and one k-step past it for the unsplit,
#      2-way and 4-way tiles; 512 on tile 1 and 2048 / 2080 on the 4-way tiles two trips; 4128.
#      Every tile has a K >= 1024, where every K-split group does real work.
CASES = [
    (9, 1, 32, 0), (63, 15, 96, 0), (64, 16, 256, 0), (65, 17, 1056, 0),
    (9, 16385, 32, 0), (65, 8193, 32, 0), (65, 32641, 32, 0),
    (9, 63, 512, 1), (65, 64, 288, 1), (70, 65, 4128, 1),
    (64, 31, 512, 2), (63, 33, 544, 2), (9, 32, 4128, 2),
    (9, 32, 1024, 3), (65, 33, 2048, 3), (64, 17, 4128, 3),
    (127, 127, 256, 4), (128, 129, 96, 4), (130, 128, 4128, 4),
    (129, 65, 512, 5), (128, 63, 1056, 5),
    (127, 31, 1024, 6), (129, 32, 2080, 6), (130, 33, 4128, 6),
]


def _views(M, N, K, dev):
    """NaN-padded bf16 views (row strides > K) of the exact-sum operands, and the fp64 ones."""
    x, xs, w, _, _, bias = lc.operands(M, N, K)
    _, xv = ao.padded(M, K, torch.bfloat16, float("nan"), dev, x)
    _, xsv = ao.padded(M, K, torch.bfloat16, float("nan"), dev, xs)
    _, wv = ao.padded(N, K, torch.bfloat16, float("nan"), dev, w)
    return x, xs, w, bias, xv, xsv, wv, bias.float().to(dev)  # bias: 5 NaN entries past N


@pytest.mark.parametrize("M,N,K,tile", CASES)
def test_linear_stream_equals_fp64(dev, M, N, K, tile):
    """Every activation, fp32 and bf16 y, bias and None: linear / relu EQUAL fp64 (every partial
    sum is exact), sigmoid within the GEMV's bounds (same act_fwd), padding of y untouched."""
    x, xs, w, bias, xv, xsv, wv, bv = _views(M, N, K, dev)
    worst = 0.0
    for b, bdev in ((bias, bv), (None, None)):
        for act in ao.ACTS:
            xa, xdev = (xs, xsv) if act == "sigmoid" else (x, xv)
            z = xa @ w.t() + (0.0 if b is None else b[:N])
            assert act != "sigmoid" or float(z.abs().max()) <= 68.0
            ref = ao.act_fwd(z, act)
            what = f"linear_stream {M}x{N}x{K} tile {tile} {act} bias={b is not None}"
            for dtype in (torch.float32, torch.bfloat16):
                ybuf, yv = ao.padded(M, N, dtype, ao.SENTINEL, dev)
                ops.linear_fwd_stream(xdev, wv, bdev, yv, act, tile=tile)
                if dtype == torch.bfloat16:
                    ao.assert_bf16_close(yv, ref, 1 if act == "sigmoid" else 0, what)
                elif act == "sigmoid":
                    worst = max(worst, gc.f32_ulps(yv.cpu(), ref))
                else:
                    assert torch.equal(yv.cpu().double(), ref), f"{what}: not the exact sum"
                ao.assert_padding_untouched(ybuf, M, N, what=what)
    assert worst <= SIGMOID_F32_MAX_ULP


def test_linear_stream_random_operands_within_derived_bound(dev):
    """Random bf16 operands against fp64. bf16 products are exact in fp32, so the error is that of
    the additions: K products in one accumulator plus at most 3 cross-group additions, T = K + 3
    (the kernel's header), then the bias add and a spare unit, each at most 2^-24 of the magnitude:
    |y - ref| <= (T + 2) * 2^-24 * (sum_k |x w| + |b|). tile 0 is the 2-way 64 x 32 here, 1 the
    unsplit 64 x 64, 3 the 4-way 64 x 32. A second call is bit-identical."""
    M, N, K = 70, 300, 4128
    g = torch.Generator().manual_seed(K)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    bias = torch.randn(N, generator=g)
    _, xv = ao.padded(M, K, torch.bfloat16, float("nan"), dev, x)
    _, wv = ao.padded(N, K, torch.bfloat16, float("nan"), dev, w)
    x64, w64, b64 = x.double(), w.double(), bias.double()
    ref = x64 @ w64.t() + b64
    T = K + 3
    assert T == 4131
    bound = (T + 2) * 2.0 ** -24 * (x64.abs() @ w64.abs().t() + b64.abs())
    for tile in (0, 1, 3):
        ybuf, yv = ao.padded(M, N, torch.float32, ao.SENTINEL, dev)
        ops.linear_fwd_stream(xv, wv, bias.to(dev), yv, "linear", tile=tile)
        ratio = float(((yv.cpu().double() - ref).abs() / bound).max())
        print(f"\nlinear_stream random 70x300x4128 tile {tile}: error at {ratio:.4f} x the bound")
        assert ratio <= 1.0
        ao.assert_padding_untouched(ybuf, M, N, what="linear_stream random")
        ybuf2, yv2 = ao.padded(M, N, torch.float32, ao.SENTINEL, dev)
        ops.linear_fwd_stream(xv, wv, bias.to(dev), yv2, "linear", tile=tile)
        assert torch.equal(ybuf, ybuf2), "two runs differ"


def test_linear_stream_agrees_with_gemv_at_the_seam(dev):
    """On exact-sum operands: at M = 8 the op IS ops.gemv; at M = 9 (the MFMA kernel) its first 8
    rows equal gemv of those rows bit for bit (both exact, through the same act_fwd)."""
    N, K = 65, 544
    x, xs, w, bias, xv, xsv, wv, bv = _views(9, N, K, dev)
    for act in ao.ACTS:
        xdev = xsv if act == "sigmoid" else xv
        y8, g8, y9 = (torch.zeros(m, N, device=dev) for m in (8, 8, 9))
        ops.gemv(xdev[:8], wv, bv, g8, act)
        ops.linear_fwd_stream(xdev[:8], wv, bv, y8, act)
        ops.linear_fwd_stream(xdev, wv, bv, y9, act)
        assert torch.equal(y8, g8) and torch.equal(y9[:8], g8), act


def test_linear_stream_rejects_bad_operands(dev):
    x = torch.zeros(9, 64, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(4, 64, dtype=torch.bfloat16, device=dev)
    y = torch.zeros(9, 4, device=dev)
    ops.linear_fwd_stream(x, w, None, y)  # fine
    with pytest.raises(ValueError):
        ops.linear_fwd_stream(x[:, :48], w, None, y)  # K % 32
    with pytest.raises(ValueError):  # rows of w not 16-byte aligned
        ops.linear_fwd_stream(x, torch.zeros(4, 68, dtype=torch.bfloat16, device=dev)[:, :64],
                              None, y)
    with pytest.raises(ValueError):
        ops.linear_fwd_stream(x, w, torch.zeros(3, device=dev), y)  # bias shorter than N
    with pytest.raises(TypeError):
        ops.linear_fwd_stream(x, w.float(), None, y)
    with pytest.raises(ValueError):
        ops.linear_fwd_stream(x, w, None, y, tile=ops.LINEAR_STREAM_TILES + 1)


def _engine(acts, dev, split=False, **kw):
    L = _layers(acts)
    return InferenceEngine([L[:1], L[1:]] if split else [L], dev, expected_input=40, **kw)


@pytest.mark.parametrize("mode", ["eager", "graph", "native"])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_engine_stream_buckets_chain_linear_fwd_stream(dev, monkeypatch, model, mode):
    """bf16_gemm="stream": predict at 9, 64 and 65 rows (buckets 64, 64, 128) is bit-equal to
    ops.linear_fwd_stream chained by hand on bucket-padded rows -- eagerly, under HIP-graph
    replay and under native Program replay, twice each; the sigmoid model as two stages."""
    monkeypatch.setenv("DNN_SERVE_REPLAY", "native" if mode == "native" else "graph")
    eng = _engine(MODELS[model], dev, split=model == "sigmoid", use_graphs=mode != "eager",
                  bf16_gemm="stream")
    (w0, b0, a0), (w1, b1, a1) = [(st.w[i], st.b[i], st.acts[i]) for st in eng.stages
                                  for i in range(len(st.layers))]
    for rows, bucket in ((9, 64), (64, 64), (65, 128)):
        x = np.random.default_rng(rows).standard_normal((rows, 40))
        xb = torch.zeros(bucket, 64, dtype=torch.bfloat16, device=dev)
        ops.pack_bf16(torch.from_numpy(x).float().to(dev), xb[:rows])
        h = torch.zeros(bucket, 64, dtype=torch.bfloat16, device=dev)
        f = torch.zeros(bucket, 64, dtype=torch.float32, device=dev)
        ops.linear_fwd_stream(xb, w0, b0, h, a0)
        ops.linear_fwd_stream(h, w1, b1, f, a1)
        want = f[:rows, :10].double().cpu().numpy()
        for _ in range(2):  # capture / record, then replay
            assert np.array_equal(eng.predict(x), want), f"{model} {mode} rows={rows}"


@pytest.mark.parametrize("model", sorted(MODELS))
def test_engine_stream_leaves_other_buckets_alone(dev, model):
    """Requests of 1, 5 and 8 rows (the GEMV) and of 2 * BF16_STREAM_MAX_ROWS rows (linear_fwd)
    equal the default engine bit for bit."""
    stream = _engine(MODELS[model], dev, bf16_gemm="stream")
    default = _engine(MODELS[model], dev)
    for rows in (1, 5, 8, 2 * ops.BF16_STREAM_MAX_ROWS):
        x = np.random.default_rng(rows).standard_normal((rows, 40))
        for _ in range(2):
            assert np.array_equal(stream.predict(x), default.predict(x)), f"rows={rows}"
