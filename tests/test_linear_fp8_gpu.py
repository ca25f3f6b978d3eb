"""The fp8-weight GEMM (csrc/kernels/linear_fp8.hip, ops.linear_fwd_fp8) and the engine's
fp8_gemm="direct" path on the GPU, against the exact oracles _fp8_oracle.py (the format) and
_act_oracle.py (the activations): operands and method in _linear_fp8_cases.py.

The kernel's constants (linear_fp8.hip): a wave owns 16 neurons; the x tile is BM = 64 rows
(while ceil(N / 64) * ceil(M / 64) <= 256, or M <= 64) or 128; a workgroup takes BN = BM neurons
("wide") when that gives >= 256 workgroups, else BM / 2 with a 2-way K split ("narrow"); a k-step
is 64 columns, an LDS stage 128; 4 stages = 512 columns of x and codes are in flight (one trip
of the unrolled k loop).
``tile`` = 1 .. 4 forces 64 x 64, 64 x 32, 128 x 128, 128 x 64; 0 is the launcher's choice."""
import numpy as np
import pytest
import torch

import _act_oracle as ao
import _fp8_oracle as fo
import _gemv_fp8_cases as gc
import _linear_fp8_cases as lc
from test_gemv_gpu import SIGMOID_F32_MAX_ULP
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.config import LayerWeights
from docker_dist_nn_amd.engine.inference import InferenceEngine

pytestmark = pytest.mark.gpu

# (M, N, K, tile). Which edge each value hits:
#   M  9 first past the GEMV; 63 / 64 / 65 below, at, past the 64-row tile (65: a second row
#      tile with one row); 70 and 130: two and three 64-row tiles; 127 / 128 / 129 / 130 below,
#      at, past the 128-row tile (tiles 3, 4).
#   N  1; 15 / 16 / 17 around a wave's 16 neurons; 31 / 32 / 33 around the narrow 64-row
#      workgroup; 63 / 64 / 65 around the wide 64-row and the narrow 128-row workgroup; 127 /
#      128 / 129 around the wide 128-row workgroup. Where the launcher itself leaves the narrow
#      64-row tile: 16385 at 9 rows (257 workgroups of 64 x 64: wide), 8193 at 65 rows (258 > 256
#      workgroups of 64 rows: 128 x 64), 32641 at 65 rows (256 workgroups of 128 x 128: wide).
#   K  16 (one code load of lane group 0, everything else past K); 48 a k-step cut in the
#      middle; 64 one k-step; 80 one 16-byte step past it; 128 one stage; 144 a step past it;
#      512 / 528 the prefetch depth (one loop trip) and a 16-byte step past it; 1024 / 1040 the
#      same of two trips; 4112 eight trips and a step.
CASES = [
    (9, 1, 16, 0), (63, 15, 64, 0), (64, 16, 80, 0), (64, 32, 128, 0), (65, 17, 48, 0),
    (127, 31, 1040, 0), (128, 33, 144, 0), (130, 65, 4112, 0),
    (9, 16385, 16, 0), (65, 8193, 16, 0), (65, 32641, 16, 0),
    (9, 63, 16, 1), (65, 64, 80, 1), (70, 65, 1040, 1), (9, 17, 4112, 2), (64, 33, 1024, 2),
    (127, 127, 64, 3), (128, 129, 144, 3), (130, 128, 4112, 3), (64, 63, 528, 4),
    (129, 65, 512, 4),
]


@pytest.mark.parametrize("M,N,K,tile", CASES)
def test_linear_fp8_equals_fp64_oracle(dev, M, N, K, tile):
    """Every activation, fp32 and bf16 output, bias and None, NaN-padded x / codes / scale /
    bias: linear and relu EQUAL the fp64 value (every partial sum is exact, so any tile, K split
    and MFMA slot order must give it), sigmoid within the GEMV's bounds, padding of y untouched."""
    worst = lc.check_exact(ops.linear_fwd_fp8, M, N, K, dev, SIGMOID_F32_MAX_ULP, tile=tile)
    print(f"\nlinear_fp8 {M}x{N}x{K} tile {tile}: sigmoid fp32 worst {worst:.2f} ulp (bound "
          f"{SIGMOID_F32_MAX_ULP:g})")


@pytest.mark.parametrize("tile", [0, 1, 3])
def test_linear_fp8_decodes_every_code(dev, tile):
    """q[n][0] = n, x = e_0 in 9 rows (row 0 only), scale 1: y[0][n] is the kernel's decode of
    code n through v_cvt_pk_f32_fp8 + the high-half pack + the MFMA. It equals the oracle's
    table bit for bit for the 254 finite codes and is NaN for 0x7F / 0xFF; rows 1..8 (x = 0)
    are +0 in the finite columns."""
    q = torch.zeros(256, 16, dtype=torch.uint8)
    q[:, 0] = torch.arange(256, dtype=torch.uint8)
    x = torch.zeros(9, 16, dtype=torch.bfloat16)
    x[0, 0] = 1.0
    y = torch.full((9, 256), ao.SENTINEL, dtype=torch.float32, device=dev)
    ops.linear_fwd_fp8(x.to(dev), q.to(dev), torch.ones(256, device=dev), None, y, "linear",
                       tile=tile)
    got = y.cpu().numpy()
    want = fo.DEC.astype(np.float32) + np.float32(0.0)
    finite = np.isfinite(fo.DEC)
    assert finite.sum() == 254 and not finite[0x7F] and not finite[0xFF]
    assert np.array_equal(fo.bits32(got[0][finite]), fo.bits32(want[finite]))
    assert np.isnan(got[0][0x7F]) and np.isnan(got[0][0xFF])
    assert not fo.bits32(got[1:, finite]).any()  # +0: no bit set


def test_linear_fp8_agrees_with_gemv_at_the_seam(dev):
    """On exact-sum operands: at M = 8 ops.linear_fwd_fp8 IS ops.gemv_fp8 (it dispatches to it);
    at M = 9 (the MFMA kernel) its first 8 rows equal gemv_fp8 of those rows bit for bit (both
    are exact, so the format means the same on both sides of the 8 / 9-row line)."""
    N, K = 65, 528
    x, _, _, q, scale, bias = lc.operands(9, N, K)
    xv, qv = x.to(torch.bfloat16).to(dev), q.to(dev)
    sv, bv = scale.float().to(dev), bias.float().to(dev)
    for act in ("linear", "relu", "sigmoid"):
        y8 = torch.zeros(8, N, device=dev)
        g8 = torch.zeros(8, N, device=dev)
        y9 = torch.zeros(9, N, device=dev)
        ops.gemv_fp8(xv[:8], qv, sv, bv, g8, act)
        ops.linear_fwd_fp8(xv[:8], qv, sv, bv, y8, act)
        ops.linear_fwd_fp8(xv, qv, sv, bv, y9, act)
        assert torch.equal(y8, g8), act
        assert torch.equal(y9[:8], g8), act  # exact pre-activations through the same act_fwd


def _random_case(dev):
    M, N, K = 70, 300, 4112
    g = torch.Generator().manual_seed(4112)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    bias = torch.randn(N, generator=g)
    q, s, _ = fo.quant_ref(w)
    _, xv = ao.padded(M, K, torch.bfloat16, float("nan"), dev, x)
    return (M, N, K, x, q, s, bias, xv, gc.padded_codes(torch.from_numpy(q), dev),
            torch.from_numpy(s).to(dev), bias.to(dev))


def test_linear_fp8_random_operands_within_derived_bound(dev):
    """Random bf16 x and quantised random weights at 70 x 300 x 4112 against s * (x . dec(q)^T)
    + bias in fp64. dec * x is exact in fp32 (4 x 8 significant bits), so the error is that of
    the additions and the epilogue. One accumulator element takes 2 MFMAs per 64-column k-step
    (lane group g's codes 0..7 and 8..15), each adding 32 products into it: over the
    ceil(4112 / 64) = 65 k-steps of the longest chain (the wide tile, one wave over all of K)
    that is 2 * 65 * 32 = 4160 additions; the narrow tiles split them over two waves and add
    one cross-wave addition through LDS: T = 4160 + 1 = 4161 covers both. Then the scale
    multiply, the bias add and a spare unit, each at most 2^-24 of the running magnitude
    <= s * sum_k |x_k dec_k| + |bias|:
    |y - ref| <= (T + 3) * 2^-24 * (s * sum_k |x_k dec_k| + |bias|) per output.
    A second call is bit-identical (fixed summation order)."""
    M, N, K, x, q, s, bias, xv, qv, sv, bv = _random_case(dev)
    deq = s.astype(np.float64)[:, None] * fo.DEC[q]
    x64, b64 = x.double().numpy(), bias.double().numpy()
    ref = x64 @ deq.T + b64
    T = 2 * 32 * -(-K // 64) + 1
    assert T == 4161
    bound = (T + 3) * 2.0 ** -24 * (np.abs(x64) @ np.abs(deq).T + np.abs(b64))
    for tile in (0, 1, 4):  # 64 x 32 with the K split (the launcher's choice), 64 x 64, 128 x 64
        ybuf, yv = ao.padded(M, N, torch.float32, ao.SENTINEL, dev)
        ops.linear_fwd_fp8(xv, qv, sv, bv, yv, "linear", tile=tile)
        ratio = float((np.abs(yv.cpu().double().numpy() - ref) / bound).max())
        print(f"\nlinear_fp8 random 70x300x4112 tile {tile}: error at {ratio:.4f} x the derived "
              f"bound")
        assert ratio <= 1.0
        ao.assert_padding_untouched(ybuf, M, N, what="linear_fp8 random")
        ybuf2, yv2 = ao.padded(M, N, torch.float32, ao.SENTINEL, dev)
        ops.linear_fwd_fp8(xv, qv, sv, bv, yv2, "linear", tile=tile)
        assert torch.equal(ybuf, ybuf2), "two runs differ"


def test_linear_fp8_rejects_bad_operands(dev):
    x = torch.zeros(9, 32, dtype=torch.bfloat16, device=dev)
    q = torch.zeros(4, 32, dtype=torch.uint8, device=dev)
    s = torch.ones(4, device=dev)
    y = torch.zeros(9, 4, device=dev)
    ops.linear_fwd_fp8(x, q, s, None, y)  # 9 rows are fine
    with pytest.raises(ValueError):
        ops.linear_fwd_fp8(x[:, :24], q, s, None, y)  # K % 16
    with pytest.raises(ValueError):
        ops.linear_fwd_fp8(x, q, s[:3], None, y)  # scale shorter than N
    with pytest.raises(TypeError):
        ops.linear_fwd_fp8(x, q.to(torch.int8), s, None, y)
    with pytest.raises(ValueError):  # rows of codes not 16-byte aligned: the launcher's -2
        ops.linear_fwd_fp8(x[:, :16], torch.zeros(4, 24, dtype=torch.uint8, device=dev)[:, :16],
                           s, None, y)
    with pytest.raises(ValueError):  # no such tile: the launcher's -8
        ops.linear_fwd_fp8(x, q, s, None, y, tile=5)


# ---- engine ---------------------------------------------------------------------------------

DIMS = [40, 24, 10]
MODELS = {"relu": ("relu", "linear"), "sigmoid": ("sigmoid", "sigmoid")}


def _layers(acts):
    rng = np.random.default_rng(len(acts[0]))
    return [LayerWeights(rng.standard_normal((DIMS[i + 1], DIMS[i])) / np.sqrt(DIMS[i]),
                         rng.standard_normal(DIMS[i + 1]) * 0.1, acts[i]) for i in range(2)]


def _engine(acts, dev, split=False, **kw):
    L = _layers(acts)
    return InferenceEngine([L[:1], L[1:]] if split else [L], dev, expected_input=40,
                           weights="fp8", **kw)


def _all_layers(eng):
    return [(st.q[i], st.s[i], st.b[i], st.acts[i]) for st in eng.stages
            for i in range(len(st.layers))]


@pytest.mark.parametrize("mode", ["eager", "graph", "native"])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_engine_fp8_direct_buckets_chain_linear_fwd_fp8(dev, monkeypatch, model, mode):
    """fp8_gemm="direct": predict at 9, 64 and 65 rows (buckets 64, 64, 128) is bit-equal to
    ops.linear_fwd_fp8 chained by hand over the stage's codes on bucket-padded rows -- eagerly,
    under HIP-graph replay and under native Program replay, twice each; the sigmoid model as
    two stages. No such bucket allocates the bf16 scratch."""
    monkeypatch.setenv("DNN_SERVE_REPLAY", "native" if mode == "native" else "graph")
    eng = _engine(MODELS[model], dev, split=model == "sigmoid", use_graphs=mode != "eager",
                  fp8_gemm="direct")
    (q0, s0, b0, a0), (q1, s1, b1, a1) = _all_layers(eng)
    for rows, bucket in ((9, 64), (64, 64), (65, 128)):
        x = np.random.default_rng(rows).standard_normal((rows, 40))
        xb = torch.zeros(bucket, 64, dtype=torch.bfloat16, device=dev)
        ops.pack_bf16(torch.from_numpy(x).float().to(dev), xb[:rows])
        h = torch.zeros(bucket, 64, dtype=torch.bfloat16, device=dev)
        f = torch.zeros(bucket, 64, dtype=torch.float32, device=dev)
        ops.linear_fwd_fp8(xb, q0, s0, b0, h, a0)
        ops.linear_fwd_fp8(h, q1, s1, b1, f, a1)
        want = f[:rows, :10].double().cpu().numpy()
        for _ in range(2):  # capture / record, then replay
            assert np.array_equal(eng.predict(x), want), f"{model} {mode} rows={rows}"
    assert all(st._wscratch is None for st in eng.stages)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_engine_fp8_direct_leaves_other_buckets_alone(dev, model):
    """Under fp8_gemm="direct" a request of 2 * FP8_DIRECT_MAX_ROWS rows (the scratch path) and
    requests of 1, 5 and 8 rows (the GEMV) equal the default engine bit for bit."""
    direct = _engine(MODELS[model], dev, fp8_gemm="direct")
    default = _engine(MODELS[model], dev)
    for rows in (2 * ops.FP8_DIRECT_MAX_ROWS, 1, 5, 8):
        x = np.random.default_rng(rows).standard_normal((rows, 40))
        for _ in range(2):
            assert np.array_equal(direct.predict(x), default.predict(x)), f"rows={rows}"
    assert direct.stages[0]._wscratch is not None  # the large bucket took the scratch path


def test_engine_fp8_direct_one_layer_within_format_bound(dev):
    """One linear layer at 9 rows (the MFMA kernel) against the fp64 product with the ORIGINAL
    bf16 weights: every row inside the format + summation bound of the 1-row test (gc.
    check_one_layer), so the 9-row path is no less accurate than the definition."""
    w, b, _ = gc.one_layer_case()
    x = torch.randn(9, 64, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16)
    eng = InferenceEngine([[LayerWeights(w.float().numpy(), b.numpy(), "linear")]], dev,
                          expected_input=64, weights="fp8", fp8_gemm="direct")
    y = eng.predict(x.float().numpy())
    ratios = [gc.check_one_layer(y[m:m + 1], w, b, x[m:m + 1]) for m in range(9)]
    print(f"\nfp8 one-layer predict, 9 rows direct: error at {max(ratios):.3f} x the bound")
    assert eng.stages[0]._wscratch is None
