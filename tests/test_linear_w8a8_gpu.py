"""The w8a8 GEMM (csrc/kernels/linear_w8a8.hip, ops.linear_w8a8 / ops.linear_fwd_w8a8) and the
engine's fp8_gemm="w8a8" mode on the GPU, against the exact oracles _fp8_oracle.py (the format)
and _act_oracle.py (the activations): operands and method in _linear_w8a8_cases.py.

The kernel's constants (linear_w8a8.hip): 4 waves; a wave owns NG groups of 16 neurons; a k-step
is 128 columns = one MFMA = one LDS stage; 4 stages = 512 columns of x and of codes are in flight
(one trip of the unrolled k loop). ``tile`` = 1 / 2 forces BM x BN = 64 x 64 (NG 1) / 128 x 128
(NG 2); 0 is the launcher's choice: tile 1 while M <= 64 or ceil(N / 64) * ceil(M / 64) <= 512,
else tile 2."""
import numpy as np
import pytest
import torch

import _act_oracle as ao
import _fp8_oracle as fo
import _gemv_fp8_cases as gc
import _linear_w8a8_cases as wc
from test_gemv_gpu import SIGMOID_F32_MAX_ULP
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.config import LayerWeights
from docker_dist_nn_amd.engine.inference import InferenceEngine

pytestmark = pytest.mark.gpu

# (M, N, K, tile). Which edge each value hits:
#   M  9 first past the GEMV; 63 / 64 / 65 below, at, past the 64-row tile (tile 1; 65: a second
#      row tile with one row); 70 and 130: two and three 64-row tiles; 127 / 128 / 129 below, at,
#      past the 128-row tile (tile 2; 129 and 130: two of them); 257: three 128-row tiles.
#   N  1; 15 / 16 / 17 around a group of 16 neurons; 31 / 32 / 33 around a wave's 32 neurons
#      (tile 2); 63 / 64 / 65 around the 64-wide workgroup (tile 1); 127 / 128 / 129 / 130 around
#      the 128-wide one (tile 2). Where the launcher itself leaves tile 1, with K = 16: 16384 /
#      16385 at 65 rows (512 / 514 workgroups of 64 x 64: the second takes 128 x 128).
#   K  16 (one 16-byte half of lane group 0, everything else past K); 112 / 128 / 144 below, at,
#      16 past one MFMA k-step; 496 / 512 / 528 around the prefetch depth (one loop trip); 1008 /
#      1024 / 1040 around twice the depth; 4112 eight trips and a step.
CASES = [
    (9, 1, 16, 0), (63, 15, 112, 0), (64, 16, 128, 0), (65, 17, 144, 0), (70, 63, 496, 0),
    (130, 64, 512, 0), (127, 65, 528, 0), (128, 33, 1008, 0), (129, 31, 1024, 0),
    (9, 17, 1040, 0), (130, 65, 4112, 0),
    (65, 16384, 16, 0), (65, 16385, 16, 0),
    (9, 63, 16, 1), (65, 64, 144, 1), (70, 65, 1040, 1), (130, 17, 528, 1),
    (9, 1, 16, 2), (127, 127, 112, 2), (128, 128, 128, 2), (129, 129, 144, 2),
    (257, 130, 496, 2), (130, 15, 512, 2), (63, 16, 528, 2), (128, 17, 1008, 2),
    (129, 33, 1024, 2), (127, 31, 1040, 2), (64, 32, 16, 2), (130, 128, 4112, 2),
]


@pytest.mark.parametrize("M,N,K,tile", CASES)
def test_linear_w8a8_equals_fp64_oracle(dev, M, N, K, tile):
    """Every activation, fp32 and bf16 output, bias and None, NaN-padded xq / q / sx / sw /
    bias: linear and relu EQUAL the fp64 value (every partial sum and both scale multiplies are
    exact, so any tile, lane map and MFMA-internal order must give it; this is what establishes
    the operand map of v_mfma_scale_f32_16x16x128_f8f6f4 as the kernel uses it), sigmoid within
    the GEMV's bounds, padding of y untouched."""
    worst = wc.check_exact(ops.linear_w8a8, M, N, K, dev, SIGMOID_F32_MAX_ULP, tile=tile)
    print(f"\nlinear_w8a8 {M}x{N}x{K} tile {tile}: sigmoid fp32 worst {worst:.2f} ulp (bound "
          f"{SIGMOID_F32_MAX_ULP:g})")


ONE = 0x38  # the e4m3 code of 1.0


@pytest.mark.parametrize("tile", [0, 1, 2])
def test_linear_w8a8_decodes_every_weight_code(dev, tile):
    """q[n][0] = n, xq = the code of 1.0 in row 0 only (9 rows), scales 1: y[0][n] is the MFMA's
    own decode of code n on its A operand. It equals the oracle's table bit for bit for the 254
    finite codes (OCP e4m3, not fnuz) and is NaN for 0x7F / 0xFF; rows 1..8 are +0."""
    assert fo.DEC[ONE] == 1.0
    q = torch.zeros(256, 16, dtype=torch.uint8)
    q[:, 0] = torch.arange(256, dtype=torch.uint8)
    xq = torch.zeros(9, 16, dtype=torch.uint8)
    xq[0, 0] = ONE
    y = torch.full((9, 256), ao.SENTINEL, dtype=torch.float32, device=dev)
    ops.linear_w8a8(xq.to(dev), torch.ones(9, device=dev), q.to(dev),
                    torch.ones(256, device=dev), None, y, "linear", tile=tile)
    got = y.cpu().numpy()
    want = fo.DEC.astype(np.float32) + np.float32(0.0)
    finite = np.isfinite(fo.DEC)
    assert finite.sum() == 254 and not finite[0x7F] and not finite[0xFF]
    assert np.array_equal(fo.bits32(got[0][finite]), fo.bits32(want[finite]))
    assert np.isnan(got[0][0x7F]) and np.isnan(got[0][0xFF])
    assert not fo.bits32(got[1:, finite]).any()  # +0: no bit set


@pytest.mark.parametrize("tile", [0, 1, 2])
def test_linear_w8a8_decodes_every_activation_code(dev, tile):
    """xq[m][0] = m for 256 rows against one neuron whose code 0 is 1.0: y[m][0] is the MFMA's
    decode of code m on its B operand, bit for bit the oracle's table, NaN at 0x7F / 0xFF."""
    xq = torch.zeros(256, 16, dtype=torch.uint8)
    xq[:, 0] = torch.arange(256, dtype=torch.uint8)
    q = torch.zeros(1, 16, dtype=torch.uint8)
    q[0, 0] = ONE
    y = torch.full((256, 1), ao.SENTINEL, dtype=torch.float32, device=dev)
    ops.linear_w8a8(xq.to(dev), torch.ones(256, device=dev), q.to(dev),
                    torch.ones(1, device=dev), None, y, "linear", tile=tile)
    got = y.cpu().numpy()[:, 0]
    want = fo.DEC.astype(np.float32) + np.float32(0.0)
    finite = np.isfinite(fo.DEC)
    assert np.array_equal(fo.bits32(got[finite]), fo.bits32(want[finite]))
    assert np.isnan(got[0x7F]) and np.isnan(got[0xFF])


def test_linear_w8a8_random_operands_within_derived_bound(dev):
    """Random bf16 x quantised by the kernel ops.quant_rows_fp8 (codes and scales first asserted
    equal to fo.quant_ref bit for bit) and random weights quantised by fo.quant_ref, at 70 x 300
    x 4112, against sx * sw * (dec(xq) . dec(q)^T) + b in fp64. A product of two e4m3 values is
    exact in fp32 (4 x 4 significant bits), so the error is that of the additions and the
    epilogue. Every tile gives one wave all of K for an output: one MFMA per 128-column k-step,
    each adding its 128 products into the accumulator, so the longest chain is T = 128 *
    ceil(4112 / 128) = 128 * 33 = 4224 additions (the k loop's rounding up to whole trips only
    adds zeros), the same for every tile. Then the two scale multiplies, the bias add and a
    spare unit:
    |y - ref| <= (T + 4) * u * (sx * sw * sum_k |dec dec| + |b|) per output, u = 2^-24.
    u = 2^-24 held on MI355X: the worst error was 0.0059 of the bound on every tile. (The
    bound grows with T while rounding errors mostly cancel, so this margin does not tell a
    rounding accumulator from a chopping one; 2^-23 was not needed.)
    A second call is bit-identical (fixed summation order)."""
    M, N, K = 70, 300, 4112
    g = torch.Generator().manual_seed(4112)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    bias = torch.randn(N, generator=g)
    q, sw, _ = fo.quant_ref(w)
    xq_ref, sx_ref, _ = fo.quant_ref(x)
    _, xv = ao.padded(M, K, torch.bfloat16, float("nan"), dev, x)
    xqv = gc.padded_codes(torch.zeros(M, K, dtype=torch.uint8), dev)
    sxv = torch.full((M + 5,), float("nan"), device=dev)
    ops.quant_rows_fp8(xv, xqv, sxv)
    assert np.array_equal(xqv.cpu().numpy(), xq_ref), "quantiser codes differ from the oracle"
    assert np.array_equal(fo.bits32(sxv[:M]), fo.bits32(sx_ref)), "quantiser scales differ"
    qv, swv, bv = gc.padded_codes(torch.from_numpy(q), dev), torch.from_numpy(sw).to(dev), \
        bias.to(dev)
    dx, dq = fo.DEC[xq_ref], fo.DEC[q]
    ss = sx_ref.astype(np.float64)[:, None] * sw.astype(np.float64)[None, :]
    b64 = bias.double().numpy()
    ref = ss * (dx @ dq.T) + b64
    assert wc.chain_terms(K) == 4224
    bound = wc.summation_bound(K, ss * (np.abs(dx) @ np.abs(dq).T), b64, u=2.0 ** -24)
    for tile in (0, 1, 2):  # the launcher's choice (64 x 64 here), 64 x 64, 128 x 128
        ybuf, yv = ao.padded(M, N, torch.float32, ao.SENTINEL, dev)
        ops.linear_w8a8(xqv, sxv, qv, swv, bv, yv, "linear", tile=tile)
        ratio = float((np.abs(yv.cpu().double().numpy() - ref) / bound).max())
        print(f"\nlinear_w8a8 random 70x300x4112 tile {tile}: error at {ratio:.4f} x the "
              f"derived bound (u = 2^-24)")
        assert ratio <= 1.0
        ao.assert_padding_untouched(ybuf, M, N, what="linear_w8a8 random")
        ybuf2, yv2 = ao.padded(M, N, torch.float32, ao.SENTINEL, dev)
        ops.linear_w8a8(xqv, sxv, qv, swv, bv, yv2, "linear", tile=tile)
        assert torch.equal(ybuf, ybuf2), "two runs differ"


def test_linear_fwd_w8a8_is_quantiser_plus_gemm(dev):
    """ops.linear_fwd_w8a8(x, ...) on random bf16 rows equals quant_rows_fp8 + linear_w8a8 by
    hand bit for bit, with its own temporaries and with the caller's (wider, taller) code and
    scale buffers, which then hold the quantised rows."""
    M, N, K = 70, 65, 528
    g = torch.Generator().manual_seed(70)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    q, sw, _ = fo.quant_ref(w)
    qv, swv = torch.from_numpy(q).to(dev), torch.from_numpy(sw).to(dev)
    bv = torch.randn(N, generator=g).to(dev)
    for act in ao.ACTS:
        xq = torch.zeros(M, K, dtype=torch.uint8, device=dev)
        sx = torch.zeros(M, device=dev)
        want = torch.zeros(M, N, device=dev)
        ops.quant_rows_fp8(x, xq, sx)
        ops.linear_w8a8(xq, sx, qv, swv, bv, want, act)
        got = torch.zeros(M, N, device=dev)
        ops.linear_fwd_w8a8(x, qv, swv, bv, got, act)
        assert torch.equal(got, want), act
        xq2 = torch.zeros(M + 2, K + 16, dtype=torch.uint8, device=dev)
        sx2 = torch.zeros(M + 2, device=dev)
        got2 = torch.zeros(M, N, device=dev)
        ops.linear_fwd_w8a8(x, qv, swv, bv, got2, act, xq=xq2, sx=sx2)
        assert torch.equal(got2, want), act
        assert torch.equal(xq2[:M, :K], xq) and torch.equal(sx2[:M], sx)


def test_linear_fwd_w8a8_equals_linear_fwd_fp8_where_nothing_is_lost(dev):
    """The seam between the two fp8 GEMMs. The exact-sum operands of the first test with +-448
    in column 0 of every row: the row's amax is 448, so the quantiser's scale and inverse are 1
    (asserted: all sx are 1) and its codes are the values themselves -- it loses nothing. The
    sums stay exact (|z| <= 2 * (896 + 4 * 527) + 4 < 2^13 with 3 fraction bits), so
    ops.linear_fwd_w8a8(x) and ops.linear_fwd_fp8(x) both give the fp64 pre-activation to the
    same act_fwd and agree bit for bit, with the fp64 value too for linear and relu."""
    M, N, K = 70, 65, 528
    x, xs, _, _, _, w, q, sw, bias = wc.operands(M, N, K)
    qv, swv, bv = q.to(dev), sw.float().to(dev), bias.float().to(dev)
    for act in ao.ACTS:
        src = (xs if act == "sigmoid" else x).clone()
        src[:, 0] = torch.where(src[:, 0] < 0, -448.0, 448.0)
        xv = src.to(torch.bfloat16).to(dev)
        assert torch.equal(xv.double().cpu(), src)
        a = torch.zeros(M, N, device=dev)
        b = torch.zeros(M, N, device=dev)
        sx = torch.zeros(M, device=dev)
        ops.linear_fwd_fp8(xv, qv, swv, bv, a, act)
        ops.linear_fwd_w8a8(xv, qv, swv, bv, b, act, sx=sx)
        assert bool((sx == 1.0).all())
        assert torch.equal(a, b), act
        if act != "sigmoid":
            z = gc.oracle_z(src, w, sw, bias, M, N)
            assert torch.equal(b.double().cpu(), ao.act_fwd(z, act)), act


def test_linear_w8a8_rejects_bad_operands(dev):
    xq = torch.zeros(9, 32, dtype=torch.uint8, device=dev)
    q = torch.zeros(4, 32, dtype=torch.uint8, device=dev)
    sx, s = torch.ones(9, device=dev), torch.ones(4, device=dev)
    y = torch.zeros(9, 4, device=dev)
    ops.linear_w8a8(xq, sx, q, s, None, y)
    with pytest.raises(ValueError):
        ops.linear_w8a8(xq[:, :24], sx, q, s, None, y)  # K % 16
    with pytest.raises(ValueError):
        ops.linear_w8a8(xq, sx[:8], q, s, None, y)  # sx shorter than M
    with pytest.raises(ValueError):
        ops.linear_w8a8(xq, sx, q, s[:3], None, y)  # sw shorter than N
    with pytest.raises(TypeError):
        ops.linear_w8a8(xq.to(torch.int8), sx, q, s, None, y)
    with pytest.raises(TypeError):
        ops.linear_w8a8(xq, sx, q.to(torch.int8), s, None, y)
    narrow = torch.zeros(9, 24, dtype=torch.uint8, device=dev)[:, :16]
    with pytest.raises(ValueError):  # rows of weight codes not 16-byte aligned: the launcher's -2
        ops.linear_w8a8(xq[:, :16], sx, narrow[:4], s, None, y)
    with pytest.raises(ValueError):  # rows of activation codes not 16-byte aligned
        ops.linear_w8a8(narrow, sx, q[:, :16], s, None, y)
    with pytest.raises(ValueError):  # no such tile: the launcher's -8
        ops.linear_w8a8(xq, sx, q, s, None, y, tile=3)


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
def test_engine_w8a8_buckets_chain_quantiser_and_gemm(dev, monkeypatch, model, mode):
    """fp8_gemm="w8a8": predict at 9, 64, 65 and 1025 rows (buckets 64, 64, 128, 2048 -- no row
    cap) is bit-equal to quant_rows_fp8 -> linear_w8a8 -> quant_rows_fp8 -> linear_w8a8 chained
    by hand on bucket-padded rows -- eagerly, under HIP-graph replay and under native Program
    replay, twice each; the sigmoid model as two stages (its hidden pad columns hold 0.5 and
    enter the row's amax on both sides). No stage allocates the bf16 scratch."""
    monkeypatch.setenv("DNN_SERVE_REPLAY", "native" if mode == "native" else "graph")
    eng = _engine(MODELS[model], dev, split=model == "sigmoid", use_graphs=mode != "eager",
                  fp8_gemm="w8a8")
    (q0, s0, b0, a0), (q1, s1, b1, a1) = _all_layers(eng)
    for rows, bucket in ((9, 64), (64, 64), (65, 128), (1025, 2048)):
        x = np.random.default_rng(rows).standard_normal((rows, 40))
        xb = torch.zeros(bucket, 64, dtype=torch.bfloat16, device=dev)
        ops.pack_bf16(torch.from_numpy(x).float().to(dev), xb[:rows])
        h = torch.zeros(bucket, 64, dtype=torch.bfloat16, device=dev)
        f = torch.zeros(bucket, 64, dtype=torch.float32, device=dev)
        c = torch.zeros(bucket, 64, dtype=torch.uint8, device=dev)
        sc = torch.zeros(bucket, device=dev)
        ops.quant_rows_fp8(xb, c, sc)
        ops.linear_w8a8(c, sc, q0, s0, b0, h, a0)
        ops.quant_rows_fp8(h, c, sc)
        ops.linear_w8a8(c, sc, q1, s1, b1, f, a1)
        want = f[:rows, :10].double().cpu().numpy()
        for _ in range(2):  # capture / record, then replay
            assert np.array_equal(eng.predict(x), want), f"{model} {mode} rows={rows}"
    assert all(st._wscratch is None for st in eng.stages)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_engine_w8a8_leaves_small_requests_alone(dev, model):
    """Requests of 1, 5 and 8 rows (gemv_fp8 on bf16 activations) equal the default fp8 engine
    bit for bit."""
    w8a8 = _engine(MODELS[model], dev, fp8_gemm="w8a8")
    default = _engine(MODELS[model], dev)
    for rows in (1, 5, 8):
        x = np.random.default_rng(rows).standard_normal((rows, 40))
        for _ in range(2):
            assert np.array_equal(w8a8.predict(x), default.predict(x)), f"rows={rows}"
    assert w8a8.stages[0]._wscratch is None


def test_engine_w8a8_one_layer_within_format_bound(dev):
    """One linear 64 -> 24 layer at 9 rows against the fp64 product x . w^T + bias with the
    ORIGINAL bf16 weights and inputs. The kernel computes sum_k X_k W_k with X = sx dec(xq), W =
    sw dec(q), and X_k W_k - x_k w_k = (X_k - x_k) w_k + (W_k - w_k) x_k + (X_k - x_k)(W_k - w_k).
    Each operand's codes are within b(v) = fo.round_trip_bound(v, row amax) less its bf16 term
    2^-8 |v| of the value (nothing is rounded to bf16 here: wc.element_bound, asserted for both
    operands), so
    |y - ref| <= sum_k (b(x_k) |w_k| + b(w_k) |x_k| + b(x_k) b(w_k))
                 + (T + 4) 2^-24 (sum_k |X_k W_k| + |bias|),   T = 128 ceil(64 / 128) = 128,
    the second line being the summation term of the random-operand test."""
    w, b, _ = gc.one_layer_case()
    x = torch.randn(9, 64, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16)
    eng = InferenceEngine([[LayerWeights(w.float().numpy(), b.numpy(), "linear")]], dev,
                          expected_input=64, weights="fp8", fp8_gemm="w8a8")
    y = eng.predict(x.float().numpy())
    w64, x64, b64 = w.double().numpy(), x.double().numpy(), b.double().numpy()
    bw, bx = wc.element_bound(w64), wc.element_bound(x64)
    (qw, sw, _), (qx, sx, _) = fo.quant_ref(w), fo.quant_ref(x)
    W = sw.astype(np.float64)[:, None] * fo.DEC[qw]
    X = sx.astype(np.float64)[:, None] * fo.DEC[qx]
    assert (np.abs(W - w64) <= bw).all() and (np.abs(X - x64) <= bx).all()
    ref = x64 @ w64.T + b64
    bound = bx @ np.abs(w64).T + np.abs(x64) @ bw.T + bx @ bw.T + \
        wc.summation_bound(64, np.abs(X) @ np.abs(W).T, b64)
    ratio = float((np.abs(y - ref) / bound).max())
    print(f"\nw8a8 one-layer predict, 9 rows: error at {ratio:.3f} x the format + summation bound")
    assert ratio <= 1.0
    assert eng.stages[0]._wscratch is None
