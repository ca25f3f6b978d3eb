"""The w4a8 GEMM (csrc/kernels/linear_w4a8.hip, ops.linear_w4a8 / ops.linear_fwd_w4a8) and the
engine's mxfp4_gemm="w4a8" mode on the GPU, against the exact oracles _mxfp4_oracle.py and
_fp8_oracle.py (the formats) and _act_oracle.py (the activations): operands and method in
_linear_w4a8_cases.py.

The kernel's constants (linear_w4a8.hip): 4 waves; a wave owns NG groups of 16 neurons; a k-step
is 128 columns = one MFMA = one LDS stage = 4 MX blocks, one per lane group; 4 stages = 512
columns of x, of codes and of scale bytes are in flight (one trip of the unrolled k loop).
``tile`` = 1 / 2 forces BM x BN = 64 x 64 (NG 1) / 128 x 128 (NG 2); 0 is the launcher's choice:
tile 1 while M <= 64 or ceil(N / 64) * ceil(M / 64) <= 512, else tile 2."""
import numpy as np
import pytest
import torch

import _act_oracle as ao
import _fp8_oracle as fo
import _gemv_fp8_cases as gc
import _gemv_mxfp4_cases as mg
import _linear_w4a8_cases as c4
import _linear_w8a8_cases as wc
import _mxfp4_oracle as mo
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
#      the 128-wide one (tile 2). Where the launcher itself leaves tile 1, with K = 32: 16384 /
#      16385 at 65 rows (512 / 514 workgroups of 64 x 64: the second takes 128 x 128).
#   K  32 (one block: lane group 0 of the first k-step, everything else past K); 96 / 128 / 160
#      one block below, at, one block past one MFMA k-step; 480 / 512 / 544 around the prefetch
#      depth (one loop trip); 992 / 1024 / 1056 around twice the depth; 4128 eight trips and a
#      block.
CASES = [
    (9, 1, 32, 0), (63, 15, 96, 0), (64, 16, 128, 0), (65, 17, 160, 0), (70, 63, 480, 0),
    (130, 64, 512, 0), (127, 65, 544, 0), (128, 33, 992, 0), (129, 31, 1024, 0),
    (9, 17, 1056, 0), (130, 65, 4128, 0),
    (65, 16384, 32, 0), (65, 16385, 32, 0),
    (9, 63, 32, 1), (65, 64, 160, 1), (70, 65, 1056, 1), (130, 17, 544, 1),
    (9, 1, 32, 2), (127, 127, 96, 2), (128, 128, 128, 2), (129, 129, 160, 2),
    (257, 130, 480, 2), (130, 15, 512, 2), (63, 16, 544, 2), (128, 17, 992, 2),
    (129, 33, 1024, 2), (127, 31, 1056, 2), (64, 32, 32, 2), (130, 128, 4128, 2),
]


@pytest.mark.parametrize("M,N,K,tile", CASES)
def test_linear_w4a8_equals_fp64_oracle(dev, M, N, K, tile):
    """Every activation, fp32 and bf16 output, bias and None, xq / q / e / sx / bias inside junk
    (e at an odd byte offset, 0xFE beside it, 0xFF in the rows past N): linear and relu EQUAL the
    fp64 value (every partial sum and the row-scale multiply are exact, so any tile, lane map
    and MFMA-internal order must give it; this is what establishes the operand and scale lane
    map of v_mfma_scale_f32_16x16x128_f8f6f4 in its fp4 x fp8 form as the kernel uses it, and
    that E = 0 blocks over junk codes add nothing), sigmoid within the GEMV's bounds, padding of
    y untouched."""
    worst = c4.check_exact(ops.linear_w4a8, M, N, K, dev, SIGMOID_F32_MAX_ULP, tile=tile)
    print(f"\nlinear_w4a8 {M}x{N}x{K} tile {tile}: sigmoid fp32 worst {worst:.2f} ulp (bound "
          f"{SIGMOID_F32_MAX_ULP:g})")


@pytest.mark.parametrize("tile", [0, 1, 2])
def test_linear_w4a8_decodes_every_code_and_scale(dev, tile):
    """16 codes x the 238 scale bytes the quantiser can write against x = 1.0: the MFMA's own
    decode of its fp4 operand and of its e8m0 scale operand, bit for bit; and an E = 0 block
    gives +0 for all 16 codes."""
    c4.check_decode(ops.linear_w4a8, dev, tile=tile)
    c4.check_zero_block(ops.linear_w4a8, dev, tile=tile)


def test_linear_fwd_w4a8_seam_where_nothing_is_lost(dev):
    """The seam between the paths that serve one mxfp4 layer. The exact-sum operands with +-448
    in column 0 of every row: the row's amax is 448, so the activation quantiser's scale is 1
    (asserted) and its codes are the values themselves. The sums stay exact (|z| <= 448 * 12 +
    2 * 12 * 575 + 4 < 2^15 with 2 fraction bits), so rows 0..7 of ops.linear_fwd_w4a8 at 128
    rows, ops.gemv_mxfp4 on those 8 rows and the parent path (dequant_rows_mxfp4 + linear_fwd)
    all hand the fp64 pre-activation to the same act_fwd and agree bit for bit, with the fp64
    value too for linear and relu."""
    M, N, K = 128, 128, 576
    o = c4.operands(M, N, K)
    ev, bv = o["e"].to(dev), o["bias"].float().to(dev)
    for act in ao.ACTS:
        sig = act == "sigmoid"
        src = o["xs" if sig else "x"].clone()
        src[:, 0] = torch.where(src[:, 0] < 0, -448.0, 448.0)
        w = o["ws" if sig else "w"]
        qv = o["qs" if sig else "q"].to(dev)
        xv = src.to(torch.bfloat16).to(dev)
        assert torch.equal(xv.double().cpu(), src)
        a = torch.zeros(M, N, device=dev)
        sx = torch.zeros(M, device=dev)
        ops.linear_fwd_w4a8(xv, qv, ev, bv, a, act, sx=sx)
        assert bool((sx == 1.0).all())
        b = torch.zeros(8, N, device=dev)
        ops.gemv_mxfp4(xv[:8], qv, ev, bv, b, act)
        assert torch.equal(a[:8], b), f"{act}: w4a8 differs from gemv_mxfp4"
        wd = torch.zeros(N, K, dtype=torch.bfloat16, device=dev)
        ops.dequant_rows_mxfp4(qv, ev, wd)
        c = torch.zeros(M, N, device=dev)
        ops.linear_fwd(xv, wd, bv, c, act)
        assert torch.equal(a, c), f"{act}: w4a8 differs from dequantise + bf16 GEMM"
        if not sig:
            z = src @ w.t() + o["bias"][:N]
            assert float(z.abs().max()) < 2.0 ** 15
            assert torch.equal(a.double().cpu(), ao.act_fwd(z, act)), act


def test_linear_w4a8_random_operands_within_derived_bound(dev):
    """Random bf16 x quantised by the kernel ops.quant_rows_fp8 (codes and scales first asserted
    equal to fo.quant_ref bit for bit) and random weights quantised by mo.quant_ref, at 70 x 300
    x 4128, against sx * (dec(xq) . values(q, e)^T) + b in fp64. The product of an e4m3 value (4
    significant bits) and an e2m1 value (2) times a power of two is exact in fp32, so the error
    is that of the additions and the epilogue. Every tile gives one wave all of K for an output:
    one MFMA per 128-column k-step, each adding its 128 products into the accumulator, so the
    longest chain is T = 128 * ceil(4128 / 128) = 128 * 33 = 4224 additions (the k loop's
    rounding up to whole trips only adds zeros), the same for every tile. Then the row-scale
    multiply, the bias add and a spare unit:
    |y - ref| <= (T + 3) * u * (sx * sum_k |dec value| + |b|) per output, u = 2^-24.
    u = 2^-24 held on MI355X: the worst error was 0.0020 of the bound on every tile (tile 0, 1
    and 2 alike; printed per tile). (The bound grows with T while rounding errors mostly
    cancel, so this margin does not tell a rounding accumulator from a chopping one; 2^-23, the
    only admissible alternative, was not needed.)
    A second call is bit-identical (fixed summation order)."""
    M, N, K = 70, 300, 4128
    g = torch.Generator().manual_seed(4128)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    bias = torch.randn(N, generator=g)
    q, e, _ = mo.quant_ref(w)
    xq_ref, sx_ref, _ = fo.quant_ref(x)
    _, xv = ao.padded(M, K, torch.bfloat16, float("nan"), dev, x)
    xqv = gc.padded_codes(torch.zeros(M, K, dtype=torch.uint8), dev)
    sxv = torch.full((M + 5,), float("nan"), device=dev)
    ops.quant_rows_fp8(xv, xqv, sxv)
    assert np.array_equal(xqv.cpu().numpy(), xq_ref), "quantiser codes differ from the oracle"
    assert np.array_equal(fo.bits32(sxv[:M]), fo.bits32(sx_ref)), "quantiser scales differ"
    qv = mg.padded_codes(torch.from_numpy(q), dev)
    ev = mg.padded_scales(torch.from_numpy(e), dev)
    bv = bias.to(dev)
    dx, dw = fo.DEC[xq_ref], mo.values(q, e)
    s64 = sx_ref.astype(np.float64)[:, None]
    b64 = bias.double().numpy()
    ref = s64 * (dx @ dw.T) + b64
    assert c4.chain_terms(K) == 4224
    bound = c4.summation_bound(K, s64 * (np.abs(dx) @ np.abs(dw).T), b64, u=2.0 ** -24)
    for tile in (0, 1, 2):  # the launcher's choice (64 x 64 here), 64 x 64, 128 x 128
        ybuf, yv = ao.padded(M, N, torch.float32, ao.SENTINEL, dev)
        ops.linear_w4a8(xqv, sxv, qv, ev, bv, yv, "linear", tile=tile)
        ratio = float((np.abs(yv.cpu().double().numpy() - ref) / bound).max())
        print(f"\nlinear_w4a8 random 70x300x4128 tile {tile}: error at {ratio:.4f} x the "
              f"derived bound (u = 2^-24)")
        assert ratio <= 1.0
        ao.assert_padding_untouched(ybuf, M, N, what="linear_w4a8 random")
        ybuf2, yv2 = ao.padded(M, N, torch.float32, ao.SENTINEL, dev)
        ops.linear_w4a8(xqv, sxv, qv, ev, bv, yv2, "linear", tile=tile)
        assert torch.equal(ybuf, ybuf2), "two runs differ"


def test_linear_fwd_w4a8_is_quantiser_plus_gemm(dev):
    """ops.linear_fwd_w4a8(x, ...) on random bf16 rows equals quant_rows_fp8 + linear_w4a8 by
    hand bit for bit, with its own temporaries and with the caller's (wider, taller) code and
    scale buffers, which then hold the quantised rows."""
    M, N, K = 70, 65, 544
    g = torch.Generator().manual_seed(70)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    q, e, _ = mo.quant_ref(w)
    qv, ev = torch.from_numpy(q).to(dev), torch.from_numpy(e).to(dev)
    bv = torch.randn(N, generator=g).to(dev)
    for act in ao.ACTS:
        xq = torch.zeros(M, K, dtype=torch.uint8, device=dev)
        sx = torch.zeros(M, device=dev)
        want = torch.zeros(M, N, device=dev)
        ops.quant_rows_fp8(x, xq, sx)
        ops.linear_w4a8(xq, sx, qv, ev, bv, want, act)
        got = torch.zeros(M, N, device=dev)
        ops.linear_fwd_w4a8(x, qv, ev, bv, got, act)
        assert torch.equal(got, want), act
        xq2 = torch.zeros(M + 2, K + 16, dtype=torch.uint8, device=dev)
        sx2 = torch.zeros(M + 2, device=dev)
        got2 = torch.zeros(M, N, device=dev)
        ops.linear_fwd_w4a8(x, qv, ev, bv, got2, act, xq=xq2, sx=sx2)
        assert torch.equal(got2, want), act
        assert torch.equal(xq2[:M, :K], xq) and torch.equal(sx2[:M], sx)


def test_linear_w4a8_rejects_bad_operands(dev):
    xq = torch.zeros(9, 64, dtype=torch.uint8, device=dev)
    q = torch.zeros(4, 32, dtype=torch.uint8, device=dev)
    e = torch.full((4, 2), 127, dtype=torch.uint8, device=dev)
    sx, b = torch.ones(9, device=dev), torch.zeros(4, device=dev)
    y = torch.zeros(9, 4, device=dev)
    ops.linear_w4a8(xq, sx, q, e, b, y)
    with pytest.raises(ValueError):
        ops.linear_w4a8(xq[:, :48], sx, q, e, None, y)  # K % 32
    with pytest.raises(ValueError):
        ops.linear_w4a8(xq, sx[:8], q, e, None, y)  # sx shorter than M
    with pytest.raises(ValueError):
        ops.linear_w4a8(xq, sx, q, e[:, :1], None, y)  # e narrower than K / 32
    with pytest.raises(ValueError):
        ops.linear_w4a8(xq, sx, q, e[:3], None, y)  # e shorter than N
    with pytest.raises(ValueError):
        ops.linear_w4a8(xq, sx, q, e, b[:3], y)  # bias shorter than N
    with pytest.raises(TypeError):
        ops.linear_w4a8(xq.to(torch.int8), sx, q, e, None, y)
    with pytest.raises(TypeError):
        ops.linear_w4a8(xq, sx, q.to(torch.int8), e, None, y)
    with pytest.raises(TypeError):
        ops.linear_w4a8(xq, sx, q, e.to(torch.int8), None, y)
    with pytest.raises(TypeError):
        ops.linear_w4a8(xq, sx, q, e, None, y.to(torch.float16))
    narrow_q = torch.zeros(4, 24, dtype=torch.uint8, device=dev)[:, :16]
    with pytest.raises(ValueError):  # rows of weight codes not 16-byte aligned
        ops.linear_w4a8(xq[:, :32], sx, narrow_q, e, None, y)
    narrow_x = torch.zeros(9, 40, dtype=torch.uint8, device=dev)[:, :32]
    with pytest.raises(ValueError):  # rows of activation codes not 16-byte aligned
        ops.linear_w4a8(narrow_x, sx, q[:, :16], e, None, y)
    with pytest.raises(ValueError):  # no such tile
        ops.linear_w4a8(xq, sx, q, e, None, y, tile=3)


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
                           weights="mxfp4", **kw)


def _all_layers(eng):
    return [(st.q4[i], st.e4[i], st.b[i], st.acts[i]) for st in eng.stages
            for i in range(len(st.layers))]


@pytest.mark.parametrize("mode", ["eager", "graph", "native"])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_engine_w4a8_buckets_chain_quantiser_and_gemm(dev, monkeypatch, model, mode):
    """mxfp4_gemm="w4a8": predict at 9, 64, 65 and 1025 rows (buckets 64, 64, 128, 2048 -- no row
    cap) is bit-equal to quant_rows_fp8 -> linear_w4a8 -> quant_rows_fp8 -> linear_w4a8 chained
    by hand on bucket-padded rows -- eagerly, under HIP-graph replay and under native Program
    replay, twice each; the sigmoid model as two stages. No stage allocates the bf16 scratch."""
    monkeypatch.setenv("DNN_SERVE_REPLAY", "native" if mode == "native" else "graph")
    eng = _engine(MODELS[model], dev, split=model == "sigmoid", use_graphs=mode != "eager",
                  mxfp4_gemm="w4a8")
    (q0, e0, b0, a0), (q1, e1, b1, a1) = _all_layers(eng)
    for rows, bucket in ((9, 64), (64, 64), (65, 128), (1025, 2048)):
        x = np.random.default_rng(rows).standard_normal((rows, 40))
        xb = torch.zeros(bucket, 64, dtype=torch.bfloat16, device=dev)
        ops.pack_bf16(torch.from_numpy(x).float().to(dev), xb[:rows])
        h = torch.zeros(bucket, 64, dtype=torch.bfloat16, device=dev)
        f = torch.zeros(bucket, 64, dtype=torch.float32, device=dev)
        c = torch.zeros(bucket, 64, dtype=torch.uint8, device=dev)
        sc = torch.zeros(bucket, device=dev)
        ops.quant_rows_fp8(xb, c, sc)
        ops.linear_w4a8(c, sc, q0, e0, b0, h, a0)
        ops.quant_rows_fp8(h, c, sc)
        ops.linear_w4a8(c, sc, q1, e1, b1, f, a1)
        want = f[:rows, :10].double().cpu().numpy()
        for _ in range(2):  # capture / record, then replay
            assert np.array_equal(eng.predict(x), want), f"{model} {mode} rows={rows}"
    assert all(st._wscratch is None for st in eng.stages)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_engine_w4a8_leaves_small_requests_alone(dev, model):
    """Requests of 1, 5 and 8 rows (gemv_mxfp4 on bf16 activations) equal the default mxfp4
    engine bit for bit."""
    w4a8 = _engine(MODELS[model], dev, mxfp4_gemm="w4a8")
    default = _engine(MODELS[model], dev)
    for rows in (1, 5, 8):
        x = np.random.default_rng(rows).standard_normal((rows, 40))
        for _ in range(2):
            assert np.array_equal(w4a8.predict(x), default.predict(x)), f"rows={rows}"
    assert w4a8.stages[0]._wscratch is None


def test_engine_w4a8_one_layer_within_format_bound(dev):
    """One linear 64 -> 24 layer at 9 rows against the fp64 product x . w^T + bias with the
    ORIGINAL bf16 weights and inputs. The kernel computes sum_k X_k W_k with X = sx dec(xq), W =
    dec(q) 2^(e - 127), and X_k W_k - x_k w_k = (X_k - x_k) w_k + (W_k - w_k) x_k + (X_k - x_k)
    (W_k - w_k). The weight term is mo.format_bound (|W - w| <= max(2^(E - 127), |w|) / 4,
    asserted), the activation term wc.element_bound (fo.round_trip_bound less its bf16 term:
    nothing is rounded to bf16 here, asserted), so
    |y - ref| <= sum_k (bx(x_k) |w_k| + bw(w_k) |x_k| + bx(x_k) bw(w_k))
                 + (T + 3) 2^-24 (sum_k |X_k W_k| + |bias|),   T = 128 ceil(64 / 128) = 128,
    the second line being the summation term of the random-operand test."""
    w, b, _ = gc.one_layer_case()
    x = torch.randn(9, 64, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16)
    eng = InferenceEngine([[LayerWeights(w.float().numpy(), b.numpy(), "linear")]], dev,
                          expected_input=64, weights="mxfp4", mxfp4_gemm="w4a8")
    y = eng.predict(x.float().numpy())
    w64, x64, b64 = w.double().numpy(), x.double().numpy(), b.double().numpy()
    (qw, ew, _), (qx, sx, _) = mo.quant_ref(w), fo.quant_ref(x)
    W = mo.values(qw, ew)
    X = sx.astype(np.float64)[:, None] * fo.DEC[qx]
    bw, bx = mo.format_bound(w64, ew), wc.element_bound(x64)
    assert (np.abs(W - w64) <= bw).all() and (np.abs(X - x64) <= bx).all()
    ref = x64 @ w64.T + b64
    bound = bx @ np.abs(w64).T + np.abs(x64) @ bw.T + bx @ bw.T + \
        c4.summation_bound(64, np.abs(X) @ np.abs(W).T, b64)
    ratio = float((np.abs(y - ref) / bound).max())
    print(f"\nw4a8 one-layer predict, 9 rows: error at {ratio:.3f} x the format + summation bound")
    assert ratio <= 1.0
    assert eng.stages[0]._wscratch is None
