"""Fused stage forward (csrc/kernels/stage_fwd.hip) on the GPU: exact operands EQUAL fp64,
random operands within a derived forward bound, the last-layer softmax, the refusals, and the
engine option ``stage_gemm="fused"`` under graph and native replay."""
import numpy as np
import pytest
import torch

import _stage_fwd_cases as sc
from _act_oracle import SENTINEL as SENT, assert_padding_untouched, padded
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.engine.inference import InferenceEngine

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def run(x, ws, bs, acts, M, out_dtype, n_cls=0, tile=0):
    """ops.stage_fwd on junk-surrounded strided views; returns (y buffer, y view)."""
    op = lambda t: padded(*t.shape, torch.bfloat16, 7.0, DEV, torch.as_tensor(t))[1]  # noqa: E731
    bv = [None if b is None else torch.as_tensor(b, dtype=torch.float32).to(DEV) for b in bs]
    ybuf, yv = padded(M, ws[-1].shape[0], out_dtype, SENT, DEV)
    ops.stage_fwd(op(x), [op(w) for w in ws], bv, acts, yv, n_cls=n_cls, tile=tile)
    torch.cuda.synchronize()
    return ybuf, yv.cpu()


ALL64, GROW, ODD = [64, 64, 64], [64, 128, 512], [832, 64, 192, 320]
EXACT = (
    # M around each tile (16, 64), 1 and 9 rows, 200 = three 64-row tiles + a partial one
    [(M, ALL64, t, "rows vs tile edges") for M in (1, 9, 15, 16, 17, 63, 64, 65, 200)
     for t in (0, 1, 2)] +
    [(M, sc.HEADLINE, t, "headline widths, K0 = 832, NG 8/4/2/1") for M in (17, 200)
     for t in (1, 2)] +
    [(65, GROW, t, "widths grow, 512-wide last layer") for t in (1, 2)] +
    [(33, ODD, t, "NG 1/3/5: ring depths 4 and the k-step remainder") for t in (1, 2)] +
    [(65, [64] * 5 + [128, 64, 128, 64], 0, "8 layers")] +
    [(M, ALL64, 0, "launcher's tile threshold") for M in (4096, 4097)])


@pytest.mark.parametrize("M,widths,tile,why", EXACT)
def test_exact_operands_equal_fp64(M, widths, tile, why):
    acts = ["relu" if l % 2 == 0 else "linear" for l in range(len(widths) - 1)]
    for bias in (True, False):
        x, ws, bs = sc.exact_case(M, widths, seed=M + len(widths), bias=bias)
        want, _ = sc.chain64(x, ws, bs, acts, exact=True)
        for dt in (torch.float32, torch.bfloat16):
            ybuf, y = run(x, ws, bs, acts, M, dt, tile=tile)
            assert np.array_equal(y.double().numpy(), want), f"{why} {dt} bias={bias}"
            assert_padding_untouched(ybuf, M, widths[-1], what=why)


@pytest.mark.parametrize("M,widths,acts", [
    (130, sc.HEADLINE, ["relu", "sigmoid", "relu", "linear"]),
    (130, sc.HEADLINE, ["sigmoid", "relu", "sigmoid", "sigmoid"]),
    (70, [128, 192, 64], ["sigmoid", "linear"])])
def test_random_operands_within_forward_bound(M, widths, acts):
    x, ws, bs = sc.random_case(M, widths, seed=M)
    for dt in (torch.float32, torch.bfloat16):
        want, e = sc.chain64(x, ws, bs, acts, out_bf16=dt == torch.bfloat16)
        for tile in (1, 2):
            _, y = run(x, ws, bs, acts, M, dt, tile=tile)
            ratio = float((np.abs(y.double().numpy() - want) / e).max())
            print(f"stage_fwd {widths} {acts} {dt} tile {tile}: worst error / bound {ratio:.4f}")
            assert ratio <= 1.0


@pytest.mark.parametrize("n_cls", [1, 10, 63, 64])
@pytest.mark.parametrize("tile", [1, 2])
def test_last_layer_softmax(n_cls, tile):
    M, widths = 70, [128, 192, 64]
    x, ws, bs = sc.random_case(M, widths, seed=n_cls)
    _, logits = run(x, ws, bs, ["relu", "linear"], M, torch.float32, tile=tile)
    z = logits.double()[:, :n_cls]
    want = torch.softmax(z, dim=1)
    ybuf, y = run(x, ws, bs, ["relu", "softmax"], M, torch.float32, n_cls=n_cls, tile=tile)
    torch.testing.assert_close(y.double()[:, :n_cls], want, rtol=1e-5, atol=1e-6)
    assert bool((y[:, n_cls:] == SENT).all())
    assert_padding_untouched(ybuf, M, 64)


@pytest.mark.parametrize("widths,acts,n_cls,why", sc.REFUSED + [
    ([64, 128, 64], ["relu", "linear"], 0, "Kp / Np mismatch")])
def test_refusals_launch_nothing(widths, acts, n_cls, why):
    assert why == "Kp / Np mismatch" or not ops.stage_fwd_supported(widths, acts, n_cls)
    x = torch.zeros(16, widths[0], dtype=torch.bfloat16, device=DEV)
    ws = [torch.zeros(n, k, dtype=torch.bfloat16, device=DEV) for k, n in zip(widths, widths[1:])]
    if why == "Kp / Np mismatch":
        ws[1] = torch.zeros(64, 64, dtype=torch.bfloat16, device=DEV)
    y = torch.full((16, widths[-1]), SENT, device=DEV)
    with pytest.raises(ValueError):
        ops.stage_fwd(x, ws, [None] * len(ws), acts, y, n_cls=n_cls)
    torch.cuda.synchronize()
    assert bool((y == SENT).all()), why


DIMS, ACTS = [784, 512, 256, 128, 10], ["relu", "sigmoid", "relu", "softmax"]


@pytest.mark.parametrize("mode", ["graph", "native"])
@pytest.mark.parametrize("split", [[4], [2, 2]])
def test_engine_fused(mode, split, monkeypatch):
    monkeypatch.setenv("DNN_SERVE_REPLAY", mode)
    L = sc.model_layers(DIMS, ACTS, seed=3)
    stages = [L[sum(split[:i]):sum(split[:i + 1])] for i in range(len(split))]
    eng = InferenceEngine(stages, DEV, expected_input=784, stage_gemm="fused")
    for rows in (9, 64, 65, 200):
        for rep in range(2):  # the second request replays what the first recorded
            x = np.random.default_rng(rows + rep).standard_normal((rows, 784))
            got = eng.predict(x)
            R = eng._bucket(rows)
            assert all(st.buffers(R)["fused"] and st.buffers(R)["h"][0] is None
                       for st in eng.stages)
            # bit for bit a direct ops.stage_fwd per stage on the same padded input
            h = torch.zeros(R, 832, dtype=torch.bfloat16, device=DEV)
            h[:rows, :784] = torch.as_tensor(x, dtype=torch.float32).to(DEV).to(torch.bfloat16)
            x64 = h.double().cpu().numpy()
            for st in eng.stages:
                y = torch.zeros(R, st.pads[-1], device=DEV,
                                dtype=torch.float32 if st.is_last else torch.bfloat16)
                h = ops.stage_fwd(h, st.w, st.b, st.acts, y, n_cls=10 if st.is_last else 0)
            assert np.array_equal(got, h[:rows, :10].double().cpu().numpy()), (rows, rep)
            # within the forward bound of the fp64 chain (a hop is that activation's one bf16
            # rounding; softmax: |dp_i| <= 2 max |dz|, plus test_last_layer_softmax's tolerance)
            ws = [w.double().cpu().numpy() for st in eng.stages for w in st.w]
            bs = [b.double().cpu().numpy() for st in eng.stages for b in st.b]
            z, e = sc.chain64(x64, ws, bs, ACTS[:-1] + ["linear"])
            want = torch.softmax(torch.as_tensor(z[:rows, :10]), dim=1).numpy()
            bound = 2 * e[:rows, :10].max(axis=1, keepdims=True) + 1e-5 * want + 1e-6
            assert (np.abs(got - want) <= bound).all(), (rows, rep)


def test_engine_fallbacks_never_reach_the_kernel():
    L = sc.model_layers(DIMS, ACTS, seed=4)
    wide = sc.model_layers([784, 1024, 10], ["relu", "softmax"], seed=5)
    for layers, kw, rows in ((L, {}, 8), (L, {"weights": "fp8"}, 64), (wide, {}, 64)):
        a = InferenceEngine([layers], DEV, expected_input=784, **kw)
        b = InferenceEngine([layers], DEV, expected_input=784, stage_gemm="fused", **kw)
        x = np.random.default_rng(rows).standard_normal((rows, 784))
        assert np.array_equal(a.predict(x), b.predict(x))
        st = b.stages[0]
        bufs = st.buffers(b._bucket(rows))
        assert not bufs["fused"] and all(h is not None for h in bufs["h"])
    assert not ops.stage_fwd_supported([832, 1024, 64], ["relu", "softmax"], 10)
