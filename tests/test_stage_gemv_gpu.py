"""Fused small-batch stage forward (csrc/kernels/stage_gemv.hip) on the GPU: bit for bit the
chain of ops.gemv (+ ops.softmax_rows), equal to / within the forward bound of the fp64 chain,
the hand-off's workspace and counter across launches, the refusals, and the engine option
``stage_gemv="fused"`` under graph and native replay."""
import numpy as np
import pytest
import torch

import _stage_fwd_cases as sc
from _act_oracle import SENTINEL as SENT, assert_padding_untouched, padded
from docker_dist_nn_amd import ops
from docker_dist_nn_amd.engine.inference import InferenceEngine

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROWS = [1, 2, 3, 5, 8]  # every row template (1, 2, 4, 8) and both guarded ones
WIDTHS = [sc.HEADLINE,            # two chunks in the head, the second partial
          [64, 64, 64],           # lanes >= 8 idle; the tail's smallest layer
          [2112, 512, 512, 64],   # the head's loop beyond 2048; the tail's widest layer
          [64] * 9]               # 8 layers
HIDDEN = ["relu", "sigmoid", "linear"]


def operands(x, ws, bs):
    op = lambda t: padded(*t.shape, torch.bfloat16, 7.0, DEV, torch.as_tensor(t))[1]  # noqa: E731
    return op(x), [op(w) for w in ws], [torch.as_tensor(b, dtype=torch.float32).to(DEV)
                                        for b in bs]


def hand_off(widths):
    return (torch.full((8 * widths[1],), 3.0, dtype=torch.bfloat16, device=DEV),
            torch.zeros(1, dtype=torch.int32, device=DEV))


def per_layer(x, ws, bs, acts, M, out_dtype, n_cls):
    """The path the kernel replaces: one ops.gemv per layer, ops.softmax_rows after a softmax."""
    h = x
    for l, (w, b, a) in enumerate(zip(ws, bs, acts)):
        last = l == len(ws) - 1
        y = torch.zeros(M, w.shape[0], device=DEV, dtype=out_dtype if last else torch.bfloat16)
        ops.gemv(h, w, b, y, act="linear" if a == "softmax" else a)
        if a == "softmax":
            ops.softmax_rows(y, y, n_cls)
        h = y
    return h.cpu()


@pytest.mark.parametrize("last", ["bf16", "f32", "softmax"])
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: f"{w[0]}x{len(w) - 1}")
@pytest.mark.parametrize("M", ROWS)
def test_bits_of_the_per_layer_path_and_fp64_bound(M, widths, last):
    L = len(widths) - 1
    acts = [HIDDEN[(l + M) % 3] for l in range(L - 1)] + ["softmax" if last == "softmax"
                                                          else "linear"]
    dt, n_cls = (torch.bfloat16 if last == "bf16" else torch.float32), 10
    x64, ws64, bs64 = sc.random_case(M, widths, seed=M + L)
    x, ws, bs = operands(x64, ws64, bs64)
    want = per_layer(x, ws, bs, acts, M, dt, n_cls)
    work, counter = hand_off(widths)
    outs = []
    for _ in range(3):  # the same workspace and counter, no reset in between
        ybuf, y = padded(M, widths[-1], dt, SENT, DEV)
        ops.stage_gemv(x, ws, bs, acts, y, work, counter, n_cls=n_cls)
        torch.cuda.synchronize()
        assert int(counter.item()) == 0
        assert_padding_untouched(ybuf, M, widths[-1])
        outs.append(y.cpu())
    cols = n_cls if last == "softmax" else widths[-1]
    for y in outs:
        assert torch.equal(y[:, :cols].view(torch.int16 if last == "bf16" else torch.int32),
                           want[:, :cols].view(torch.int16 if last == "bf16" else torch.int32))
        assert bool((y[:, cols:] == SENT).all())  # nothing beyond the classes
    got = outs[0].double().numpy()
    z, e = sc.chain64(x64, ws64, [b.double().cpu().numpy() for b in bs],
                      acts[:-1] + ["linear"], out_bf16=last == "bf16")
    if last == "softmax":  # test_stage_fwd_gpu.test_engine_fused's bound
        p = torch.softmax(torch.as_tensor(z[:, :n_cls]), dim=1).numpy()
        bound = 2 * e[:, :n_cls].max(axis=1, keepdims=True) + 1e-5 * p + 1e-6
        assert (np.abs(got[:, :n_cls] - p) <= bound).all()
    else:
        ratio = float((np.abs(got - z) / e).max())
        print(f"stage_gemv {widths} {acts} rows {M} {dt}: worst error / bound {ratio:.4f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: f"{w[0]}x{len(w) - 1}")
@pytest.mark.parametrize("M", ROWS)
def test_exact_operands_equal_fp64(M, widths):
    acts = ["relu" if l % 2 == 0 else "linear" for l in range(len(widths) - 1)]
    x64, ws64, bs64 = sc.exact_case(M, widths, seed=M + len(widths))
    want, _ = sc.chain64(x64, ws64, bs64, acts, exact=True)
    x, ws, bs = operands(x64, ws64, bs64)
    work, counter = hand_off(widths)
    for dt in (torch.float32, torch.bfloat16):
        ybuf, y = padded(M, widths[-1], dt, SENT, DEV)
        ops.stage_gemv(x, ws, bs, acts, y, work, counter)
        assert np.array_equal(y.double().cpu().numpy(), want), dt
        assert_padding_untouched(ybuf, M, widths[-1])


@pytest.mark.parametrize("M,widths,acts,counter,why", [
    (1, [64, 576, 64], ["relu", "linear"], True, "width 576"),
    (1, [64] * 10, ["relu"] * 9, True, "9 layers"),
    (1, [64, 64, 64], ["softmax", "linear"], True, "hidden softmax"),
    (9, [64, 64, 64], ["relu", "linear"], True, "9 rows"),
    (1, [64, 64, 64], ["relu", "linear"], False, "missing counter")])
def test_refusals_launch_nothing(M, widths, acts, counter, why):
    x = torch.zeros(M, widths[0], dtype=torch.bfloat16, device=DEV)
    ws = [torch.zeros(n, k, dtype=torch.bfloat16, device=DEV) for k, n in zip(widths, widths[1:])]
    y = torch.full((M, widths[-1]), SENT, device=DEV)
    work, cnt = hand_off(widths)
    with pytest.raises(ValueError):
        ops.stage_gemv(x, ws, [None] * len(ws), acts, y, work, cnt if counter else None, n_cls=10)
    torch.cuda.synchronize()
    assert bool((y == SENT).all()) and bool((work == 3.0).all()) and int(cnt.item()) == 0, why


DIMS, ACTS = [784, 512, 256, 128, 10], ["relu", "sigmoid", "relu", "softmax"]


@pytest.mark.parametrize("mode", ["graph", "native"])
@pytest.mark.parametrize("split", [[4], [2, 2]])
def test_engine_fused_equals_layers(mode, split, monkeypatch):
    monkeypatch.setenv("DNN_SERVE_REPLAY", mode)
    L = sc.model_layers(DIMS, ACTS, seed=3)
    stages = [L[sum(split[:i]):sum(split[:i + 1])] for i in range(len(split))]
    a = InferenceEngine(stages, DEV, expected_input=784)
    b = InferenceEngine(stages, DEV, expected_input=784, stage_gemv="fused")
    for rows in (1, 8):
        for rep in range(2):  # the second request replays what the first recorded
            x = np.random.default_rng(rows + rep).standard_normal((rows, 784))
            assert np.array_equal(a.predict(x), b.predict(x)), (rows, rep)
            assert all(st.buffers(rows)["gemv_fused"] for st in b.stages)
            assert not any(st.buffers(rows)["gemv_fused"] for st in a.stages)


def test_engine_wide_softmax_and_fallbacks():
    """100 classes: the kernel with a linear last layer, then ops.softmax_rows. A 9-row request,
    an fp8 stage and a 1024-wide layer never reach the kernel. All bit for bit ``layers``."""
    L = sc.model_layers(DIMS, ACTS, seed=4)
    wide = sc.model_layers([784, 1024, 10], ["relu", "softmax"], seed=5)
    c100 = sc.model_layers([784, 128, 100], ["sigmoid", "softmax"], seed=6)
    for layers, kw, rows, fused in ((c100, {}, 5, True), (L, {}, 9, False),
                                    (L, {"weights": "fp8"}, 8, False), (wide, {}, 8, False)):
        a = InferenceEngine([layers], DEV, expected_input=784, **kw)
        b = InferenceEngine([layers], DEV, expected_input=784, stage_gemv="fused", **kw)
        x = np.random.default_rng(rows).standard_normal((rows, 784))
        assert np.array_equal(a.predict(x), b.predict(x))
        assert b.stages[0].buffers(b._bucket(rows))["gemv_fused"] is fused
    assert not ops.stage_gemv_supported([832, 1024, 64], ["relu", "softmax"], 10)
