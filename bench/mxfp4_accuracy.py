"""What the serving weight formats cost in accuracy, reported and not gated: top-1 agreement and
mean absolute logit difference of the fp8 and the mxfp4 engine against the bf16 engine, on the
same model and the same inputs. The model is the mnist-fcnn MLP (784-512-256-128-10) trained for
``--steps`` SGD steps on the synthetic teacher-labelled MNIST-shaped set (data.synthetic_mnist,
what ``run_grpc_inference.py --local`` is pointed at when no real data is present); the inputs
are ``--rows`` held-out rows of that set, sent in requests of 8 rows (the GEMV path, which reads
the codes in place) and as one batch (the large-bucket path); the mxfp4 engine with
``mxfp4_gemm="w4a8"`` (fp8 activations against the codes) is one more contender, in requests of
64 rows. The last layer is served as
``linear`` so that logits, not probabilities, are compared. One JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from docker_dist_nn_amd import NAMED_MODELS  # noqa: E402
from docker_dist_nn_amd.config import LayerWeights  # noqa: E402
from docker_dist_nn_amd.data import synthetic_mnist  # noqa: E402
from docker_dist_nn_amd.engine import OptimConfig, Trainer  # noqa: E402
from docker_dist_nn_amd.engine.inference import InferenceEngine  # noqa: E402


def train(spec, steps, dev):
    tr = Trainer(spec, micro_batch=256, num_micro=2, optim=OptimConfig(lr=0.1), device=dev)
    x, y = synthetic_mnist(512 * 16, seed=0)
    xb = torch.zeros(len(x), tr.stages[0].x_in.shape[1], dtype=torch.bfloat16, device=dev)
    xb[:, :784] = torch.from_numpy(x).to(dev, torch.bfloat16)
    yb = torch.from_numpy(y).to(dev)
    for s in range(steps):
        k = (s % 16) * 512
        tr.set_batch(xb[k:k + 512], yb[k:k + 512])
        tr.step()
    loss = tr.loss()
    ww = tr.local_weights()
    return [ww[i] for i in range(len(spec.layers))], float(loss)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--out", type=str, default="", help="also append the line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mxfp4_accuracy needs a GPU: the engines under test run there")
    dev = torch.device("cuda:0")
    spec = NAMED_MODELS["mnist-fcnn"]
    ww, loss = train(spec, a.steps, dev)
    n = len(ww)
    layers = [LayerWeights(ww[i][0], ww[i][1], "linear" if i == n - 1 else "relu")
              for i in range(n)]
    x, labels = synthetic_mnist(a.rows, seed=1)
    out = {"case": "serving_format_accuracy", "model": "mnist-fcnn", "train_steps": a.steps,
           "train_loss": round(loss, 4), "rows": a.rows}
    logits = {}
    for fmt in ("bf16", "fp8", "mxfp4"):
        eng = InferenceEngine([layers], dev, expected_input=784, weights=fmt)
        small = np.concatenate([eng.predict(x[k:k + 8]) for k in range(0, a.rows, 8)])
        logits[fmt] = {"rows8": small, "batch": eng.predict(x)}
        out[f"{fmt}_resident_weight_bytes"] = eng.resident_weight_bytes()
        out[f"{fmt}_top1_vs_labels"] = round(float((small.argmax(1) == labels).mean()), 4)
    # mxfp4 codes against fp8 activations (--mxfp4-gemm w4a8), in requests of 64 rows: the bucket
    # its MFMA path serves; against the bf16 engine on the same requests
    rows64 = {}
    for name, kw in (("bf16", {}), ("mxfp4_w4a8", {"weights": "mxfp4", "mxfp4_gemm": "w4a8"})):
        eng = InferenceEngine([layers], dev, expected_input=784, **kw)
        rows64[name] = np.concatenate([eng.predict(x[k:k + 64]) for k in range(0, a.rows, 64)])
    got, want = rows64["mxfp4_w4a8"], rows64["bf16"]
    out["mxfp4_w4a8_top1_vs_labels"] = round(float((got.argmax(1) == labels).mean()), 4)
    out["mxfp4_w4a8_rows64_top1_agreement"] = round(
        float((got.argmax(1) == want.argmax(1)).mean()), 4)
    out["mxfp4_w4a8_rows64_mean_abs_logit_diff"] = round(float(np.abs(got - want).mean()), 5)
    out["bf16_mean_abs_logit"] = round(float(np.abs(logits["bf16"]["rows8"]).mean()), 4)
    for fmt in ("fp8", "mxfp4"):
        for path in ("rows8", "batch"):
            got, want = logits[fmt][path], logits["bf16"][path]
            out[f"{fmt}_{path}_top1_agreement"] = round(
                float((got.argmax(1) == want.argmax(1)).mean()), 4)
            out[f"{fmt}_{path}_mean_abs_logit_diff"] = round(float(np.abs(got - want).mean()), 5)
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
