"""bench.py's options around the headline run: ``--full`` (the comparison measurements, off by
default), ``--dump-outputs DIR`` (the last timed step's results as .npy files) and the fields
of the result line the step count of later measurements is chosen by."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    sp = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(b)
    return b


def test_plain_run_is_the_default(bench):
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs == "" and (a.steps, a.warmup) == (7, 2)
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


@pytest.mark.gpu
def test_dump_outputs_same_arguments_same_arrays(bench, tmp_path, capsys):
    """Two runs with the same arguments write the same arrays (seeded weights, data and batch
    order; the step is deterministic), in float32 / float64, finite, and the result line
    reports the timed steps asked for and the time of one."""
    from docker_dist_nn_amd import NAMED_MODELS

    dims = [(l.out_dim, l.in_dim) for l in NAMED_MODELS["mnist-fcnn"].layers]
    runs = []
    for tag in ("a", "b"):
        d = tmp_path / tag
        assert bench.main(["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "1024",
                           "--dump-outputs", str(d)]) == 0
        lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        out = json.loads(lines[0])
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
        # (ms_per_step is printed to 1e-4 ms: ~1 % of a step this small)
        assert out["value"] == pytest.approx(1024 / (out["ms_per_step"] * 1e-3), rel=2e-2)
        arrs = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
        assert sorted(arrs) == sorted([f"w{k}" for k in range(len(dims))] +
                                      [f"b{k}" for k in range(len(dims))] + ["loss"])
        for k, (o, i) in enumerate(dims):
            assert arrs[f"w{k}"].shape == (o, i) and arrs[f"w{k}"].dtype == np.float32
            assert arrs[f"b{k}"].shape == (o,) and arrs[f"b{k}"].dtype == np.float32
        assert arrs["loss"].dtype == np.float64
        assert float(arrs["loss"][0]) == pytest.approx(out["last_loss"], abs=1e-5)
        assert all(np.isfinite(v).all() for v in arrs.values())
        assert sum(v.nbytes for v in arrs.values()) < 64 << 20
        runs.append(arrs)
    for name in runs[0]:
        assert np.array_equal(runs[0][name], runs[1][name]), name
