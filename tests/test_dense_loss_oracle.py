"""Dense-target losses (ops.dense_loss) on the CPU path against the fp64 oracle of
tests/_dense_loss_oracle.py -- the same checks, with the same bounds, that
tests/test_dense_loss_gpu.py applies to the gfx950 kernel."""
import pytest
import torch

import _dense_loss_oracle as do
from _act_oracle import CPU
from docker_dist_nn_amd import ops


@pytest.mark.parametrize("width,n_out", do.SHAPES)
def test_dense_loss_cases_on_cpu_path(width, n_out):
    stats = do.new_stats()
    do.check_shape(width, n_out, CPU, stats)
    print("\n" + do.statline(f"cpu {width}/{n_out}", stats))


def test_matches_torch_losses():
    """No padding rows, scale = 1 / rows: the summed partials are nn.MSELoss / BCEWithLogitsLoss
    (mean reduction) and dz is their gradient with respect to z."""
    rows, width, n = 128, 320, 257
    g = torch.Generator().manual_seed(5)
    z = torch.randn(rows, width, generator=g)
    t = torch.rand(rows, width, generator=g).to(torch.bfloat16)
    acts = {"linear": lambda v: v, "relu": torch.relu, "sigmoid": torch.sigmoid}
    for loss, act in do.PAIRS:
        dz = torch.zeros(rows, width, dtype=torch.bfloat16)
        lp = torch.zeros(ops.dense_loss_row_blocks(rows) * ops.dense_loss_col_chunks(width))
        ops.dense_loss(z, t, dz, n, 1.0 / rows, loss, act, loss_part=lp)
        zz = z[:, :n].clone().requires_grad_()
        want = torch.nn.BCEWithLogitsLoss()(zz, t[:, :n].float()) if loss == "bce" else \
            torch.nn.MSELoss()(acts[act](zz), t[:, :n].float())
        want.backward()
        assert abs(float(lp.double().sum()) / rows - float(want.detach())) <= 1e-6 * float(want.detach())
        torch.testing.assert_close(dz[:, :n].float(), zz.grad, rtol=2 ** -8, atol=1e-9)
        assert bool((dz[:, n:] == 0).all())


def test_argument_validation():
    z = torch.zeros(64, 64)
    t = torch.zeros(64, 64, dtype=torch.bfloat16)
    dz = torch.zeros(64, 64, dtype=torch.bfloat16)
    ops.dense_loss(z, t, dz, 10, 1.0, "mse", "linear")
    for loss, act in [("bce", "linear"), ("bce", "relu"), ("mse", "softmax"), ("bce", "softmax"),
                      ("softmax_ce", "softmax"), ("l1", "linear")]:
        with pytest.raises(ValueError):
            ops.dense_loss(z, t, dz, 10, 1.0, loss, act)
    with pytest.raises(ValueError):  # width not a multiple of 64
        ops.dense_loss(z, t, dz[:, :60], 10, 1.0, "mse", "linear")
    with pytest.raises(ValueError):  # n_out > width
        ops.dense_loss(z, t, dz, 65, 1.0, "mse", "linear")
    with pytest.raises(ValueError):  # one partial per (row block, column chunk)
        ops.dense_loss(z, t, torch.zeros(64, 320, dtype=torch.bfloat16), 10, 1.0, "mse", "linear",
                       loss_part=torch.zeros(1))
    with pytest.raises(ValueError):
        ops.dense_loss(z, t, dz, 10, 1.0, "mse", "linear", colsum=torch.zeros(1, 32))
    with pytest.raises(ValueError):
        ops.dense_loss(z, t, dz, 10, 1.0, "mse", "linear", row_ok=torch.zeros(64))
    with pytest.raises(ValueError):
        ops.dense_loss(z, t.float(), dz, 10, 1.0, "mse", "linear")
