"""The gfx950 dense-target loss kernel (csrc/kernels/dense_loss.hip) against the fp64 oracle of
tests/_dense_loss_oracle.py, whose bounds are derived there from the kernel's operation count:
every loss/activation pair, one and several column chunks (also a partial last chunk and an
n_out that is no multiple of 4), 1..300 rows, +-200 pre-activations, padding rows, omitted
outputs, and the element-wise form taken by unaligned views."""
import pytest
import torch

import _dense_loss_oracle as do
from docker_dist_nn_amd import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("width,n_out", do.SHAPES)
def test_dense_loss_fp64(dev, width, n_out):
    stats = do.new_stats()
    do.check_shape(width, n_out, dev, stats)
    print("\n" + do.statline(f"gpu {width}/{n_out}", stats))


def test_dense_loss_reproducible(dev):
    """No atomics: two launches give the same bits in every output."""
    rows, width, n = 300, 832, 784
    case = do.dense_case(rows, n, 77)
    z = torch.zeros(rows, width)
    z[:, :n] = case["z"].float()
    t = torch.zeros(rows, width, dtype=torch.bfloat16)
    t[:, :n] = case["t"].to(torch.bfloat16)
    z, t, ok = z.to(dev), t.to(dev), case["ok"].to(dev)
    nb, nc = ops.dense_loss_row_blocks(rows), ops.dense_loss_col_chunks(width)
    outs = []
    for _ in range(2):
        dz = torch.zeros(rows, width, dtype=torch.bfloat16, device=dev)
        lp = torch.zeros(nb * nc, device=dev)
        cs = torch.zeros(nb, width, device=dev)
        ops.dense_loss(z, t, dz, n, 1.0 / rows, "bce", "sigmoid", row_ok=ok, loss_part=lp,
                       colsum=cs)
        outs.append((dz.cpu(), lp.cpu(), cs.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_dense_loss_preconditions(dev):
    """Host-side checks of the launcher: a failed precondition raises, nothing is launched."""
    from docker_dist_nn_amd.utils.native import native

    n = native()
    z = torch.zeros(64, 64, device=dev)
    t = torch.zeros(64, 64, dtype=torch.bfloat16, device=dev)
    dz = torch.full((64, 64), 5.0, dtype=torch.bfloat16, device=dev)

    def call(**kw):
        a = dict(z=z.data_ptr(), ld_z=64, t=t.data_ptr(), ld_t=64, row_ok=0, dz=dz.data_ptr(),
                 ld_dz=64, rows=64, n_out=10, width=64, loss=1, act=0, scale=1.0, loss_part=0,
                 colsum=0, ld_colsum=0, stream=torch.cuda.current_stream(dev).cuda_stream)
        a.update(kw)
        n.dense_loss(**a)

    for bad in (dict(width=96), dict(n_out=65), dict(n_out=0), dict(rows=0), dict(ld_dz=32),
                dict(ld_z=8), dict(ld_t=8), dict(loss=2, act=0), dict(loss=2, act=1),
                dict(loss=1, act=3), dict(loss=0), dict(z=0), dict(colsum=z.data_ptr(),
                                                                  ld_colsum=32)):
        with pytest.raises(ValueError):
            call(**bad)
    torch.cuda.synchronize(dev)
    assert bool((dz == 5.0).all())
    call()
    torch.cuda.synchronize(dev)
    assert bool((dz == 0).all())
