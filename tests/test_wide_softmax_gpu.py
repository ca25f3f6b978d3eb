"""The wide softmax kernels (csrc/kernels/softmax_wide.hip: softmax_xent and softmax_rows beyond
256 columns) against the fp64 oracle: lo's comparators and sentinel checks as they are, and the
tight bounds of tests/_wide_softmax_oracle.py derived from the kernel's own addition chain.
Shapes cross every boundary of the sweep: one column past the narrow kernels (257), a full
width (320/320), several 1024-column sweeps (1025, 2101), a last 4-column group partly beyond
n_cls (2101), a width that is no multiple of 64 (300) -- with 1, 63, 64, 65 and 300 rows (a
partial last block behind an all-padding one)."""
import pytest
import torch

import _loss_oracle as lo
import _wide_softmax_oracle as wo
from docker_dist_nn_amd import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("width,n_cls", wo.WIDE_SHAPES)
def test_softmax_xent_wide_fp64(dev, width, n_cls):
    stats, tight = lo.new_stats(), lo.new_stats()
    for rows in lo.XENT_ROWS:
        case = wo.wide_case(rows, n_cls, seed=rows + n_cls)
        for scale in (1.0, 1.0 / rows):
            wo.check_softmax_xent(case, width, scale, dev, tight, lo_stats=stats)
        wo.check_softmax_xent(case, width, 1.0 / rows, dev, tight, lo_stats=stats, colsum=False)
        wo.check_softmax_xent(case, width, 1.0, dev, tight, lo_stats=stats, loss=False,
                              correct=False)
    print("\n" + lo.statline(f"gpu softmax_xent wide {width}/{n_cls}", stats))
    print(lo.statline(f"gpu softmax_xent wide {width}/{n_cls} tight D={wo.kernel_depth(n_cls)}",
                      tight))


@pytest.mark.parametrize("width,n_cls", wo.WIDE_SHAPES)
def test_softmax_xent_wide_layouts_bitwise_equal(dev, width, n_cls):
    """Contiguous tensors and lo's padded views take the 16-/8-byte path, a view shifted by one
    column the scalar one: all three give the same bits, each inside the tight bounds, and a
    second launch repeats them."""
    rows = 300
    case = wo.wide_case(rows, n_cls, seed=7 * width + n_cls)
    outs = {}
    for layout in wo.LAYOUTS:
        outs[layout] = wo.run_softmax_xent(case, width, 1.0 / rows, dev, layout)
        wo.judge_softmax_xent(outs[layout], case, width, 1.0 / rows)
    again = wo.run_softmax_xent(case, width, 1.0 / rows, dev, "plain")
    for other in (outs["padded"], outs["shifted"], again):
        for k in ("dz", "loss", "corr"):
            assert torch.equal(outs["plain"][k], other[k]), f"{other['what']}: {k} differs"
        assert torch.equal(outs["plain"]["cs"][:5, :width], other["cs"][:5, :width]), \
            f"{other['what']}: colsum differs"


@pytest.mark.parametrize("width,n_cls", wo.NARROW_SHAPES)
def test_narrow_widths_stay_on_the_narrow_kernels(dev, width, n_cls):
    """Up to 256 columns nothing changes: lo's comparators pass as before and the outputs are
    bitwise those of every layout (the narrow kernel has one path), inside bounds of depth
    n_cls - 1 (its own chain is not the wide kernel's)."""
    rows = 300
    case = lo.logits_case(rows, n_cls, seed=rows + n_cls)
    lo.check_softmax_xent(case, width, 1.0 / rows, dev)
    a = wo.run_softmax_xent(case, width, 1.0 / rows, dev, "plain")
    b = wo.run_softmax_xent(case, width, 1.0 / rows, dev, "padded")
    wo.judge_softmax_xent(a, case, width, 1.0 / rows, depth=n_cls - 1)
    for k in ("dz", "loss", "corr"):
        assert torch.equal(a[k], b[k]), k


def test_existing_narrow_shapes_still_pass(dev):
    for width, n_cls in lo.XENT_SHAPES:
        case = lo.logits_case(65, n_cls, seed=65 + n_cls)
        lo.check_softmax_xent(case, width, 1.0 / 65, dev)


@pytest.mark.parametrize("n_cls", wo.ROWS_CLS)
def test_softmax_rows_wide_fp64(dev, n_cls):
    stats = lo.new_stats()
    for rows in lo.ROWS_ROWS:
        case = wo.wide_case(rows, n_cls, seed=3 * rows + n_cls)
        wo.check_softmax_rows(case, dev, stats)
        wo.check_softmax_rows(case, dev, stats, inplace=True)
    wo.check_softmax_rows(case, dev, out=False)
    wo.check_softmax_rows(case, dev, labels=False)
    wo.check_softmax_rows(case, dev, pred=False)
    wo.check_softmax_rows(case, dev, base=7)  # the counter accumulates onto what it held
    print("\n" + lo.statline(f"gpu softmax_rows wide /{n_cls} D={wo.kernel_depth(n_cls)}",
                             stats))


def test_softmax_rows_wide_aligned_rows(dev):
    """A contiguous [rows][1024] buffer (16-byte rows: the vector path, the padded views of the
    other tests have odd leading dimensions at 257 / 1025 / 2101) with 1000 classes, in place:
    columns 1000.. keep what they held."""
    rows, n_cls = 65, 1000
    case = wo.wide_case(rows, n_cls, seed=11)
    buf = torch.full((rows, 1024), 3.0)
    buf[:, :n_cls] = case["x"].float()
    buf = buf.to(dev)
    pred = torch.zeros(rows, dtype=torch.int32, device=dev)
    ops.softmax_rows(buf, buf, n_cls, None, pred, None)
    ref = lo.xent_ref(case["x"], case["labels"], 1.0)
    wo.assert_probs_tight(buf[:, :n_cls], ref, what="softmax_rows 65x1024 in place")
    assert bool((buf[:, n_cls:] == 3.0).all()) and torch.equal(pred.cpu().long(), ref["argmax"])
