"""test_optimizer_paths_cpu.py's comparison on the GPU, through the recorded segments: replaying
O against O0-1 + O1-3 + OADV gives the same weights, shadow and optimizer state bit for bit,
and the device step counter follows the host's."""
import pytest
import torch

import _optimizer_paths as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("opt", P.OPTS, ids=P.OPT_IDS)
def test_gpu_split_segments_equal_whole_segment(dev, opt):
    whole = P.train(dev, opt, split=False, native=True)
    split = P.train(dev, opt, split=True, native=True)
    segs = whole[0]._prog.segments()
    assert {"O", "O0-1", "O1-3", "OADV"} <= set(segs)
    P.assert_same(whole, split)
    if opt["name"] != "sgd":
        for st, _ in (whole, split):
            assert int(st.params.step_dev[0]) == st.params.step_count == len(P.LRS)


def test_gpu_set_step_reaches_the_device_counter(dev):
    st = P.make_stage(dev, P.OPTS[1], native=True)
    st.params.set_step(5)
    P.gradients(st)
    st.optimizer_step(3e-3)
    assert int(st.params.step_dev[0]) == st.params.step_count == 6
