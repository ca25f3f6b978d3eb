"""The optimizer update whole (Stage.optimizer_step) and split over layer ranges
(Stage.update_layers) are the same update, bit for bit, and the step counter set by set_step is
the one Adam's bias correction uses (see _optimizer_paths.py for the model and the steps)."""
import pytest
import torch

import _optimizer_paths as P
from docker_dist_nn_amd import ops

CPU = torch.device("cpu")


@pytest.mark.parametrize("opt", P.OPTS, ids=P.OPT_IDS)
def test_split_update_equals_whole_update(opt):
    P.assert_same(P.train(CPU, opt, split=False), P.train(CPU, opt, split=True))


def test_set_step_is_the_step_adam_corrects_for():
    n, lr, opt = 5, 3e-3, P.OPTS[1]
    real = P.make_stage(CPU, opt)
    for _ in range(2):
        P.gradients(real)
        real.optimizer_step(lr)
    st = P.make_stage(CPU, opt)
    st.params.set_step(2)
    assert st.params.step_count == real.params.step_count == 2
    st.params.set_step(n)
    P.gradients(st)
    p, o = st.params, st.params.optim
    want = {}
    for step in (1, n + 1):
        master, m, v = p.master.clone(), p.state[0].clone(), p.state[1].clone()
        ops.adam_update(master, p.grad, m, v, p.shadow.clone(), lr=lr, betas=o.betas, eps=o.eps,
                        weight_decay=o.weight_decay, decoupled=False, step=step)
        want[step] = master
    st.optimizer_step(lr)
    assert p.step_count == n + 1
    assert torch.equal(p.master, want[n + 1]) and not torch.equal(p.master, want[1])
