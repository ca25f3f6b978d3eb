"""Shared by test_optimizer_paths_{cpu,gpu}.py: three full training steps of the model
70-96-40-10 held by ONE Stage (64 rows, one micro-batch: several layers, padded widths, both
Adam moments), with a learning rate that changes every step, the optimizer update done either
whole (Stage.optimizer_step) or split (Stage.update_layers over [0, 1) without and [1, 3) with
the step advance). The two must agree bit for bit."""
import torch

from docker_dist_nn_amd.engine import OptimConfig, Stage
from docker_dist_nn_amd.models.mlp import MLPSpec

SPEC = MLPSpec.parse("70-96-40-10")
ROWS = 64
LRS = (1e-2, 4e-3, 7e-3)
OPTS = [dict(name="sgd", momentum=0.9, weight_decay=1e-4),
        dict(name="adam", weight_decay=1e-4),
        dict(name="adamw", weight_decay=1e-2)]
OPT_IDS = [o["name"] for o in OPTS]

_gen = torch.Generator().manual_seed(11)
X = torch.zeros(ROWS, 128, dtype=torch.bfloat16)  # 70 inputs padded to the GEMM's K tile
X[:, :70] = torch.randn(ROWS, 70, generator=_gen).to(torch.bfloat16)
Y = torch.randint(0, 10, (ROWS,), generator=_gen, dtype=torch.int32)


def make_stage(device, opt, native=False):
    st = Stage(SPEC, 0, 3, micro_batch=ROWS, num_micro=1, device=device,
               optim=OptimConfig(lr=LRS[0], **opt))
    assert st.x_buf.shape == X.shape
    st.params.init_default(3)
    if native:
        st.compile_native()
    return st


def gradients(st):
    """One forward / backward / wgrad / gradient reduction of the fixed batch."""
    st.set_batch(X.to(st.device), Y.to(st.device))
    st.begin_step()
    st.forward(0)
    st.backward(0)
    st.wgrad()
    st.finalize_grads()


def train(device, opt, split, native=False):
    """(stage, losses) after one step per rate of LRS."""
    st = make_stage(device, opt, native)
    losses = []
    for lr in LRS:
        gradients(st)
        if split:
            st.update_layers(0, 1, lr, advance=False)
            st.update_layers(1, 3, lr, advance=True)
        else:
            st.optimizer_step(lr)
        losses.append(st.loss_sum())
    return st, losses


def assert_same(a, b):
    (sa, la), (sb, lb) = a, b
    pa, pb = sa.params, sb.params
    assert la == lb
    assert torch.equal(pa.master, pb.master) and torch.equal(pa.shadow, pb.shadow)
    assert len(pa.state) == len(pb.state) == (1 if pa.optim.name == "sgd" else 2)
    for x, y in zip(pa.state, pb.state):
        assert torch.equal(x, y)
    assert pa.step_count == pb.step_count == len(LRS)
    # the weights moved, so equality says something
    fresh = make_stage(sa.device, dict(name=pa.optim.name))
    assert not torch.equal(pa.master, fresh.params.master)
