"""The optimizer of one stage: which update kernel runs, with which scalars, over which range
of the stage's flat buffers, and who counts the steps.

On a GPU the learning rate and the number of updates done live in device memory (``lr_dev``,
``step_dev``), so the same launches are valid eagerly, recorded into a native Program or
captured in a HIP graph (by-value Adam bias corrections would be frozen by a capture). The host
protocol around one step is therefore ``arm(lr)`` before its first update launch or replay and
``commit()`` after it; the launches themselves (``apply``, ``record_advance``, the fused forms
built from ``fused_args`` / ``epilogue_args``) carry no per-step host value. On the CPU there
are no device scalars: ``apply`` uses the armed rate and ``step_count + 1``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from .. import ops

OPTIMIZERS = ("sgd", "adam", "adamw")


@dataclass
class OptimConfig:
    name: str = "sgd"
    lr: float = 0.05
    momentum: float = 0.0
    weight_decay: float = 0.0
    betas: tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8
    decoupled: bool = False


class Optimizer:
    """Update of the flat fp32 ``master`` (and its bf16 ``shadow``) from the flat ``grad``."""

    def __init__(self, cfg: OptimConfig, master: torch.Tensor, grad: torch.Tensor,
                 shadow: torch.Tensor):
        if cfg.name not in OPTIMIZERS:
            raise ValueError(f"unknown optimizer {cfg.name!r} ({' | '.join(OPTIMIZERS)})")
        self.cfg = cfg
        self.master, self.grad, self.shadow = master, grad, shadow
        self.is_sgd = cfg.name == "sgd"
        self.decoupled = cfg.decoupled or cfg.name == "adamw"
        # momentum | Adam's first and second moment
        n_state = (1 if cfg.momentum else 0) if self.is_sgd else 2
        self.state = [torch.zeros_like(master) for _ in range(n_state)]
        self.step_count = 0  # whole updates done
        self._lr = float(cfg.lr)  # the armed rate (GPU: what lr_dev holds)
        self.gpu = master.device.type == "cuda"
        self.lr_dev = self.step_dev = None
        if self.gpu:
            self.lr_dev = torch.full((1,), self._lr, dtype=torch.float32, device=master.device)
            self.step_dev = torch.zeros(1, dtype=torch.int32, device=master.device)

    # launches -----------------------------------------------------------------------------
    def apply(self, e0: int, e1: int) -> None:
        """ONE update launch over the flat element range [e0, e1)."""
        c, sl = self.cfg, slice(e0, e1)
        st = [s[sl] for s in self.state]
        if self.is_sgd:
            ops.sgd_update(self.master[sl], self.grad[sl], st[0] if st else None,
                           self.shadow[sl], lr=self._lr, momentum=c.momentum,
                           weight_decay=c.weight_decay, lr_dev=self.lr_dev)
        else:
            step = dict(step_dev=self.step_dev) if self.gpu else dict(step=self.step_count + 1)
            ops.adam_update(self.master[sl], self.grad[sl], st[0], st[1], self.shadow[sl],
                            lr=self._lr, betas=c.betas, eps=c.eps, weight_decay=c.weight_decay,
                            decoupled=self.decoupled, lr_dev=self.lr_dev, **step)

    def record_advance(self) -> None:
        """The device step counter's += 1 (once per step, after its last Adam launch); nothing
        for SGD or on the CPU."""
        if self.gpu and not self.is_sgd:
            ops.step_advance(self.step_dev)

    def fused_args(self) -> dict:
        """``sgd=`` of ops.reduce_multi: this update applied by the gradient reduction's own
        launch (over every element it reduces)."""
        c = self.cfg
        args = dict(grad=self.grad, master=self.master, shadow=self.shadow, lr=c.lr,
                    weight_decay=c.weight_decay, lr_dev=self.lr_dev)
        if self.is_sgd:
            return dict(args, mom=self.state[0] if self.state else None, momentum=c.momentum)
        return dict(args, mom=self.state[0], v=self.state[1], adam=True, betas=c.betas,
                    eps=c.eps, decoupled=self.decoupled, step_dev=self.step_dev)

    def epilogue_args(self, w32: torch.Tensor, wbf: torch.Tensor, off: int) -> dict:
        """``upd=`` of ops.linear_wgrad (SGD): the update of one layer's weights -- the views
        ``w32`` / ``wbf`` at flat offset ``off`` -- applied by its weight gradient GEMM."""
        c = self.cfg
        mom = self.state[0][off:off + w32.numel()].view_as(w32) if self.state else None
        return dict(master=w32, shadow=wbf, lr_dev=self.lr_dev, mom=mom, momentum=c.momentum,
                    weight_decay=c.weight_decay)

    # host protocol of a step --------------------------------------------------------------
    def arm_writes(self, lr: Optional[float] = None) -> bool:
        """Would ``arm(lr)`` write ``lr_dev``? (It must not while an update still reads it.)"""
        return self.gpu and float(self.cfg.lr if lr is None else lr) != self._lr

    def arm(self, lr: Optional[float] = None) -> None:
        """This step's learning rate (default: the config's), before its first update launch
        or replay; the device scalar is written only when the rate changed."""
        write = self.arm_writes(lr)
        self._lr = float(self.cfg.lr if lr is None else lr)
        if write:
            self.lr_dev.fill_(self._lr)

    def commit(self) -> None:
        """One whole update was launched."""
        self.step_count += 1

    def set_step(self, n: int) -> None:
        """Number of updates done (checkpoint resume): host counter and device counter."""
        self.step_count = int(n)
        if self.step_dev is not None:
            self.step_dev.fill_(int(n))

    def restore_count(self, n: int) -> None:
        """Host counter only (launches nothing): the caller has put the device side right."""
        self.step_count = int(n)

    def tensors(self) -> list[torch.Tensor]:
        """Every device tensor of the optimizer (state snapshots)."""
        return self.state + ([self.lr_dev, self.step_dev] if self.gpu else [])
