"""Flat parameter / gradient buffers of a stage's layers: layout and views, load / init /
export, W^T shadows and the sharded-DP pieces. What an update IS belongs to the optimizer
(engine/optimizer.py); this module knows over which ranges it runs and which W^T it stales."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from .. import ops
from ..models.mlp import LayerGeom, round_up
from .optimizer import OptimConfig, Optimizer

_ALIGN = 64  # elements; keeps every layer's region 256-B aligned
# Bias of the padding units of a sigmoid layer (width not a multiple of 64). With a zero bias they
# would output sigmoid(0) = 0.5, the next layer's padded weight columns would receive the gradient
# 0.5 * sum(dZ) and stop being zero: the padded model would drift away from the specified one (and
# from what export() returns). At this bias their output is exactly 0 and so is their derivative
# y (1 - y): every gradient of the padding stays exactly 0. Weight decay (and an L2 term under
# Adam) would move the entries like any other bias, so every update is followed by
# StageParams.pin_padding, which writes them back: the off-state does not depend on the step
# count. A power of two: exact in bf16 (the pin's source) and fp32; its square is finite.
PAD_OFF_BIAS = -2.0 ** 50


def _of_opt(name: str) -> property:
    """Read-only ``params.opt.<name>`` (checkpointing, tests and bench scripts read these)."""
    return property(lambda self: getattr(self.opt, name))


class StageParams:
    """Flat parameter / gradient / optimizer buffers of a stage's layers."""

    def __init__(self, geoms: Sequence[LayerGeom], device: torch.device,
                 optim: Optional[OptimConfig] = None, shard: Optional[tuple[int, int]] = None):
        self.geoms = list(geoms)
        self.device = device
        # sharded data parallelism (shard = (dp, dp_rank), see shard_piece): every layer's
        # region ends on a multiple of dp * _ALIGN, so any bucket of whole layers splits into
        # dp equal, aligned pieces
        self.sharded = shard is not None
        self.dp, self.dp_rank = shard or (1, 0)
        off = 0
        self.w_off, self.b_off = [], []
        if self.sharded:
            # weights first, each padded to dp pieces; then every bias (replicated update)
            for g in self.geoms:
                self.w_off.append(off)
                off = round_up(off + g.np_ * g.kp, _ALIGN * self.dp)
            self.bias_lo = off
            for g in self.geoms:
                self.b_off.append(off)
                off = round_up(off + g.np_, _ALIGN)
        else:
            for g in self.geoms:
                self.w_off.append(off)
                off = round_up(off + g.np_ * g.kp, _ALIGN)
                self.b_off.append(off)
                off = round_up(off + g.np_, _ALIGN)
        self.numel = off
        self.master = torch.zeros(off, dtype=torch.float32, device=device)
        self.shadow = torch.zeros(off, dtype=torch.bfloat16, device=device)
        self.grad = torch.zeros(off, dtype=torch.float32, device=device)
        if self.sharded:
            # bf16 gradient (reduce-scatter input) and the reduced pieces this rank owns: the
            # piece of bucket [e0, e1) lives at [e0 / dp, e1 / dp) of grad_piece
            self.grad16 = torch.zeros(off, dtype=torch.bfloat16, device=device)
            self.grad_piece = torch.zeros(off // self.dp, dtype=torch.bfloat16, device=device)
            self.shard_buckets: list[tuple[int, int]] = []
        self.opt = Optimizer(optim or OptimConfig(), self.master, self.grad, self.shadow)
        # transposed bf16 weight shadows W^T[Kp][Np] of the layers whose dgrad reads them
        # (enable_wt); refreshed after every update of their layer (refresh_t)
        self.wt: dict[int, torch.Tensor] = {}
        # padding-unit biases held at PAD_OFF_BIAS: layer -> (fp32 master entries, bf16 shadow
        # entries, bf16 source of the pin), each [1][np_ - out_dim]
        self.pad_pins: dict[int, tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = {}
        for i, g in enumerate(self.geoms):
            n = g.np_ - g.spec.out_dim
            if g.spec.activation == "sigmoid" and n:
                lo = self.b_off[i] + g.spec.out_dim
                self.pad_pins[i] = (self.master[lo:lo + n].view(1, n),
                                    self.shadow[lo:lo + n].view(1, n),
                                    torch.full((1, n), PAD_OFF_BIAS, dtype=torch.bfloat16,
                                               device=device))
        # layers whose weight gradient GEMM applies the SGD step itself (Stage.enable_fused_
        # wgrad_update): the per-step update paths below skip their weights and W^T
        self.fused_layers: set[int] = set()

    optim = _of_opt("cfg")
    state = _of_opt("state")
    step_count = _of_opt("step_count")
    lr_dev = _of_opt("lr_dev")
    step_dev = _of_opt("step_dev")

    def set_lr(self, lr: float) -> None:
        self.opt.arm(lr)

    def set_step(self, n: int) -> None:
        self.opt.set_step(n)

    # views ------------------------------------------------------------------------------
    def w32(self, i):
        g = self.geoms[i]
        return self.master[self.w_off[i]:self.w_off[i] + g.np_ * g.kp].view(g.np_, g.kp)

    def b32(self, i):
        return self.master[self.b_off[i]:self.b_off[i] + self.geoms[i].np_]

    def wbf(self, i):
        g = self.geoms[i]
        return self.shadow[self.w_off[i]:self.w_off[i] + g.np_ * g.kp].view(g.np_, g.kp)

    def gw(self, i):
        g = self.geoms[i]
        return self.grad[self.w_off[i]:self.w_off[i] + g.np_ * g.kp]

    def gb(self, i):
        return self.grad[self.b_off[i]:self.b_off[i] + self.geoms[i].np_]

    def layer_grad_range(self, i) -> tuple[int, int]:
        """Flat [start, end) of layer i's W and b gradients (a DP all-reduce bucket). Sharded
        layout: layer i's WEIGHTS only (the biases live together at [bias_lo, numel))."""
        if self.sharded:
            return self.w_off[i], (self.w_off[i + 1] if i + 1 < len(self.geoms)
                                   else self.bias_lo)
        end = self.w_off[i + 1] if i + 1 < len(self.geoms) else self.numel
        return self.w_off[i], end

    def layers_range(self, a: int, b: int) -> tuple[int, int]:
        """Flat [start, end) of layers a..b-1 (weights, biases and alignment padding)."""
        if self.sharded:
            raise ValueError("sharded layout: layer ranges are not contiguous")
        return self.w_off[a], (self.w_off[b] if b < len(self.geoms) else self.numel)

    # weights in/out -----------------------------------------------------------------------
    def _load_flat(self, buf: torch.Tensor, weights: Sequence[np.ndarray],
                   biases: Sequence[np.ndarray], what: str) -> None:
        buf.zero_()
        for i, g in enumerate(self.geoms):
            w = torch.as_tensor(np.asarray(weights[i], dtype=np.float32))
            b = torch.as_tensor(np.asarray(biases[i], dtype=np.float32))
            if tuple(w.shape) != (g.spec.out_dim, g.spec.in_dim):
                raise ValueError(f"layer {g.index}: {what} shape {tuple(w.shape)} != "
                                 f"{(g.spec.out_dim, g.spec.in_dim)}")
            view = buf[self.w_off[i]:self.w_off[i] + g.np_ * g.kp].view(g.np_, g.kp)
            view[:g.spec.out_dim, :g.spec.in_dim] = w.to(self.device)
            buf[self.b_off[i]:self.b_off[i] + g.spec.out_dim] = b.to(self.device)

    def load(self, weights: Sequence[np.ndarray], biases: Sequence[np.ndarray]) -> None:
        """Set from unpadded [out][in] weights / [out] biases (any float dtype)."""
        self._load_flat(self.master, weights, biases, "weight")
        self.refresh_shadow()  # (pins the padding biases too)

    def init_default(self, seed: int) -> None:
        """nn.Linear default init, U(-1/sqrt(in), 1/sqrt(in)); seeded by GLOBAL layer index so
        any stage split of the same model starts from identical weights."""
        ws, bs = [], []
        for g in self.geoms:
            gen = torch.Generator().manual_seed(seed * 7919 + g.index)
            bound = 1.0 / math.sqrt(g.spec.in_dim)
            ws.append((torch.rand(g.spec.out_dim, g.spec.in_dim, generator=gen) * 2 - 1) * bound)
            bs.append((torch.rand(g.spec.out_dim, generator=gen) * 2 - 1) * bound)
        self.load([w.numpy() for w in ws], [b.numpy() for b in bs])

    def refresh_shadow(self) -> None:
        self.shadow.copy_(self.master.to(torch.bfloat16))
        self.refresh_t()

    def enable_wt(self, i: int) -> None:
        g = self.geoms[i]
        if i not in self.wt:
            self.wt[i] = torch.zeros(g.kp, g.np_, dtype=torch.bfloat16, device=self.device)
            ops.transpose_bf16(self.wbf(i), self.wt[i])

    def refresh_t(self, a: int = 0, b: Optional[int] = None, step: bool = False,
                  skip: frozenset = frozenset()) -> None:
        """Re-derive W^T of the local layers [a, b) that keep one (after their update), and
        re-pin their padding biases (pin_padding).
        ``step``: a per-step update -- layers updated by their wgrad epilogue (which writes
        W^T itself) are skipped; so are the ``skip`` layers (W^T written by the update)."""
        b = len(self.geoms) if b is None else b
        ops.transpose_multi([(self.wbf(i), self.wt[i]) for i in range(a, b) if i in self.wt and
                             i not in skip and not (step and i in self.fused_layers)])
        self.pin_padding(a, b)

    def pin_padding(self, a: int = 0, b: Optional[int] = None) -> None:
        """Write the padding-unit biases of the sigmoid layers in [a, b) back to PAD_OFF_BIAS
        (master and shadow): two copy launches per such layer, none for any other model. Runs
        after every update of those layers (through refresh_t), so it is recorded / captured
        with the update it follows."""
        b = len(self.geoms) if b is None else b
        for i in range(a, b):
            if i in self.pad_pins:
                m, sh, src = self.pad_pins[i]
                ops.unpack_bf16(src, m)
                ops.pack_bf16(m, sh)

    def _layers_of(self, e0: int, e1: int) -> tuple[int, int]:
        """Local layers whose parameters lie in the flat element range [e0, e1)."""
        ls = [i for i in range(len(self.geoms)) if self.w_off[i] < e1 and
              self.b_off[i] + self.geoms[i].np_ > e0]
        return (ls[0], ls[-1] + 1) if ls else (0, 0)

    def _export_flat(self, buf: torch.Tensor) -> tuple[list[np.ndarray], list[np.ndarray]]:
        ws, bs = [], []
        for i, g in enumerate(self.geoms):
            w = buf[self.w_off[i]:self.w_off[i] + g.np_ * g.kp].view(g.np_, g.kp)
            ws.append(w[:g.spec.out_dim, :g.spec.in_dim].detach().cpu().numpy().copy())
            bs.append(buf[self.b_off[i]:self.b_off[i] + g.spec.out_dim]
                      .detach().cpu().numpy().copy())
        return ws, bs

    def export(self) -> tuple[list[np.ndarray], list[np.ndarray]]:
        return self._export_flat(self.master)

    def export_state(self, k: int) -> tuple[list[np.ndarray], list[np.ndarray]]:
        """Unpadded per-layer view of optimizer state buffer k (momentum / Adam m, v)."""
        return self._export_flat(self.state[k])

    def load_state(self, k: int, weights: Sequence[np.ndarray],
                   biases: Sequence[np.ndarray]) -> None:
        """Set optimizer state buffer k from unpadded per-layer arrays (padding stays 0)."""
        self._load_flat(self.state[k], weights, biases, "state")

    # optimizer update ---------------------------------------------------------------------
    # The launches of an update, the same whether run eagerly, recorded into a native Program
    # or captured in a graph; the host side of a step (Optimizer.arm before, commit after) is
    # the caller's.
    def _unfused_ranges(self) -> list[tuple[int, int]]:
        """[0, numel) minus the weight regions of fused_layers (updated by their wgrad)."""
        cuts = sorted((self.w_off[i], self.w_off[i] + self.geoms[i].np_ * self.geoms[i].kp)
                      for i in self.fused_layers)
        out, lo = [], 0
        for a, b in cuts:
            if a > lo:
                out.append((lo, a))
            lo = b
        if lo < self.numel:
            out.append((lo, self.numel))
        return out

    def update(self) -> None:
        """The whole step's update: one launch (one per range between fused layers), the
        step-counter advance, W^T."""
        for a, b in self._unfused_ranges():
            self.opt.apply(a, b)
        self.opt.record_advance()
        self.refresh_t(step=True)

    def update_range(self, a: int, b: int, advance: bool, refresh: bool = True) -> None:
        """Update of the flat element range [a, b) only (a DP bucket of whole layers); the
        step counter advances only when ``advance`` (once per step: the last range of a split
        update). ``refresh=False``: leave W^T alone (a shard piece, whose layers are complete
        only after the all-gather)."""
        self.opt.apply(a, b)
        if advance:
            self.opt.record_advance()
        if refresh:
            self.refresh_t(*self._layers_of(a, b))

    def epilogue_args(self, i: int) -> dict:
        """``upd=`` of ops.linear_wgrad for the fused layer i."""
        return self.opt.epilogue_args(self.w32(i), self.wbf(i), self.w_off[i])

    # sharded data parallelism --------------------------------------------------------------
    # Per bucket [e0, e1) of whole layers' WEIGHTS: the fp32 gradient is cast to bf16
    # (shard_pack), reduce-scattered over the DP group (rank r receives the sum of piece r),
    # cast back into grad[piece] (shard_unpack) and only that piece is updated (fp32 master +
    # optimizer state of the piece are authoritative on this rank); the bf16 shadow is then
    # all-gathered and W^T refreshed. The biases (fp32 in the GEMM epilogues, a few KB) are
    # all-reduced in fp32 and updated on every rank. Bytes on the wire: 2 x (dp-1)/dp x 2 B per
    # weight, half of an fp32 all-reduce, and the optimizer touches 1/dp of the weights.
    def shard_piece(self, e0: int, e1: int) -> tuple[int, int]:
        c = (e1 - e0) // self.dp
        if c * self.dp != e1 - e0:
            raise ValueError("bucket length is not a multiple of the DP degree")
        return e0 + self.dp_rank * c, e0 + (self.dp_rank + 1) * c

    def shard_pack(self, e0: int, e1: int) -> None:
        ops.pack_bf16(self.grad[e0:e1].view(1, -1), self.grad16[e0:e1].view(1, -1))

    def shard_unpack(self, e0: int, e1: int) -> None:
        p0, p1 = self.shard_piece(e0, e1)
        d = self.dp
        ops.unpack_bf16(self.grad_piece[e0 // d:e1 // d].view(1, -1),
                        self.grad[p0:p1].view(1, -1))

    def gather_full(self, group) -> None:
        """All-gather the fp32 master and optimizer state over the DP group: afterwards every
        rank holds the whole (checkpoint / export); a no-op without sharding."""
        if not self.sharded or not self.shard_buckets:
            return
        import torch.distributed as dist

        for buf in [self.master] + list(self.state):
            for e0, e1 in self.shard_buckets:
                p0, p1 = self.shard_piece(e0, e1)
                dist.all_gather_into_tensor(buf[e0:e1], buf[p0:p1].clone(), group=group)
