"""How a network ends: the loss head of the last pipeline stage.

A head runs, for micro-batch j, the forward of the stage's last layer(s), the loss, and
whatever part of the backward pass its kernel fuses in; it owns the label / target slots and the
loss partials. This module is the only place in ``engine/`` that knows which heads exist and
when each is chosen (:meth:`LossHead.choose`):

=============  ==========================================  =====================================
head           chosen when                                 launches for micro-batch j
=============  ==========================================  =====================================
TailHead       GEMM-fused CE possible, GPU, >= 3 local     ops.mlp_tail: forward of layers L-2
               layers of a geometry ops.tail_supported     and L-1, CE, dgrads of L-1 and L-2
               takes, DNN_TAIL=1
FusedXentHead  softmax_ce, 64 or 128 padded classes,       ops.linear_fwd_xent (logits never
               DNN_FUSED_XENT=1                            exist in memory)
XentHead       any other softmax_ce                        ops.linear_fwd to fp32 logits +
                                                           ops.softmax_xent
DenseHead      loss mse | bce                              ops.linear_fwd to fp32
                                                           pre-activations + ops.dense_loss
=============  ==========================================  =====================================

A Stage reads two integers off its head -- ``fwd_from`` and ``dgrad_from`` -- and needs to know
nothing else about which head it has.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch

from .. import ops, switches


def check_loss(loss: str, last_activation: str) -> None:
    """Raise unless ``loss`` is a known loss defined for the network's last activation."""
    if loss != "softmax_ce":
        ops.check_dense_loss(loss, last_activation)


class Slot:
    """A per-step input a head reads (labels, dense targets): an owned buffer that batches are
    copied into, or -- zero-copy -- a caller's tensor read in place. Under the native executor
    the slot is a relocatable Program region, so re-pointing it needs no re-recording."""

    def __init__(self, buf: torch.Tensor, in_place_ok: Callable[[torch.Tensor], bool]):
        self.buf = buf  # owned
        self.cur = buf  # what the kernels read: ``buf`` or an alias of a dataset slice
        self._in_place_ok = in_place_ok
        self._prog = self.region = None

    def attach(self, prog) -> None:
        """Make the slot a region of ``prog`` (about to be recorded, reading the owned buffer)."""
        self.cur = self.buf
        self.region = prog.region(self.buf.data_ptr(), self.buf.numel() * self.buf.element_size())
        self._prog = prog

    def bind(self, t: torch.Tensor) -> None:
        """Read ``t`` (laid out like the owned buffer) in place from now on."""
        self.cur = t
        if self._prog is not None:
            self._prog.rebase(self.region, t.data_ptr())

    def reset(self) -> None:
        self.bind(self.buf)  # never write through an alias of the caller's dataset

    def load(self, src: torch.Tensor, zero_copy: bool = False) -> None:
        """This step reads ``src``: in place when ``zero_copy`` and it is laid out like the
        owned buffer, else copied into it (a narrower matrix fills the leading columns)."""
        b = self.buf
        if zero_copy and src.shape == b.shape and src.dtype == b.dtype and \
                src.device == b.device and self._in_place_ok(src):
            self.bind(src)
        else:
            self.reset()
            (b if src.dim() == 1 else b[:, :src.shape[1]]).copy_(src)

    def pin(self) -> None:
        """Before a graph capture: a graph needs the fixed owned buffer (later batches are
        copied into it), so what is bound in place moves there."""
        if self.cur.data_ptr() != self.buf.data_ptr():
            self.buf.copy_(self.cur)
            self.reset()


class LossHead:
    """What every head exposes to its Stage, all fixed at construction:

    ``fwd_from``    first local layer whose forward the head runs (layers below are the
                    stage's own forward GEMMs);
    ``dgrad_from``  dgrads of local layers at or above this index run inside the head, so dZ of
                    layers >= dgrad_from - 1 comes from the head, with ``blocks`` bias-gradient
                    partials per micro-batch;
    ``blocks``      row-block partials per micro-batch; ``chunks``: loss partials per row block;
    ``logits``      the last layer's output is materialised (fp32 [rows][Np]), else it is the
                    empty [0][Np] tensor;
    ``labels`` / ``targets`` (dense only) slots, ``loss_part`` and ``correct`` buffers.
    """

    tail = fused_xent = dense = False
    logits = True

    @staticmethod
    def choose(st) -> Optional["LossHead"]:
        """The head of Stage ``st`` (None unless it is the last stage); ``st.loss`` has passed
        check_loss."""
        if not st.last:
            return None
        if st.loss != "softmax_ce":
            return DenseHead(st)
        # the last layer's softmax-CE is fused into its GEMM epilogue when the padded class
        # count is one 64/128-wide tile
        if not (st.geoms[-1].np_ in (64, 128) and switches.get("DNN_FUSED_XENT") == "1"):
            return XentHead(st)
        return TailHead(st) if TailHead.supported(st) else FusedXentHead(st)

    def __init__(self, st, blocks: int, chunks: int = 1):
        L, dev = len(st.geoms), st.device
        self.fwd_from, self.dgrad_from = (L - 2, L - 2) if self.tail else (L - 1, L)
        self.blocks, self.chunks = blocks, chunks
        self.labels = Slot(torch.full((st.rows,), -1, dtype=torch.int32, device=dev),
                           lambda y: y.is_contiguous())
        self.targets: Optional[Slot] = None
        self.loss_part = torch.zeros(blocks * chunks * st.nm, dtype=torch.float32, device=dev)
        # per-block correct counts, written (not accumulated) by the loss kernels
        self.correct = torch.zeros(blocks * st.nm, dtype=torch.int32, device=dev)

    def slots(self) -> list[Slot]:
        return [s for s in (self.labels, self.targets) if s is not None]

    def _parts(self, j: int) -> tuple[torch.Tensor, torch.Tensor]:
        """Micro-batch j's slices of loss_part and correct."""
        n = self.blocks * self.chunks
        return self.loss_part[j * n:(j + 1) * n], self.correct[j * self.blocks:(j + 1) * self.blocks]

    def forward(self, st, j: int) -> None:
        raise NotImplementedError

    def set_batch(self, labels: Optional[torch.Tensor], targets: Optional[torch.Tensor],
                  zero_copy: bool = False) -> None:
        if targets is not None:
            raise ValueError("dense targets need Trainer(loss='mse' | 'bce')")
        if labels is None:
            raise ValueError("last stage needs labels")
        self.labels.load(labels, zero_copy)

    def pin(self) -> None:
        for s in self.slots():
            s.pin()

    def loss_sum(self) -> float:
        """Sum of per-row losses of the last step (fixed-order fp64 host sum)."""
        return float(self.loss_part.detach().cpu().double().sum())

    def correct_sum(self) -> Optional[int]:
        """Correct predictions of the last step (None under a dense loss: no classes)."""
        return int(self.correct.sum().item())


class XentHead(LossHead):
    """fp32 logits + the stand-alone softmax cross-entropy kernel (any class count)."""

    def __init__(self, st):
        super().__init__(st, ops.xent_blocks(st.mb))

    def forward(self, st, j: int) -> None:
        i, r, p = len(st.geoms) - 1, st.rows_of(j), st.params
        y = st.acts[i][r]
        lp, cr = self._parts(j)
        ops.linear_fwd(st.input_of(i)[r], p.wbf(i), p.b32(i), y, act="linear")  # fp32 logits
        ops.softmax_xent(y, self.labels.cur[r], st.dz[i][r], st.n_cls, 1.0 / st.global_batch,
                         lp, cr, colsum=st._bpart(i, j))


class FusedXentHead(LossHead):
    """Softmax cross-entropy in the last layer's GEMM epilogue."""

    fused_xent = True
    logits = False

    def __init__(self, st):
        super().__init__(st, st.mb // ops.xent_tiles(st.mb, st.geoms[-1].np_)[0])

    def forward(self, st, j: int) -> None:
        i, r, p = len(st.geoms) - 1, st.rows_of(j), st.params
        lp, cr = self._parts(j)
        ops.linear_fwd_xent(st.input_of(i)[r], p.wbf(i), p.b32(i), st.dz[i][r],
                            self.labels.cur[r], st.n_cls, 1.0 / st.global_batch, lp, cr,
                            colsum=st._bpart(i, j))


class TailHead(LossHead):
    """Narrow classifier tail (csrc/kernels/mlp_tail.hip): the forward of the last two layers,
    the softmax CE and both of their dgrads run as ONE kernel inside the last layer's forward;
    the second-to-last layer's forward and both dgrads are then no-ops of the stage."""

    tail = fused_xent = True  # chosen only where the GEMM-fused CE would be
    logits = False

    @staticmethod
    def supported(st) -> bool:
        """Given that the GEMM-fused CE applies."""
        if not (st.device.type == "cuda" and len(st.geoms) >= 3 and
                switches.get("DNN_TAIL") == "1"):
            return False
        g2, g3, g4 = st.geoms[-3], st.geoms[-2], st.geoms[-1]
        acts = ("relu", "sigmoid", "linear")
        return (ops.tail_supported(g3.kp, g3.np_, g4.np_, st.n_cls) and
                g3.spec.activation in acts and g2.spec.activation in acts and
                st.mb % 16 == 0)

    def __init__(self, st):
        super().__init__(st, ops.tail_blocks(st.mb))

    def forward(self, st, j: int) -> None:
        L, r, p = len(st.geoms), st.rows_of(j), st.params
        lp, cr = self._parts(j)
        ops.mlp_tail(st.acts[L - 3][r], p.wbf(L - 2), p.b32(L - 2), p.wbf(L - 1),
                     p.b32(L - 1), self.labels.cur[r], st.acts[L - 2][r], st.dz[L - 1][r],
                     st.dz[L - 2][r], st.dz[L - 3][r], st.n_cls, 1.0 / st.global_batch,
                     act3=st.geoms[L - 2].spec.activation,
                     act2=st.geoms[L - 3].spec.activation, loss_part=lp, correct=cr,
                     cs4=st._bpart(L - 1, j), cs3=st._bpart(L - 2, j),
                     cs2=st._bpart(L - 3, j))


class DenseHead(LossHead):
    """fp32 pre-activations + the dense-target loss kernel (mse | bce) against bf16 targets
    [rows][Np]; ``labels`` is then only the row-validity vector (-1 = padding row)."""

    dense = True

    def __init__(self, st):
        gl = st.geoms[-1]
        super().__init__(st, ops.xent_blocks(st.mb), ops.dense_loss_col_chunks(gl.np_))
        self.loss = st.loss
        buf = torch.zeros(st.rows, gl.np_, dtype=torch.bfloat16, device=st.device)
        self.targets = Slot(buf, lambda t: t.stride() == buf.stride() and
                            t.data_ptr() % 16 == 0)

    def forward(self, st, j: int) -> None:
        i, r, p = len(st.geoms) - 1, st.rows_of(j), st.params
        y = st.acts[i][r]
        ops.linear_fwd(st.input_of(i)[r], p.wbf(i), p.b32(i), y, act="linear")  # fp32 pre-act.
        ops.dense_loss(y, self.targets.cur[r], st.dz[i][r], st.n_cls, 1.0 / st.global_batch,
                       self.loss, st.geoms[i].spec.activation, row_ok=self.labels.cur[r],
                       loss_part=self._parts(j)[0], colsum=st._bpart(i, j))

    def set_batch(self, labels, targets, zero_copy: bool = False) -> None:
        if targets is None:
            raise ValueError(f"last stage needs dense targets (loss={self.loss!r})")
        self.targets.load(targets, zero_copy)
        if labels is None:
            self.labels.reset()
            self.labels.buf.zero_()  # every row valid
        else:
            self.labels.load(labels, zero_copy)

    def correct_sum(self) -> None:
        return None
