"""One pipeline stage: a contiguous slice of Linear layers resident on one device.

This is the MI355X replacement of the reference's stage worker
(/root/reference/src/grpc_node.py:16-97), which held its layers' fp64 weights and ran
``np.dot(x, W) + b`` + activation per request. A Stage instead owns, for one training step of
``num_micro`` micro-batches of ``micro_batch`` rows:

* parameters in ONE flat fp32 master buffer (padded [Np][Kp] weight + [Np] bias per layer),
  a bf16 shadow of it that the GEMMs read, one flat fp32 gradient buffer (the unit of the DP
  all-reduce) and flat optimizer state -- so the optimizer is a single fused kernel;
* step buffers for every micro-batch (activations, dZ, logits, labels) laid out as
  [num_micro * micro_batch] rows, so micro-batch j is a row slice and the deferred weight
  gradient can run as ONE batch-contraction GEMM over all rows (or per micro-batch);
* split-K wgrad slabs and bias-gradient partials, reduced deterministically (no atomics).

Per layer the compute is three fused gfx950 kernels: forward GEMM with bias+activation
epilogue, dgrad GEMM whose epilogue applies the previous layer's activation derivative (read
from the stored activation -- no mask tensor), and the wgrad GEMM. How the last stage ends --
which kernels run its last layer(s) and the loss, and which dgrads they absorb -- is its loss
head's business (engine/loss_head.py); a Stage only asks the head which layers it covers.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from .. import ops
from ..models.mlp import LayerGeom, MLPSpec
from ..utils.native import native
from .. import switches
from .loss_head import LossHead, check_loss
from .optimizer import OptimConfig  # (tests and bench scripts import both from this module)
from .params import StageParams

RELU_MASK_AUTO_WIDTH = 1024  # DNN_RELU_MASK=auto: masks for hidden layers at least this wide


def _of_head(path: str, default=None) -> property:
    """Read-only ``stage.head.<path>``; ``default`` where the stage has no head (it is not the
    last) or the head has no such part (targets of a class-label loss)."""
    def get(self):
        obj = self.head
        for name in path.split("."):
            if obj is None:
                return default
            obj = getattr(obj, name)
        return obj
    return property(get)


class Stage:
    """Compute of one pipeline stage for one step (see module doc)."""

    def __init__(self, spec: MLPSpec, layer_start: int, layer_end: int, *, micro_batch: int,
                 num_micro: int, device: torch.device, global_batch: Optional[int] = None,
                 optim: Optional[OptimConfig] = None, wgrad: str = "batched",
                 stage_index: int = 0, num_stages: int = 1, wgrad_algo: Optional[str] = None,
                 dp_shard: Optional[tuple[int, int]] = None, loss: str = "softmax_ce"):
        if not 0 <= layer_start < layer_end <= len(spec.layers):
            raise ValueError("bad layer range")
        # loss of the last stage: softmax cross-entropy against int32 class labels (default),
        # or a dense-target loss (mse | bce) against a bf16 target matrix
        check_loss(loss, spec.layers[-1].activation)
        self.loss = loss
        if micro_batch <= 0 or micro_batch % 64:
            raise ValueError("micro_batch must be a positive multiple of 64 (MFMA row tiles); "
                             "pad the batch with label -1 rows")
        self.spec = spec
        self.l0, self.l1 = layer_start, layer_end
        self.first = layer_start == 0
        self.last = layer_end == len(spec.layers)
        self.stage_index, self.num_stages = stage_index, num_stages
        self.mb, self.nm = micro_batch, num_micro
        self.rows = micro_batch * num_micro
        self.device = device
        self.global_batch = global_batch or self.rows
        self.wgrad_mode = wgrad
        self.wgrad_algo = wgrad_algo or switches.get("DNN_WGRAD_ALGO")
        if self.wgrad_algo not in ("streamk", "splitk"):
            raise ValueError(f"wgrad_algo must be streamk | splitk, got {self.wgrad_algo!r}")
        self.geoms = [LayerGeom(i, spec.layers[i]) for i in range(layer_start, layer_end)]
        self.params = StageParams(self.geoms, device, optim, shard=dp_shard)
        self.prev_act = spec.layers[layer_start - 1].activation if not self.first else "linear"
        self.n_cls = spec.out_dim
        self._alloc()

    # -------------------------------------------------------------------------------------
    def _alloc(self):
        R, dev = self.rows, self.device
        bf, f32 = torch.bfloat16, torch.float32
        g0 = self.geoms[0]
        self.x_buf = torch.zeros(R, g0.kp, dtype=bf, device=dev)
        self.x_in = self.x_buf  # may be re-pointed at a resident dataset slice (zero-copy)
        # The loss head (last stage only) runs the forward of local layers >= fwd_from and the
        # dgrads of local layers >= dgrad_from inside its own kernels; everything below those
        # two indices is a GEMM of this stage (both are L without a head)
        L = len(self.geoms)
        self.head = head = LossHead.choose(self)
        self.fwd_from = head.fwd_from if head else L
        self.dgrad_from = head.dgrad_from if head else L
        self.acts: list[torch.Tensor] = []  # output of local layer i
        for i, g in enumerate(self.geoms):
            if head and i == L - 1:  # fp32, or never in memory at all
                self.acts.append(torch.zeros(R if head.logits else 0, g.np_, dtype=f32,
                                             device=dev))
            else:
                self.acts.append(torch.zeros(R, g.np_, dtype=bf, device=dev))
        # 1-bit ReLU masks of the hidden outputs consumed by this stage's own dgrads (GPU,
        # DNN_RELU_MASK=1; off by default: measured 0.380 vs 0.371 ms on the headline step,
        # the byte-granular mask stores/loads cost more than the activation bytes saved):
        # the dgrad epilogue then reads N/8 bytes per row instead of the bf16 activation (the
        # activation itself is still kept: it is the next layer's wgrad operand)
        # DNN_RELU_MASK=2: fragment-order masks (ops.FragMask: one 16-byte access per lane), only
        # where a GEMM dgrad of this stage consumes them and it runs the forward's tile shape
        mask_mode = switches.get("DNN_RELU_MASK") if dev.type == "cuda" else "0"
        self.relu_mask = []
        for i, g in enumerate(self.geoms):
            m = None
            # auto: fragment-order masks for layers >= 1024 wide, where the dgrad's activation
            # read is the big term (wide 5.81 -> 5.44 ms, mlp8 2.73 -> 2.71; the headline's
            # 512-wide layer 0 loses: profiles/r5_tables/relu_mask_*)
            mode_i = ("2" if g.np_ >= RELU_MASK_AUTO_WIDTH else "0") if mask_mode == "auto" \
                else mask_mode
            if mode_i == "1" and i < L - 1 and g.spec.activation == "relu":
                m = torch.zeros(R, g.np_ // 8, dtype=torch.uint8, device=dev)
            elif mode_i == "2" and i + 1 < self.dgrad_from and g.spec.activation == "relu":
                tiles = ops.frag_mask_tiles(self.mb, g.np_, g.kp, self.geoms[i + 1].np_)
                if tiles is not None:
                    m = ops.FragMask.alloc(R, g.np_, tiles, dev)
            self.relu_mask.append(m)
        self.dz = [torch.zeros(R, g.np_, dtype=bf, device=dev) for g in self.geoms]
        self.dx_send = None if self.first else torch.zeros(R, g0.kp, dtype=bf, device=dev)
        # K-major weight gradients (ops.linear_wgrad dzt / xt): for big hidden layers whose dZ
        # and input activation come from this stage's own one-tile GEMMs, those GEMMs also write
        # the transposed copies in their epilogues (+1 write of each, -20 % wgrad time)
        self.dzT: dict[int, torch.Tensor] = {}
        self.actT: dict[int, torch.Tensor] = {}
        kk = switches.get("DNN_WGRAD_KK")
        if dev.type == "cuda" and self.wgrad_mode == "batched" and kk != "0":
            for i in range(1, L):
                g = self.geoms[i]
                big = kk == "1" or g.np_ * g.kp >= (1 << 24)
                dz_by_dgrad = i + 1 < self.dgrad_from and self.relu_mask[i] is None
                x_by_fwd = i - 1 < self.fwd_from and self.relu_mask[i - 1] is None
                if big and dz_by_dgrad and x_by_fwd:
                    self.dzT[i] = torch.zeros(g.np_, R, dtype=bf, device=dev)
                    self.actT[i - 1] = torch.zeros(g.kp, R, dtype=bf, device=dev)
        # dgrad GEMMs read W^T (contraction-contiguous B operand, see ops.linear_dgrad)
        if dev.type == "cuda" and switches.get("DNN_DGRAD_WT") == "1":
            for i in range(self.dgrad_from):
                if i > 0 or not self.first:
                    self.params.enable_wt(i)
        # wgrad geometry: batched = one GEMM over all rows; per_micro = one per micro-batch
        wrows = R if self.wgrad_mode == "batched" else self.mb
        if self.wgrad_algo == "streamk":  # balanced stream-K, reduced straight into the grads
            self.w_splits = [1] * len(self.geoms)
            self.slabs = []
            n = max(ops.streamk_partial_elems(g.np_, g.kp) for g in self.geoms)
            self.sk_part = torch.zeros(n, dtype=f32, device=dev)
        else:  # classic split-K slabs + reduce
            self.w_splits = [ops.pick_splits(g.np_, g.kp, wrows) for g in self.geoms]
            self.slabs = [torch.zeros(s, g.np_, g.kp, dtype=f32, device=dev)
                          for s, g in zip(self.w_splits, self.geoms)]
        # Bias-gradient partials (column sums of dZ) come fused from whichever kernel produces
        # dZ: the dgrad epilogue of the next local layer (one partial per output row tile), the
        # loss head (one per row block of its kernel), or -- for a gradient received from the
        # next stage -- a colsum kernel. self.bp[i] = partials per micro-batch.
        self.bp = []
        for i in range(L):
            if head and i >= self.dgrad_from - 1:
                self.bp.append(head.blocks)
            elif i < L - 1:
                g1 = self.geoms[i + 1]
                self.bp.append(self.mb // ops.dgrad_tiles(self.mb, g1.kp, g1.np_)[0])
            else:
                # one partial per 128 rows: enough workgroups to fill the chip (1024-row
                # partitions left a 4096-row boundary colsum at 32 workgroups, 12 us)
                self.bp.append(max(1, self.mb // 128))
        self.bpart = [torch.zeros(self.bp[i] * self.nm, g.np_, dtype=f32, device=dev)
                      for i, g in enumerate(self.geoms)]
        self._w_done = 0
        self._reduce_jobs: dict = {}
        self._colsum_by = None  # loopback: the next stage computes our boundary colsum
        self._colsum_for = None  # ... and this is the stage we compute it for
        self._prog = None  # native Program once compile_native() ran
        self._recording = False
        self._has_w = False
        self._o_native = False  # "O" recorded (device-side lr / step)
        self._rx = None
        self.boundary = "bf16"
        self._fp8_next = self._fp8_prev = False

    # the head's choice and buffers, readable where the stage's own used to be
    tail = _of_head("tail", False)
    fused_xent = _of_head("fused_xent", False)
    dense = _of_head("dense", False)
    loss_part = _of_head("loss_part")
    correct = _of_head("correct")
    labels = _of_head("labels.cur")
    labels_buf = _of_head("labels.buf")
    targets = _of_head("targets.cur")
    targets_buf = _of_head("targets.buf")

    # ---- fp8 pipeline boundary (opt-in: Trainer(boundary="fp8")) -------------------------
    def enable_fp8_boundary(self, has_prev: bool, has_next: bool) -> None:
        """Hops to/from neighbouring stages carry OCP e4m3 rows + one fp32 scale per row
        (ops.quant_rows_fp8): half the bytes of bf16 on the xGMI link, for activations forward
        and gradients backward. Buffers are step-sized like the bf16 ones."""
        R, dev, u8 = self.rows, self.device, torch.uint8
        self.boundary = "fp8"
        if has_next:
            w = self.output.shape[1]
            self.q_out, self.s_out = torch.zeros(R, w, dtype=u8, device=dev), \
                torch.zeros(R, device=dev)
            self.q_gin, self.s_gin = torch.zeros(R, w, dtype=u8, device=dev), \
                torch.zeros(R, device=dev)
        if has_prev:
            w = self.x_buf.shape[1]
            self.q_in, self.s_in = torch.zeros(R, w, dtype=u8, device=dev), \
                torch.zeros(R, device=dev)
            self.q_dx, self.s_dx = torch.zeros(R, w, dtype=u8, device=dev), \
                torch.zeros(R, device=dev)
        self._fp8_next, self._fp8_prev = has_next, has_prev

    def pack_fwd(self, j: int) -> None:
        if self._prog is not None and not self._recording:
            return self._replay(f"QF{j}")
        r = self.rows_of(j)
        ops.quant_rows_fp8(self.output[r], self.q_out[r], self.s_out[r])

    def unpack_fwd(self, j: int) -> None:
        if self._prog is not None and not self._recording:
            return self._replay(f"DQF{j}")
        r = self.rows_of(j)
        ops.dequant_rows_fp8(self.q_in[r], self.s_in[r], self.x_in[r])

    def pack_bwd(self, j: int) -> None:
        if self._prog is not None and not self._recording:
            return self._replay(f"QB{j}")
        r = self.rows_of(j)
        ops.quant_rows_fp8(self.dx_send[r], self.q_dx[r], self.s_dx[r])

    def unpack_bwd(self, j: int) -> None:
        if self._prog is not None and not self._recording:
            return self._replay(f"DQB{j}")
        r = self.rows_of(j)
        ops.dequant_rows_fp8(self.q_gin[r], self.s_gin[r], self.grad_out[r])

    def rows_of(self, j: int) -> slice:
        if not 0 <= j < self.nm:
            raise IndexError(f"micro-batch {j} out of range [0, {self.nm})")
        return slice(j * self.mb, (j + 1) * self.mb)

    def input_of(self, i: int) -> torch.Tensor:
        return self.x_in if i == 0 else self.acts[i - 1]

    @property
    def output(self) -> torch.Tensor:
        """Activation sent to the next stage (bf16 [rows][Np])."""
        return self.acts[-1]

    @property
    def grad_out(self) -> torch.Tensor:
        """dZ of this stage's last layer, written by the next stage (received gradient)."""
        return self.dz[-1]

    # -------------------------------------------------------------------------------------
    def begin_step(self) -> None:
        self._w_done = 0

    def forward(self, j: int) -> None:
        if self._prog is not None and not self._recording:
            return self._replay(f"F{j}")
        for i in range(len(self.geoms)):
            self._forward_layer(j, i)

    def forward_layers(self, j: int, i0: int, i1: int) -> None:
        """Forward of micro-batch j through local layers [i0, i1) only (a DP step whose
        update of later layers is deferred runs the earlier layers first)."""
        if self._prog is not None and not self._recording:
            self._prog.run([f"F{j}.L{i}" for i in range(i0, i1)],
                           torch.cuda.current_stream(self.device).cuda_stream)
            return
        for i in range(i0, i1):
            self._forward_layer(j, i)

    def _forward_layer(self, j: int, i: int) -> None:
        if i >= self.fwd_from:
            # the head's layers: all of its work is launched at (and recorded under) the last
            if i == len(self.geoms) - 1:
                self.head.forward(self, j)
            return
        r = self.rows_of(j)
        p = self.params
        m = self.relu_mask[i]
        ops.linear_fwd(self.input_of(i)[r], p.wbf(i), p.b32(i), self.acts[i][r],
                       act=self.geoms[i].spec.activation, mask=None if m is None else m[r],
                       yt=self.actT[i][:, r] if i in self.actT else None)

    def backward(self, j: int) -> None:
        """dgrad chain of micro-batch j; dZ of the last local layer must already be present."""
        if self._prog is not None and not self._recording:
            return self._replay(f"B{j}")
        self._backward_pre(j)
        for i in range(len(self.geoms) - 1, -1, -1):
            self._backward_layer(j, i)

    def _backward_pre(self, j: int) -> None:
        if not self.last and self._colsum_by is None:  # dZ of our last layer arrived from
            L = len(self.geoms) - 1                       # the next stage
            ops.colsum_partial(self.dz[L][self.rows_of(j)], self._bpart(L, j), self.bp[L])

    def _backward_layer(self, j: int, i: int) -> None:
        """dgrad of local layer i for micro-batch j: dZ of layer i -> dZ of layer i-1 (or the
        gradient sent to the previous stage when i == 0)."""
        if i >= self.dgrad_from:
            return  # ran inside the loss head's kernel (forward of micro-batch j)
        r = self.rows_of(j)
        p = self.params
        if i > 0:
            prev = self.geoms[i - 1].spec.activation
            m = self.relu_mask[i - 1]
            ops.linear_dgrad(self.dz[i][r], p.wbf(i), self.dz[i - 1][r],
                             y_prev=self.acts[i - 1][r], act_prev=prev,
                             colsum=self._bpart(i - 1, j),
                             mask_prev=None if m is None else m[r], wt=p.wt.get(i),
                             dxt=self.dzT[i - 1][:, r] if (i - 1) in self.dzT else None)
        elif not self.first:
            # gradient for the previous stage, already multiplied by the derivative of its
            # last layer's activation (its output is our input x_in)
            up = self._colsum_for
            ops.linear_dgrad(self.dz[0][r], p.wbf(0), self.dx_send[r], y_prev=self.x_in[r],
                             act_prev=self.prev_act,
                             colsum=None if up is None else up._bpart(len(up.geoms) - 1, j),
                             wt=p.wt.get(0))

    def wgrad(self, j: int = -1) -> None:
        """Weight/bias gradients for micro-batch j (slab-accumulated) or all rows (j = -1)."""
        if j < 0 and self._prog is not None and not self._recording and self._has_w:
            self._replay("W")
            self._w_done += 1
            return
        self._wgrad_all(j)
        self._w_done += 1

    def _wgrad_all(self, j: int = -1) -> None:
        """Every local layer's weight gradient: one grouped launch per shared tile configuration
        (ops.linear_wgrad_group; DNN_WGRAD_GROUP=0 disables), one launch per remaining layer."""
        if (self.wgrad_algo == "splitk" and self.device.type == "cuda" and
                switches.get("DNN_WGRAD_GROUP") == "1" and len(self.geoms) > 1):
            if j < 0:
                r, acc = slice(0, self.rows), False
            else:
                r, acc = self.rows_of(j), self._w_done > 0
            if j < 0 or self.wgrad_mode != "batched":
                fused = self.params.fused_layers
                idx = [i for i in range(len(self.geoms)) if i not in fused]
                items = [(self.dz[i][r], self.input_of(i)[r], self.slabs[i], self.w_splits[i],
                          acc) for i in idx]
                for k in ops.linear_wgrad_group(items):
                    self.wgrad_layer(idx[k], j)
                for i in sorted(fused):
                    self.wgrad_layer(i, j)
                return
        for i in range(len(self.geoms)):
            self.wgrad_layer(i, j)

    def _bpart(self, i: int, j: int) -> torch.Tensor:
        return self.bpart[i][j * self.bp[i]:(j + 1) * self.bp[i]]

    def wgrad_layer(self, i: int, j: int = -1) -> None:
        """Weight gradient GEMM of local layer i (bias partials were produced with dZ)."""
        if j < 0 and self._prog is not None and not self._recording and self._has_w:
            return self._replay(f"W{i}")
        if j < 0:
            r, accumulate = slice(0, self.rows), False
        else:
            if self.wgrad_mode == "batched":
                raise RuntimeError("per-micro wgrad on a stage built with wgrad='batched'")
            r, accumulate = self.rows_of(j), self._w_done > 0
        if self.wgrad_algo == "streamk":
            g = self.geoms[i]
            ops.linear_wgrad_streamk(self.dz[i][r], self.input_of(i)[r],
                                     self.params.gw(i).view(g.np_, g.kp), self.sk_part,
                                     accumulate=accumulate)
        else:
            kk = j < 0 and i in self.dzT
            upd = wt = None
            p = self.params
            if i in p.fused_layers:  # the epilogue applies SGD to W_i and writes W_i^T
                if j >= 0:
                    raise RuntimeError("fused weight update runs on the batched wgrad only")
                upd, wt = p.epilogue_args(i), p.wt.get(i)
            ops.linear_wgrad(self.dz[i][r], self.input_of(i)[r], self.slabs[i],
                             splits=self.w_splits[i], accumulate=accumulate,
                             dzt=self.dzT[i] if kk else None,
                             xt=self.actT[i - 1] if kk else None, upd=upd, wt=wt)

    def finalize_grads(self, layers: Optional[Sequence[int]] = None) -> None:
        """Reduce bias partials (and, for split-K, weight slabs) into the flat gradient."""
        if self._prog is not None and not self._recording:
            if layers is None:
                return self._replay("FIN")
            ls = list(layers)
            if len(ls) == 1:
                return self._replay(f"FIN{ls[0]}")
            if ls == list(range(ls[0], ls[-1] + 1)):
                return self._replay(f"FIN{ls[0]}-{ls[-1]}")
        key = tuple(range(len(self.geoms))) if layers is None else tuple(layers)
        ops.reduce_multi(self._jobs(key))  # one launch for every slab set and bias-partial set

    # W^T written by the fused update for layers up to this many weights: its transposed
    # stores are 2-byte scatters, cheaper than a transpose launch for the headline's 256x512
    # (step 0.3724 -> 0.3678 ms) but not measurably for mlp8's 1024x1024 layers (3.318 vs
    # 3.329 ms), which keep the coalesced LDS transpose (profiles/r2_sched/fin_wt_*)
    WT_BY_UPDATE_MAX = 1 << 19

    def _wt_by_update_layers(self) -> list:
        p = self.params
        if self.wgrad_algo == "streamk":
            return []
        return [i for i in p.wt if i not in p.fused_layers and
                self.geoms[i].np_ * self.geoms[i].kp <= self.WT_BY_UPDATE_MAX]

    def _jobs(self, key: tuple, with_wt: bool = False) -> list:
        """reduce_multi job table of the layers in ``key`` (buffers are fixed for the stage's
        lifetime: built once). ``with_wt`` (fused update only): the weight jobs of layers that
        keep a W^T shadow also write it (no transpose launch after the update)."""
        jobs = self._reduce_jobs.get((key, with_wt))
        if jobs is None:
            p = self.params
            jobs = []
            for i in key:
                g = self.geoms[i]
                n = g.np_ * g.kp
                if self.wgrad_algo != "streamk" and i not in p.fused_layers:
                    jobs.append((self.slabs[i], self.w_splits[i], n, n, p.gw(i), 1.0, False,
                                 p.wt[i] if with_wt and i in self._wt_by_update_layers()
                                 else None))
                jobs.append((self.bpart[i], self.bpart[i].shape[0], g.np_, g.np_, p.gb(i), 1.0,
                             False))
            self._reduce_jobs[(key, with_wt)] = jobs
        return jobs

    def fused_fin_sgd_ok(self) -> bool:
        """FIN + optimizer step as one launch: every gradient element must come out of a reduce
        job (not stream-K wgrad, which writes weight gradients directly); SGD, Adam or AdamW."""
        return (self.wgrad_algo != "streamk" and self.device.type == "cuda" and
                switches.get("DNN_FUSE_FIN_SGD") == "1")

    def _record_fin_sgd(self, a: int = 0, b: Optional[int] = None) -> None:
        """Record the gradient reduction of local layers [a, b) (default: all) with the
        optimizer update fused in (segment FINO, or FINO{a}-{b-1} for a layer range: SGD only,
        so the step counter needs no advance; lr from device memory like every update)."""
        p = self.params
        L = len(self.geoms)
        b = L if b is None else b
        if not p.opt.is_sgd and (a, b) != (0, L):
            raise ValueError("layer-range fused updates are SGD only")
        wt_fused = switches.get("DNN_FIN_WT") == "1" and p.shadow is not None
        jobs = self._jobs(tuple(range(a, b)), with_wt=wt_fused)
        # layers whose W^T comes out of the update launch itself (no transpose launch after it)
        skip = frozenset(i for i in self._wt_by_update_layers()) if wt_fused else frozenset()
        ops.reduce_multi(jobs, sgd=p.opt.fused_args())
        p.opt.record_advance()  # Adam (whole step only): the segment replaces FIN + O
        p.refresh_t(a, b, step=True, skip=skip)

    def update_then_forward(self, j: int, s: int, lr: Optional[float] = None) -> None:
        """Deferred DP update of layers [s, L) (completing the step: advance) followed by the
        forward of micro-batch j through [s, L) -- ONE native call when recorded."""
        L = len(self.geoms)
        if self._prog is not None and self._o_native and not self._recording:
            self.params.opt.arm(lr)
            self._prog.run([f"O{s}-{L}", "OADV"] + [f"F{j}.L{i}" for i in range(s, L)],
                           torch.cuda.current_stream(self.device).cuda_stream)
            self.params.opt.commit()
            return
        self.update_layers(s, L, lr, advance=True)
        self.forward_layers(j, s, L)

    def wgrad_finalize(self, layers: Sequence[int]) -> None:
        """Batched wgrad of ``layers`` (in the given order) + their gradient reduction: one
        native call when recorded (a DP bucket)."""
        ls = list(layers)
        lo, hi = min(ls), max(ls)
        if (self._prog is not None and not self._recording and self._has_w and
                sorted(ls) == list(range(lo, hi + 1))):
            fin = f"FIN{lo}" if lo == hi else f"FIN{lo}-{hi}"
            self._prog.run([f"W{i}" for i in ls] + [fin],
                           torch.cuda.current_stream(self.device).cuda_stream)
            return
        for i in ls:
            self.wgrad_layer(i)
        self.finalize_grads(sorted(ls))

    def enable_fused_wgrad_update(self) -> list[int]:
        """Layers whose weight gradient is ONE split (big layers: the wide model's 8192x8192)
        apply the SGD step in their wgrad GEMM's epilogue (ops.linear_wgrad upd): no fp32
        gradient round trip through HBM, no separate update pass over those weights, and W^T
        written by the same epilogue instead of a transpose launch. Only without data
        parallelism (the gradient must be complete where it is produced) and for SGD; call
        before compile_native. Returns the layers."""
        p = self.params
        if (self.device.type != "cuda" or self.wgrad_mode != "batched" or
                self.wgrad_algo != "splitk" or not p.opt.is_sgd or p.sharded or
                switches.get("DNN_WGRAD_FUSED_UPDATE") == "0" or self._prog is not None):
            return []
        p.fused_layers = {i for i in range(len(self.geoms)) if self.w_splits[i] == 1}
        self._reduce_jobs.clear()
        return sorted(p.fused_layers)

    def shard_update(self, e0: int, e1: int, lr: Optional[float] = None) -> None:
        """Sharded DP: unpack this rank's reduced piece of bucket [e0, e1) and update it (no
        step advance, no W^T refresh: both follow once per step)."""
        p = self.params
        p.opt.arm(lr)
        p.shard_unpack(e0, e1)
        p.update_range(*p.shard_piece(e0, e1), advance=False, refresh=False)

    def bias_update(self, lr: Optional[float] = None) -> None:
        """Sharded DP: every rank updates all biases (their fp32 gradients are all-reduced)."""
        p = self.params
        p.opt.arm(lr)
        p.update_range(p.bias_lo, p.numel, advance=False, refresh=False)

    def update_layers(self, a: int, b: int, lr: Optional[float] = None,
                      advance: bool = True) -> None:
        """Optimizer update of local layers [a, b) only (``advance``: this completes the
        step's update -- Adam's step counter moves once per step)."""
        p = self.params
        p.opt.arm(lr)
        if self._prog is not None and self._o_native and not self._recording:
            segs = [f"O{a}-{b}"] + (["OADV"] if advance else [])
            self._prog.run(segs, torch.cuda.current_stream(self.device).cuda_stream)
        else:
            p.update_range(*p.layers_range(a, b), advance)
        if advance:
            p.opt.commit()

    def optimizer_step(self, lr: Optional[float] = None) -> None:
        self.params.opt.arm(lr)
        if self._prog is not None and self._o_native and not self._recording:
            self._replay("O")
        else:
            self.params.update()
        self.params.opt.commit()

    def fuse_boundary_colsum(self, consumer: "Stage") -> None:
        """Same-process pipeline: ``consumer`` (the next stage) writes our last layer's
        bias-gradient partials from its input-gradient dgrad epilogue (loopback only)."""
        if consumer.mb != self.mb or consumer.nm != self.nm:
            raise ValueError("loopback stages must share the micro-batch layout")
        L = len(self.geoms) - 1
        g0 = consumer.geoms[0]
        bm = ops.dgrad_tiles(consumer.mb, g0.kp, g0.np_)[0]
        self.bp[L] = self.mb // bm
        self.bpart[L] = torch.zeros(self.bp[L] * self.nm, self.geoms[L].np_,
                                    dtype=torch.float32, device=self.device)
        self._reduce_jobs.clear()
        self._colsum_by = consumer
        consumer._colsum_for = self

    # ---- native replay (csrc/runtime/program.{hpp,cpp}) ---------------------------------
    def compile_native(self) -> None:
        """Record every per-op kernel sequence of this stage ONCE into a native Program:
        F{j} / B{j} per micro-batch, W{i} / W (batched wgrad), FIN{i} / FIN (gradient
        reduction) and O (SGD update). Afterwards forward/backward/... replay their segment
        from C++ (one Python call per schedule op instead of one per kernel). The first
        stage's input and the last stage's labels (and dense targets) are relocatable regions,
        so zero-copy batches (bind_input / bind_labels / bind_targets) work without
        re-recording. The Python bodies stay
        the reference path (CPU, per-micro wgrad, Adam)."""
        nat = native()
        prog = nat.Program()
        self.x_in = self.x_buf
        self._rx = (prog.region(self.x_buf.data_ptr(), self.x_buf.numel() * 2)
                    if self.first else None)
        for slot in (self.head.slots() if self.head else ()):
            slot.attach(prog)
        # DNN_H0_DOUBLE: the layer-0 activation alternates between two buffers from step to
        # step (a relocatable region re-based by flip_h0), so the next step's layer-0 forward
        # never has to wait for this step's side-stream weight gradient that reads it
        # (pipeline._xstep_plan drops that wait)
        L = len(self.geoms)
        self.h0_double = (switches.get("DNN_H0_DOUBLE") == "1" and self.device.type == "cuda"
                          and self.first and self.last and self.nm == 1 and L >= 2 and
                          0 not in self.actT and 0 < self.fwd_from)
        self._rh0 = None
        if self.h0_double:
            a0 = self.acts[0]
            self._h0_alt = torch.zeros_like(a0)
            self._h0_ptrs = (a0.data_ptr(), self._h0_alt.data_ptr())
            self._h0_flip = 0
            self._rh0 = prog.region(a0.data_ptr(), a0.numel() * a0.element_size())
        self._recording = True
        nat.record_begin(prog)
        try:
            for j in range(self.nm):
                prog.mark(f"F{j}")
                self.forward(j)
            for j in range(self.nm):  # per-layer forward segments (deferred DP updates)
                for i in range(len(self.geoms)):
                    prog.mark(f"F{j}.L{i}")
                    self._forward_layer(j, i)
            for j in range(self.nm):
                prog.mark(f"B{j}")
                self.backward(j)
            for j in range(self.nm):  # per-layer dgrad segments (dgrad/wgrad overlap plans)
                prog.mark(f"B{j}.pre")
                self._backward_pre(j)
                for i in range(len(self.geoms) - 1, -1, -1):
                    prog.mark(f"B{j}.L{i}")
                    self._backward_layer(j, i)
            self._has_w = self.wgrad_mode == "batched"
            if self._has_w:
                for i in range(len(self.geoms)):
                    prog.mark(f"W{i}")
                    self.wgrad_layer(i)
                prog.mark("W")
                self._wgrad_all()
            L = len(self.geoms)
            for a in range(L):  # every contiguous layer range: one reduce launch per DP bucket
                for b in range(a, L):
                    prog.mark(f"FIN{a}" if a == b else f"FIN{a}-{b}")
                    self.finalize_grads(list(range(a, b + 1)))
            prog.mark("FIN")
            self.finalize_grads()
            if self.fused_fin_sgd_ok():
                prog.mark("FINO")
                self._record_fin_sgd()
                if self.params.opt.is_sgd and L > 1:
                    # per-layer-range forms: the overlap plan updates the small layers on the
                    # side stream while the big layer's wgrad still runs (DNN_SPLIT_FINO)
                    for a in range(L):
                        for b in range(a, L):
                            prog.mark(f"FINO{a}-{b}")
                            self._record_fin_sgd(a, b + 1)
            prog.mark("O")
            p = self.params
            p.update()
            for a in range(L if not (p.sharded or p.fused_layers) else 0):
                # split updates: every contiguous layer range, no step advance
                for b in range(a + 1, L + 1):
                    prog.mark(f"O{a}-{b}")
                    p.update_range(*p.layers_range(a, b), advance=False)
            prog.mark("OADV")
            p.opt.record_advance()
            if p.sharded:  # sharded DP: per bucket pack / unpack + piece update
                for a in range(L):
                    for b in range(a, L):
                        e0, _ = p.layer_grad_range(a)
                        _, e1 = p.layer_grad_range(b)
                        prog.mark(f"SP{a}-{b}")
                        p.shard_pack(e0, e1)
                        prog.mark(f"SU{a}-{b}")
                        self.shard_update(e0, e1)
                prog.mark("SB")
                self.bias_update()
                prog.mark("T")
                p.refresh_t()
            for j in range(self.nm):  # fp8 boundary packs / unpacks per micro-batch
                if self._fp8_next:
                    prog.mark(f"QF{j}")
                    self.pack_fwd(j)
                    prog.mark(f"DQB{j}")
                    self.unpack_bwd(j)
                if self._fp8_prev:
                    prog.mark(f"DQF{j}")
                    self.unpack_fwd(j)
                    prog.mark(f"QB{j}")
                    self.pack_bwd(j)
            self._o_native = True
        finally:
            nat.record_end()
            self._recording = False
        self._prog = prog

    def _replay(self, seg: str) -> None:
        self._prog.run([seg], torch.cuda.current_stream(self.device).cuda_stream)

    def flip_h0(self) -> None:
        """Start a step on the other layer-0 activation buffer (DNN_H0_DOUBLE)."""
        if self._rh0 is not None:
            self._h0_flip ^= 1
            self._prog.rebase(self._rh0, self._h0_ptrs[self._h0_flip])

    def bind_input(self, x: torch.Tensor) -> None:
        """First stage reads ``x`` in place (zero-copy) from now on."""
        self.x_in = x
        if self._prog is not None and self._rx is not None:
            self._prog.rebase(self._rx, x.data_ptr())

    def bind_labels(self, y: torch.Tensor) -> None:
        self.head.labels.bind(y)

    def bind_targets(self, t: torch.Tensor) -> None:
        """Dense loss: the last stage reads the bf16 targets ``t`` ([rows][Np], the row stride
        of ``targets_buf``) in place from now on."""
        self.head.targets.bind(t)

    def pin_input(self) -> None:
        """Before a graph capture: a graph needs the fixed input buffer (later batches are
        copied into it), so an input bound in place moves there."""
        if self.x_in.data_ptr() != self.x_buf.data_ptr():
            self.x_buf.copy_(self.x_in)
            self.bind_input(self.x_buf)

    # convenience: a whole step when this stage holds the entire model ----------------------
    def set_batch(self, x: torch.Tensor, labels: Optional[torch.Tensor],
                  targets: Optional[torch.Tensor] = None) -> None:
        self.bind_input(self.x_buf)  # never write through an alias of the caller's dataset
        self.x_in.copy_(x)
        if self.head is not None:
            self.head.set_batch(labels, targets)

    def loss_sum(self) -> float:
        """Sum of per-row losses of the last step (fixed-order fp64 host sum)."""
        return self.head.loss_sum()

    def flops_per_step(self) -> float:
        f = 0.0
        for i, g in enumerate(self.geoms):
            mult = 3 if (i > 0 or not self.first) else 2
            f += 2.0 * mult * self.rows * g.np_ * g.kp
        return f
