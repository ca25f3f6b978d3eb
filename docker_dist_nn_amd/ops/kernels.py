"""Tensor-level entry points of the compute kernels.

Every op takes pre-allocated output tensors (the engine owns all step buffers, so a captured HIP
graph replays with fixed pointers) and dispatches on the device of its inputs:

* CUDA/HIP tensors -> the hand-written gfx950 kernels of ``csrc/kernels`` through the native
  extension. There is deliberately NO PyTorch fallback on the GPU: if the extension is missing,
  :func:`docker_dist_nn_amd.utils.native.native` raises.
* CPU tensors -> :mod:`.reference`, a torch implementation with the same numerics contract
  (bf16 operands, fp32 accumulation, bf16/fp32 outputs). It exists so the engine/pipeline/DP
  logic is testable on CPU with the gloo backend, and it is the oracle of the GPU kernel tests.
"""
from __future__ import annotations

import torch

from ..models.mlp import ACT_CODE
from ..utils.native import native
from . import reference as ref
from .. import switches
from .gemm_plan import (DIRECT_STAGES, FRAG_WAVES, GEMV_MAX_ROWS, GROUP_STAGES, NUM_CU,
                        RP_STAGED, blas_built, pick_tiles, plan)  # noqa: F401 (blas_built: the
# comparison build's blas_gemm / dact_colsum live here, and callers ask this module for it)

KMAJ, MNMAJ = 0, 1


# A/B of the activation-specialised register-direct epilogue (GemmParams::epi_probe bit 2)
_EPI_GENERIC = 4 if switches.get("DNN_GEMM_EPI_GENERIC") == "1" else 0


_BLAS_OK: dict = {}


def _blas_ok(a, b, d, trans_a, trans_b, M, N, K, bias, relu, accumulate) -> bool:
    """Does hipBLASLt have an algorithm for this problem signature? (probed once per signature;
    a table entry that asks for the library falls back to the MFMA kernels when it has none)"""
    key = (int(trans_a), int(trans_b), M, N, K, a.stride(0), b.stride(0), d.stride(-2),
           int(d.dtype == torch.float32), int(bias is not None), int(relu), int(accumulate))
    if key not in _BLAS_OK:
        _BLAS_OK[key] = bool(native().blas_supported(*key))
    return _BLAS_OK[key]


def blas_gemm(a, b, d, *, trans_a: bool, trans_b: bool, M: int, N: int, K: int, bias=None,
              relu: bool = False, accumulate: bool = False, algo: int = 0):
    """hipBLASLt library GEMM (csrc/runtime/blaslt.hpp), row-major: d[M][N] (+)= op(a).op(b)
    (+ bias, ReLU), a = [M][K] or (trans_a) [K][M], b = [K][N] or (trans_b) [N][K]."""
    if not a.is_cuda:
        raise ValueError("blas_gemm is a GPU path")
    for t, name in ((a, "a"), (b, "b")):
        _rows(t, name, torch.bfloat16)
    if d.dtype not in (torch.bfloat16, torch.float32) or d.stride(-1) != 1:
        raise ValueError("d must be a row-major bf16 or fp32 matrix")
    native().blas_gemm(int(trans_a), int(trans_b), M, N, K, _p(a), a.stride(0), _p(b),
                       b.stride(0), _p(d), d.stride(-2), int(d.dtype == torch.float32),
                       _p(bias), int(relu), int(accumulate), _stream(a), int(algo))


def dact_colsum(x, aux, act, part=None, n_part: int = 1):
    """x = act'(aux) * x in place (bf16), and (optional) part[n_part][cols] = column sums of the
    result over n_part row blocks: the epilogue of a library-GEMM dgrad."""
    rows, cols = x.shape
    if not x.is_cuda:
        x.copy_(ref.act_bwd(x.float(), aux[:rows, :cols].float(), _act(act)).to(x.dtype))
        if part is not None:
            ref.colsum_partial(x, part, n_part)
        return
    native().dact_colsum(_p(x), x.stride(0), _p(aux), aux.stride(0), _act(act), rows, cols,
                         n_part, _p(part), _stream(x))


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _p(t: torch.Tensor | None) -> int:
    return 0 if t is None else t.data_ptr()


def _rows(t: torch.Tensor, name: str, dtype: torch.dtype) -> None:
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: expected a row-major 2-D tensor, got shape {tuple(t.shape)} "
                         f"strides {t.stride()}")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")


def _act(act) -> int:
    return ACT_CODE[act] if isinstance(act, str) else int(act)


def gemm(a, b, c, *, layout_a: int, layout_b: int, M: int, N: int, K: int, bias=None, aux=None,
         act=0, accumulate: bool = False, splits: int = 1, tiles: tuple[int, int] | None = None,
         colsum=None, k_total: int = 0, stages: int = 0, group_m: int = 0, persist: int = 0,
         mask_out=None, mask_in=None, ct=None, upd=None, timeline=None, epi_probe: int = 0):
    """C (+)= epilogue(A.B). See csrc/kernels/gemm.hpp for the layout/epilogue contract.
    ``epi_probe`` (diagnosis only, results WRONG): GemmParams::epi_probe.

    ``timeline`` (int64 GPU tensor, >= 4 per workgroup; one-tile kernels): per-workgroup phase
    timestamps for bench/probes/gemm_timeline.py (GemmParams::timeline).

    ``persist`` != 0 runs the persistent-workgroup form with the register-direct epilogue
    (csrc/kernels/gemm_persist.hip): -1 = one resident round, > 0 = workgroup count.
    ``mask_out`` / ``mask_in`` (uint8 [M][>= N/8], act = relu, GPU only): the forward writes the
    1-bit ReLU mask of its stored output; a dgrad reads it instead of ``aux``.

    ``k_total`` > 0 selects uneven split-K over the full contraction length (K is ignored).
    ``colsum`` (bf16 output only): fp32 [M/bm][>=N] receives per-row-tile column sums of the
    stored output; requires explicit ``tiles`` so the caller knows the partial count."""
    if k_total:
        K = k_total
    act = _act(act)
    out_f32 = c.dtype == torch.float32
    if colsum is not None:
        if tiles is None or out_f32:
            raise ValueError("colsum needs explicit tiles and a bf16 output")
        if colsum.dtype != torch.float32 or colsum.dim() != 2 or colsum.stride(1) != 1 or \
                colsum.shape[0] < -(-M // tiles[0]) or colsum.shape[1] < N:
            raise ValueError(f"colsum must be fp32 [{-(-M // tiles[0])}][>={N}] row-major")
    if (mask_out is not None or mask_in is not None) and not a.is_cuda:
        raise ValueError("relu bit masks are a GPU-path format (CPU uses aux)")
    frag = isinstance(mask_out, FragMask) or isinstance(mask_in, FragMask)
    for m in (mask_out, mask_in):
        if isinstance(m, FragMask):
            if tiles is None or tuple(tiles) != m.tiles or stages not in DIRECT_STAGES or \
                    m.m < M or m.n < N or m.buf.numel() < FragMask.nbytes(M, N, m.tiles):
                raise ValueError(f"fragment mask of tile {m.tiles} [{m.m}][{m.n}] used by a "
                                 f"{tiles} GEMM (stage code {stages}) of [{M}][{N}]")
        elif m is not None and frag:
            raise ValueError("mask_out and mask_in must share one layout")
    for m in () if frag else (mask_out, mask_in):  # row-block-major bytes (relu_mask_bits)
        if m is not None and (m.dtype != torch.uint8 or m.dim() != 2 or not m.is_contiguous() or
                              M % 16 or m.shape[0] < M or m.shape[1] < -(-N // 8)):
            raise ValueError(f"relu mask must be a contiguous uint8 [{M}][>={-(-N // 8)}] "
                             "tensor and M a multiple of 16")
    if ct is not None and (ct.dtype != torch.bfloat16 or ct.dim() != 2 or ct.stride(1) != 1 or
                           ct.shape[0] < N or ct.shape[1] < M or (out_f32 and upd is None)):
        raise ValueError(f"ct must be a bf16 [>={N}][>={M}] row-major transposed output")
    if upd is not None:
        # fused SGD epilogue (f32 output of one split): the gradient updates the weights in place
        # -- upd = dict(master=fp32 [M][N] view (row stride = C's), mom=None | same shape,
        # shadow=None | bf16 same shape, lr_dev=fp32 [1], momentum, weight_decay); ct = W^T
        if not out_f32 or splits != 1 or accumulate or bias is not None:
            raise ValueError("fused update: f32 output, one split, no accumulation / bias")
        for k in ("master", "mom", "shadow"):
            t = upd.get(k)
            if t is not None and (t.dim() != 2 or t.stride(1) != 1 or t.shape[0] < M or
                                  t.shape[1] < N or t.stride(0) != (c if c.dim() == 2
                                                                    else c[0]).stride(0)):
                raise ValueError(f"fused update: {k} must be [M][N] with C's row stride")
    if stages in DIRECT_STAGES and (ct is not None or upd is not None):
        stages = RP_STAGED  # the register-direct epilogue has neither: same loop, staged
    if not a.is_cuda:
        ref.gemm(a, b, c, layout_a=layout_a, layout_b=layout_b, M=M, N=N, K=K, bias=bias,
                 aux=aux, act=act, accumulate=accumulate, splits=splits, colsum=colsum,
                 colsum_rows=tiles[0] if tiles else 0, k_total=k_total)
        if upd is not None:
            g = (c if c.dim() == 2 else c[0])[:M, :N]
            mom = upd.get("mom")
            sh = upd.get("shadow")
            ref.sgd_update(upd["master"][:M, :N], g, mom[:M, :N] if mom is not None else None,
                           sh[:M, :N] if sh is not None else None, float(upd["lr_dev"][0]),
                           upd.get("momentum", 0.0), upd.get("weight_decay", 0.0))
            if ct is not None:
                ct[:N, :M] = upd["master"][:M, :N].t().to(torch.bfloat16)
            return c
        if ct is not None:
            ct[:N, :M] = c[:M, :N].t()
        return c
    _rows(a, "A", torch.bfloat16)
    _rows(b, "B", torch.bfloat16)
    if splits > 1:
        if c.dim() != 3 or c.shape[0] < splits:
            raise ValueError("split-K output must be [splits][M][N] fp32")
        c_rows, split_stride = c[0], c.stride(0)
    else:
        c_rows, split_stride = (c if c.dim() == 2 else c[0]), 0
    _rows(c_rows, "C", torch.float32 if out_f32 else torch.bfloat16)
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() < N):
        raise ValueError("bias must be fp32 with >= N entries")
    if aux is not None:
        _rows(aux, "aux", torch.bfloat16)
    # shape checks against the storage the kernel will touch
    ka = k_total or K * splits
    need_a = (M, ka) if layout_a == KMAJ else (ka, M)
    need_b = (N, ka) if layout_b == KMAJ else (ka, N)
    if a.shape[0] < need_a[0] or a.shape[1] < need_a[1]:
        raise ValueError(f"A storage {tuple(a.shape)} too small for {need_a}")
    if b.shape[0] < need_b[0] or b.shape[1] < need_b[1]:
        raise ValueError(f"B storage {tuple(b.shape)} too small for {need_b}")
    if c_rows.shape[0] < M or c_rows.shape[1] < N:
        raise ValueError(f"C storage {tuple(c_rows.shape)} too small for {(M, N)}")
    if aux is not None and (aux.shape[0] < M or aux.shape[1] < N):
        raise ValueError("aux storage too small")
    bm, bn = tiles or pick_tiles(M, N, splits)
    # M or N not a multiple of the tile runs as partial edge tiles in the same launch:
    # out-of-range operand rows/columns are clamped on load and never stored (gemm.hip)
    native().gemm_bf16(_p(a), a.stride(0), _p(b), b.stride(0), _p(c_rows), c_rows.stride(0),
                       split_stride, _p(bias), _p(aux), aux.stride(0) if aux is not None else 0,
                       M, N, K, act, int(accumulate), layout_a, layout_b, int(out_f32), bm, bn,
                       splits, _stream(a), _p(colsum),
                       colsum.stride(0) if colsum is not None else 0, k_total=int(k_total),
                       stages=int(stages), group_m=int(group_m), persist=int(persist),
                       mask_out=_p(mask_out.buf if frag and mask_out is not None else mask_out),
                       mask_in=_p(mask_in.buf if frag and mask_in is not None else mask_in),
                       ld_mask=-1 if frag else
                       (mask_out if mask_out is not None else mask_in).stride(0)
                       if (mask_out is not None or mask_in is not None) else 0,
                       ct=_p(ct), ld_ct=ct.stride(0) if ct is not None else 0,
                       **({} if upd is None else dict(
                           upd_master=_p(upd["master"]), upd_mom=_p(upd.get("mom")),
                           upd_shadow=_p(upd.get("shadow")), upd_lr=_p(upd["lr_dev"]),
                           upd_mu=float(upd.get("momentum", 0.0)),
                           upd_wd=float(upd.get("weight_decay", 0.0)))),
                       timeline=_p(timeline), epi_probe=int(epi_probe) | _EPI_GENERIC)
    return c


# ---- the three GEMMs of a Linear layer -----------------------------------------------------


def gemv(x, w, bias, y, act="relu"):
    """Serving-size layer (1..8 rows): y[m][n] = act(x[m] . w[n] + bias[n]), one wave per
    output neuron (csrc/kernels/gemv.hip). y bf16 or fp32."""
    M, K = x.shape
    N = w.shape[0]
    if not x.is_cuda:
        return ref.gemm(x, w, y, layout_a=KMAJ, layout_b=KMAJ, M=M, N=N, K=K, bias=bias,
                        act=_act(act))
    if M > GEMV_MAX_ROWS or K % 8:
        raise ValueError(f"gemv takes <= {GEMV_MAX_ROWS} rows and K % 8 == 0")
    _rows(x, "x", torch.bfloat16)
    _rows(w, "w", torch.bfloat16)
    if w.shape[1] < K or y.shape[0] < M or y.shape[1] < N or y.stride(1) != 1:
        raise ValueError("gemv operand shapes do not match")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() < N):
        raise ValueError("bias must be fp32 with >= N entries")
    native().gemv_bf16(_p(x), x.stride(0), _p(w), w.stride(0), _p(bias), _p(y), y.stride(0),
                       M, N, K, _act(act), int(y.dtype == torch.float32), _stream(x))
    return y


class FragMask:
    """1-bit ReLU mask in FRAGMENT order (GemmParams::ld_mask < 0, gemm_tile.hpp
    frag_mask_offset): the bits a lane of the register-direct epilogue stores or reads are
    contiguous, so one 4/8/16-byte access per lane moves them, instead of the row-block-major
    layout's one-byte accesses (the reason DNN_RELU_MASK=1 measured slower than reading the
    activation). Tied to one tile shape: the forward that writes it and the dgrad that reads it
    must both run ``tiles`` with a register-direct stage code. Tiles are row-major in the
    buffer, so the rows of a micro-batch starting on a tile boundary are one byte range
    (``mask[r]`` with r a slice of rows)."""

    def __init__(self, buf: torch.Tensor, tiles: tuple[int, int], m: int, n: int):
        self.buf, self.tiles, self.m, self.n = buf, tuple(tiles), m, n

    @staticmethod
    def nbytes(M: int, N: int, tiles) -> int:
        bm, bn = tiles
        return -(-M // bm) * -(-N // bn) * bm * bn // 8

    @classmethod
    def alloc(cls, M: int, N: int, tiles, device) -> "FragMask":
        if tuple(tiles) not in FRAG_WAVES:
            raise ValueError(f"no fragment-order mask for tile {tuple(tiles)}")
        return cls(torch.zeros(cls.nbytes(M, N, tiles), dtype=torch.uint8, device=device),
                   tiles, M, N)

    def __getitem__(self, r: slice) -> "FragMask":
        bm, bn = self.tiles
        start, stop, step = r.indices(self.m)
        if step != 1 or start % bm:
            raise ValueError(f"fragment mask rows must start on a {bm}-row tile boundary")
        per_row_tile = -(-self.n // bn) * bm * bn // 8
        return FragMask(self.buf[start // bm * per_row_tile:], self.tiles, stop - start, self.n)

    def bits(self) -> torch.Tensor:
        """Unpack into bool [m][n] (tests)."""
        bm, bn = self.tiles
        wm_n, wn_n = FRAG_WAVES[self.tiles]
        fm, sn = bm // wm_n // 16, bn // wn_n
        fn = sn // 16
        tm_n, tn_n = -(-self.m // bm), -(-self.n // bn)
        dev = self.buf.device
        raw = self.buf[:tm_n * tn_n * bm * bn // 8].view(tm_n, tn_n, wm_n, wn_n, 64, fn // 2, fm)
        ar = lambda k: torch.arange(k, device=dev)  # noqa: E731
        tm, tn, wm, wn, lane, jj, i, e = torch.meshgrid(
            ar(tm_n), ar(tn_n), ar(wm_n), ar(wn_n), ar(64), ar(fn // 2), ar(fm), ar(8),
            indexing="ij")
        row = tm * bm + wm * 16 * fm + (lane & 15) + 16 * i
        col = tn * bn + wn * sn + 16 * ((lane >> 4) & 1) + 8 * (lane >> 5) + 32 * jj + e
        bit = (raw.unsqueeze(-1).to(torch.int32) >> ar(8).to(torch.int32)) & 1
        out = torch.zeros(tm_n * bm, tn_n * bn, dtype=torch.bool, device=dev)
        out[row.reshape(-1), col.reshape(-1)] = bit.reshape(-1).bool()
        return out[:self.m, :self.n]


def relu_mask_bits(mask: torch.Tensor, M: int, N: int) -> torch.Tensor:
    """Unpack a GEMM-written ReLU mask (uint8 [M][ld], row-block-major: the byte of row r,
    8-column chunk c is at flat index ((r // 16) * ld + c) * 16 + r % 16) into bool [M][N]."""
    ld = mask.shape[1]
    blocks = mask.reshape(-1)[:M * ld].view(M // 16, ld, 16).transpose(1, 2).reshape(M, ld)
    bits = (blocks[:, :(N + 7) // 8].to(torch.int32).unsqueeze(-1) >>
            torch.arange(8, device=mask.device, dtype=torch.int32)) & 1
    return bits.reshape(M, -1)[:, :N].bool()


def linear_fwd(x, w, bias, y, act="relu", mask=None, yt=None):
    """y[M][Np] = act(x[M][Kp] . w[Np][Kp]^T + bias). y bf16 (activation) or fp32 (logits).
    M <= 8 rows (serving) runs the GEMV kernel; otherwise the MFMA GEMM. ``mask`` (GPU, relu):
    also write the 1-bit mask of y for the next dgrad. ``yt`` (bf16 [Np][>=M], may be a column
    slice): also write y transposed (the next layer's weight gradient reads it K-major)."""
    M, K = x.shape
    N = w.shape[0]
    if not x.is_cuda:  # CPU reference: any row count
        return gemm(x, w, y, layout_a=KMAJ, layout_b=KMAJ, M=M, N=N, K=K, bias=bias, act=act,
                    ct=yt)
    if M <= GEMV_MAX_ROWS:
        return gemv(x, w, bias, y, act)
    p = plan("fwd", M, N, K)
    if mask is None and act in ("relu", "linear", 0, 1) and p.blas and \
            _blas_ok(x, w, y, False, True, M, N, K, bias, _act(act) == 1, False):
        return blas_gemm(x, w, y, trans_a=False, trans_b=True, M=M, N=N, K=K, bias=bias,
                         relu=_act(act) == 1, algo=p.blas_algo)
    return gemm(x, w, y, layout_a=KMAJ, layout_b=KMAJ, M=M, N=N, K=K, bias=bias, act=act,
                mask_out=mask, ct=yt, **p.launch_args(mask=mask is not None, ct=yt is not None))


def linear_fwd_xent(x, w, bias, dz, labels, n_cls, scale, loss_part=None, correct=None,
                    colsum=None):
    """Last layer + softmax cross-entropy in ONE kernel: dz[M][Np] = (softmax(x.w^T + b) -
    onehot) * scale; loss_part[M/bm] per-tile loss sums; correct[M/bm] per-tile #argmax==label;
    colsum[M/bm][Np] = per-tile column sums of dz (the bias-gradient partials)."""
    M, K = x.shape
    N = w.shape[0]
    p = plan("xent", M, N, K)
    bm, bn = p.tiles
    if labels.dtype != torch.int32 or labels.numel() < M:
        raise ValueError("labels must be int32 with one entry per row")
    if loss_part is not None and loss_part.numel() < M // bm:
        raise ValueError(f"loss_part needs {M // bm} entries")
    if correct is not None and (correct.dtype != torch.int32 or correct.numel() < M // bm):
        raise ValueError(f"correct needs {M // bm} int32 entries")
    if not x.is_cuda:
        logits = torch.empty(M, N, dtype=torch.float32)
        ref.gemm(x, w, logits, layout_a=KMAJ, layout_b=KMAJ, M=M, N=N, K=K, bias=bias)
        ref.softmax_xent(logits, labels, dz, n_cls, scale, loss_part, correct, bm, colsum)
        return dz
    _rows(x, "x", torch.bfloat16)
    _rows(w, "w", torch.bfloat16)
    _rows(dz, "dz", torch.bfloat16)
    if colsum is not None and (colsum.dtype != torch.float32 or colsum.shape[0] < M // bm or
                               colsum.shape[1] < N or colsum.stride(1) != 1):
        raise ValueError(f"colsum must be fp32 [{M // bm}][>={N}]")
    if bias is None or bias.dtype != torch.float32 or bias.numel() < N:
        raise ValueError("fused cross-entropy needs an fp32 bias")
    native().gemm_bf16(_p(x), x.stride(0), _p(w), w.stride(0), _p(dz), dz.stride(0), 0,
                       _p(bias), 0, 0, M, N, K, 0, 0, KMAJ, KMAJ, 0, bm, bn, 1, _stream(x),
                       _p(colsum), colsum.stride(0) if colsum is not None else 0, _p(labels),
                       int(n_cls), float(scale), _p(loss_part), _p(correct),
                       stages=p.stages)
    return dz


def transpose_bf16(src, dst):
    """dst[c][r] = src[r][c] (bf16, both dims multiples of 64)."""
    rows, cols = src.shape
    if dst.shape[0] < cols or dst.shape[1] < rows:
        raise ValueError(f"transpose_bf16: dst {tuple(dst.shape)} too small for {(cols, rows)}")
    if not src.is_cuda:
        dst[:cols, :rows] = src.t()
        return dst
    _rows(src, "src", torch.bfloat16)
    _rows(dst, "dst", torch.bfloat16)
    native().transpose_bf16(_p(src), src.stride(0), rows, cols, _p(dst), dst.stride(0),
                            _stream(src))
    return dst


def transpose_multi(pairs):
    """transpose_bf16 for every (src, dst) pair, one launch on the GPU (<= 16 pairs)."""
    pairs = list(pairs)
    if not pairs:
        return
    if not pairs[0][0].is_cuda:
        for src, dst in pairs:
            transpose_bf16(src, dst)
        return
    jobs = []
    for src, dst in pairs:
        rows, cols = src.shape
        _rows(src, "src", torch.bfloat16)
        _rows(dst, "dst", torch.bfloat16)
        if dst.shape[0] < cols or dst.shape[1] < rows:
            raise ValueError("transpose_multi: dst too small")
        jobs.append((_p(src), src.stride(0), rows, cols, _p(dst), dst.stride(0)))
    for k in range(0, len(jobs), 16):
        native().transpose_multi(jobs[k:k + 16], _stream(pairs[0][0]))


FP8_MAX = 448.0  # OCP e4m3 (gfx950's fp8; not the fnuz variant of MI300)


FP8_TINY_AMAX = 2.0 ** -110  # rows below it are sent as zeros (csrc/kernels/elementwise.hpp)


def quant_rows_fp8(x, q, scale):
    """Pipeline-boundary compression: q[r] = e4m3(x[r] * inv[r]), scale[r] = amax(x[r]) / 448,
    inv[r] = 448 / amax(x[r]): both quotients IEEE-rounded fp32, the product one fp32 multiply,
    the e4m3 rounding to nearest with ties to even (tests/_fp8_oracle.py is the exact reference
    of both paths). A row with amax < FP8_TINY_AMAX (2^-110) is sent as a zero row (scale = 0,
    codes +-0, dequantised +-0): 448 / amax overflows below ~1.3e-36 and would turn the row into
    NaN. A NaN or +-inf element comes back non-finite at its position; a row holding one is not
    otherwise specified. x bf16 [rows][cols], q uint8 [rows][>=cols], scale fp32 [rows]."""
    rows, cols = x.shape
    if q.dtype != torch.uint8 or q.shape[0] < rows or q.shape[1] < cols or scale.numel() < rows:
        raise ValueError("quant_rows_fp8: q must be uint8 [rows][>=cols], scale fp32 [>=rows]")
    if not x.is_cuda:
        xf = x.float()
        amax = xf.abs().amax(1)
        send = amax >= FP8_TINY_AMAX  # False for a zero row and for a NaN amax
        zero, top = torch.zeros_like(amax), torch.full_like(amax, FP8_MAX)
        # tensor / tensor is the correctly rounded quotient; scalar / tensor multiplies by a
        # reciprocal and is one ulp off in a quarter of the rows
        inv = torch.where(send, top / amax, zero)
        q[:rows, :cols] = (xf * inv[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
        scale[:rows] = torch.where(send, amax / top, zero)
        return
    _rows(x, "x", torch.bfloat16)
    native().quant_rows_fp8(_p(x), x.stride(0), rows, cols, _p(q), q.stride(0), _p(scale),
                            _stream(x))


def dequant_rows_fp8(q, scale, x):
    """Inverse of quant_rows_fp8 into bf16 x [rows][cols]."""
    rows, cols = x.shape
    if not x.is_cuda:
        v = q[:rows, :cols].view(torch.float8_e4m3fn).float() * scale[:rows, None]
        x.copy_(v.to(torch.bfloat16))
        return
    _rows(x, "x", torch.bfloat16)
    native().dequant_rows_fp8(_p(q), q.stride(0), _p(scale), rows, cols, _p(x), x.stride(0),
                              _stream(x))


def gemv_fp8(x, q, scale, bias, y, act="relu"):
    """Serving-size layer (1..8 rows) over fp8 weight rows in the format of quant_rows_fp8:
    y[m][n] = act(fl32(scale[n] * sum_k x[m][k] * e4m3(q[n][k])) + bias[n]), one wave per output
    neuron, the scale applied once to the reduced sum (csrc/kernels/gemv_fp8.hip). x bf16
    [M][K], q uint8 [N][>=K] e4m3 codes, scale fp32 [>=N], y bf16 or fp32; K % 16 == 0."""
    M, K = x.shape
    N = q.shape[0]
    if M > GEMV_MAX_ROWS or K % 16:
        raise ValueError(f"gemv_fp8 takes <= {GEMV_MAX_ROWS} rows and K % 16 == 0")
    _rows(x, "x", torch.bfloat16)
    _rows(q, "q", torch.uint8)
    if q.shape[1] < K or y.shape[0] < M or y.shape[1] < N or y.stride(1) != 1:
        raise ValueError("gemv_fp8 operand shapes do not match")
    if y.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("y must be bf16 or fp32")
    if scale.dtype != torch.float32 or scale.numel() < N or not scale.is_contiguous():
        raise ValueError("scale must be contiguous fp32 with >= N entries")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() < N):
        raise ValueError("bias must be fp32 with >= N entries")
    if not x.is_cuda:
        return ref.gemv_fp8(x, q, scale, bias, y, M, N, K, _act(act))
    native().gemv_fp8(_p(x), x.stride(0), _p(q), q.stride(0), _p(scale), _p(bias), _p(y),
                      y.stride(0), M, N, K, _act(act), int(y.dtype == torch.float32), _stream(x))
    return y


MXFP4_BLOCK = 32  # columns that share one e8m0 scale byte (csrc/kernels/mxfp4.hpp)


def _mxfp4_operands(name, rows, cols, q, e):
    if cols % MXFP4_BLOCK:
        raise ValueError(f"{name} takes cols % {MXFP4_BLOCK} == 0")
    _rows(q, "q", torch.uint8)
    _rows(e, "e", torch.uint8)
    if (q.shape[0] < rows or q.shape[1] < cols // 2 or e.shape[0] < rows
            or e.shape[1] < cols // MXFP4_BLOCK):
        raise ValueError(f"{name}: q must be uint8 [rows][>=cols/2], e uint8 [rows][>=cols/32]")


def quant_rows_mxfp4(x, q, e):
    """OCP MXFP4 weight rows: per block of 32 columns one e8m0 scale byte E and 32 e2m1 codes
    (magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6}, bit 3 the sign), column 2j in the low nibble of
    byte j. Per block: amax < 2^-110 gives E = 0 and nibbles 0x0; otherwise E = floor(log2 amax)
    - 2 + 127, t = x * 2^(127 - E) (exact), |t| > 6 saturates, else the nearest magnitude with a
    tie to the even code; the sign bit is kept (tests/_mxfp4_oracle.py is the exact reference of
    both paths). x bf16 [rows][cols], q uint8 [rows][>=cols/2], e uint8 [rows][>=cols/32];
    cols % 32 == 0. Rows holding NaN or infinity are not specified."""
    rows, cols = x.shape
    _rows(x, "x", torch.bfloat16)
    _mxfp4_operands("quant_rows_mxfp4", rows, cols, q, e)
    if not x.is_cuda:
        return ref.quant_rows_mxfp4(x, q, e)
    native().quant_rows_mxfp4(_p(x), x.stride(0), rows, cols, _p(q), q.stride(0), _p(e),
                              e.stride(0), _stream(x))


def dequant_rows_mxfp4(q, e, x):
    """Inverse of quant_rows_mxfp4 into bf16 x [rows][cols]: dec(code) * 2^(E - 127), exact
    (no rounding) for every E the quantiser writes; a block with E == 0 gives +0."""
    rows, cols = x.shape
    _rows(x, "x", torch.bfloat16)
    _mxfp4_operands("dequant_rows_mxfp4", rows, cols, q, e)
    if not x.is_cuda:
        return ref.dequant_rows_mxfp4(q, e, x)
    native().dequant_rows_mxfp4(_p(q), q.stride(0), _p(e), e.stride(0), rows, cols, _p(x),
                                x.stride(0), _stream(x))


def gemv_mxfp4(x, q, e, bias, y, act="relu"):
    """Serving-size layer (1..8 rows) over MXFP4 weight rows in the format of quant_rows_mxfp4:
    y[m][n] = act(sum_k x[m][k] * e2m1(q[n][k]) * 2^(e[n][k / 32] - 127) + bias[n]), one wave per
    output neuron, the block scale applied inside the hardware decode
    (csrc/kernels/gemv_mxfp4.hip). x bf16 [M][K], q uint8 [N][>=K/2], e uint8 [N][>=K/32], y
    bf16 or fp32; K % 32 == 0."""
    M, K = x.shape
    N = q.shape[0]
    if M > GEMV_MAX_ROWS or K % MXFP4_BLOCK:
        raise ValueError(f"gemv_mxfp4 takes <= {GEMV_MAX_ROWS} rows and K % {MXFP4_BLOCK} == 0")
    _rows(x, "x", torch.bfloat16)
    _mxfp4_operands("gemv_mxfp4", N, K, q, e)
    if y.shape[0] < M or y.shape[1] < N or y.stride(1) != 1:
        raise ValueError("gemv_mxfp4 operand shapes do not match")
    if y.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("y must be bf16 or fp32")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() < N):
        raise ValueError("bias must be fp32 with >= N entries")
    if not x.is_cuda:
        return ref.gemv_mxfp4(x, q, e, bias, y, M, N, K, _act(act))
    native().gemv_mxfp4(_p(x), x.stride(0), _p(q), q.stride(0), _p(e), e.stride(0), _p(bias),
                        _p(y), y.stride(0), M, N, K, _act(act), int(y.dtype == torch.float32),
                        _stream(x))
    return y


# Largest row bucket the serving engine runs on linear_fwd_fp8 under fp8_gemm="direct"; larger
# buckets keep the dequantise-into-scratch path. Measured (bench/linear_fp8_bench.py,
# profiles/linear_fp8/linear_fp8_bench.jsonl): the largest power-of-two bucket at which direct
# beats scratch on both layers (1024 x 1024 resident, 8192 x 8192 cold) by more than the larger
# of the two spreads. 1024 is also the largest bucket measured: 7.8 vs 14.4 us and 165.7 vs
# 170.2 us (spreads <= 1 %); the margin on the large layer is 3 % there, so nothing above it
# is claimed.
FP8_DIRECT_MAX_ROWS = 1024


def linear_fwd_fp8(x, q, scale, bias, y, act="relu", tile=0):
    """Forward layer over fp8 weight rows in the format of quant_rows_fp8, any number of rows:
    y[m][n] = act(fl32(scale[n] * sum_k x[m][k] * e4m3(q[n][k])) + bias[n]) -- gemv_fp8's
    definition. Up to GEMV_MAX_ROWS rows run gemv_fp8; more rows run the MFMA kernel that takes
    the codes as its weight operand (csrc/kernels/linear_fp8.hip; no bf16 copy of the weights).
    x bf16 [M][K], q uint8 [N][>=K] e4m3 codes, scale fp32 [>=N], y bf16 or fp32; K % 16 == 0.
    ``tile``: 0 = chosen by the launcher, 1..4 force one (linear_fp8.hpp; tests, benchmark)."""
    M, K = x.shape
    N = q.shape[0]
    if K % 16:
        raise ValueError("linear_fwd_fp8 takes K % 16 == 0")
    _rows(x, "x", torch.bfloat16)
    _rows(q, "q", torch.uint8)
    if q.shape[1] < K or y.shape[0] < M or y.shape[1] < N or y.stride(1) != 1:
        raise ValueError("linear_fwd_fp8 operand shapes do not match")
    if y.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("y must be bf16 or fp32")
    if scale.dtype != torch.float32 or scale.numel() < N or not scale.is_contiguous():
        raise ValueError("scale must be contiguous fp32 with >= N entries")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() < N):
        raise ValueError("bias must be fp32 with >= N entries")
    if not x.is_cuda:
        return ref.gemv_fp8(x, q, scale, bias, y, M, N, K, _act(act))
    if M <= GEMV_MAX_ROWS and not tile:
        return gemv_fp8(x, q, scale, bias, y, act)
    native().linear_fp8(_p(x), x.stride(0), _p(q), q.stride(0), _p(scale), _p(bias), _p(y),
                        y.stride(0), M, N, K, _act(act), int(y.dtype == torch.float32),
                        _stream(x), tile)
    return y


def linear_w8a8(xq, sx, q, scale, bias, y, act="relu", tile=0):
    """Forward layer with e4m3 codes on both operands, each in the format of quant_rows_fp8:
    y[m][n] = act(fl32(sx[m] * fl32(scale[n] * sum_k e4m3(xq[m][k]) * e4m3(q[n][k]))) + bias[n])
    on the fp8 MFMA (csrc/kernels/linear_w8a8.hip): the weight scale first, the row scale
    second, each a rounded fp32 multiply of its own. xq uint8 [M][>=K] codes of the rows, sx fp32
    [>=M], q uint8 [N][>=K] codes of the weights, scale fp32 [>=N], y bf16 or fp32; K % 16 == 0,
    rows of codes 16-byte aligned, any M >= 1.
    ``tile``: 0 = chosen by the launcher, 1 / 2 force one (linear_w8a8.hpp; tests, benchmark)."""
    M, K = xq.shape
    N = q.shape[0]
    if K % 16:
        raise ValueError("linear_w8a8 takes K % 16 == 0")
    _rows(xq, "xq", torch.uint8)
    _rows(q, "q", torch.uint8)
    if q.shape[1] < K or y.shape[0] < M or y.shape[1] < N or y.stride(1) != 1:
        raise ValueError("linear_w8a8 operand shapes do not match")
    if y.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("y must be bf16 or fp32")
    if sx.dtype != torch.float32 or sx.numel() < M or not sx.is_contiguous():
        raise ValueError("sx must be contiguous fp32 with >= M entries")
    if scale.dtype != torch.float32 or scale.numel() < N or not scale.is_contiguous():
        raise ValueError("scale must be contiguous fp32 with >= N entries")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() < N):
        raise ValueError("bias must be fp32 with >= N entries")
    if not xq.is_cuda:
        return ref.linear_w8a8(xq, sx, q, scale, bias, y, M, N, K, _act(act))
    native().linear_w8a8(_p(xq), xq.stride(0), _p(sx), _p(q), q.stride(0), _p(scale), _p(bias),
                         _p(y), y.stride(0), M, N, K, _act(act), int(y.dtype == torch.float32),
                         _stream(xq), tile)
    return y


def linear_fwd_w8a8(x, q, scale, bias, y, act="relu", xq=None, sx=None, tile=0):
    """A layer served with fp8 activations: quant_rows_fp8(x) into ``xq`` / ``sx`` (uint8
    [>=M][>=K] with 16-byte aligned rows and fp32 [>=M]; temporaries when not given), then
    linear_w8a8 on them. x bf16 [M][K]; everything else as linear_w8a8. Every column of x enters
    its row's amax, so the answer differs from linear_fwd_fp8's within the activation format's
    bound (tests/_fp8_oracle.round_trip_bound) unless the quantiser loses nothing."""
    M, K = x.shape
    if K % 16:
        raise ValueError("linear_fwd_w8a8 takes K % 16 == 0")
    _rows(x, "x", torch.bfloat16)
    if xq is None:
        xq = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    if sx is None:
        sx = torch.empty(M, dtype=torch.float32, device=x.device)
    quant_rows_fp8(x, xq, sx)
    return linear_w8a8(xq[:M, :K], sx, q, scale, bias, y, act, tile)


W4A8_TILES = 2  # csrc/kernels/linear_w4a8.hpp LINEAR_W4A8_TILES (asserted on the GPU path)


def linear_w4a8(xq, sx, q, e, bias, y, act="relu", tile=0):
    """Forward layer over MXFP4 weight rows (quant_rows_mxfp4) against e4m3 activation rows
    (quant_rows_fp8): y[m][n] = act(fl32(sx[m] * sum_k e4m3(xq[m][k]) * e2m1(q[n][k]) *
    2^(e[n][k / 32] - 127)) + bias[n]) on the block-scaled MFMA in its fp4 x fp8 form
    (csrc/kernels/linear_w4a8.hip): the block scales are the instruction's scale operand, the
    row scale one rounded fp32 multiply in the epilogue; a block with scale byte 0 contributes
    nothing. xq uint8 [M][>=K] codes of the rows, sx fp32 [>=M], q uint8 [N][>=K/2], e uint8
    [N][>=K/32] (any alignment), y bf16 or fp32; K % 32 == 0, rows of xq and q 16-byte aligned,
    any M >= 1.
    ``tile``: 0 = chosen by the launcher, 1 / 2 force one (linear_w4a8.hpp; tests, benchmark)."""
    M, K = xq.shape
    N = q.shape[0]
    if K % MXFP4_BLOCK:
        raise ValueError(f"linear_w4a8 takes K % {MXFP4_BLOCK} == 0")
    _rows(xq, "xq", torch.uint8)
    _mxfp4_operands("linear_w4a8", N, K, q, e)
    if y.shape[0] < M or y.shape[1] < N or y.stride(1) != 1:
        raise ValueError("linear_w4a8 operand shapes do not match")
    if y.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("y must be bf16 or fp32")
    if sx.dtype != torch.float32 or sx.numel() < M or not sx.is_contiguous():
        raise ValueError("sx must be contiguous fp32 with >= M entries")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() < N):
        raise ValueError("bias must be fp32 with >= N entries")
    if not 0 <= int(tile) <= W4A8_TILES:
        raise ValueError(f"linear_w4a8 tile must be 0..{W4A8_TILES}")
    if not xq.is_cuda:
        return ref.linear_w4a8(xq, sx, q, e, bias, y, M, N, K, _act(act))
    assert native().linear_w4a8_tiles() == W4A8_TILES
    for name, t in (("xq", xq), ("q", q)):
        if t.data_ptr() % 16 or t.stride(0) % 16:
            raise ValueError(f"linear_w4a8: rows of {name} must be 16-byte aligned")
    native().linear_w4a8(_p(xq), xq.stride(0), _p(sx), _p(q), q.stride(0), _p(e), e.stride(0),
                         _p(bias), _p(y), y.stride(0), M, N, K, _act(act),
                         int(y.dtype == torch.float32), _stream(xq), int(tile))
    return y


def linear_fwd_w4a8(x, q, e, bias, y, act="relu", xq=None, sx=None, tile=0):
    """A layer served from MXFP4 weights with fp8 activations: quant_rows_fp8(x) into ``xq`` /
    ``sx`` (uint8 [>=M][>=K] with 16-byte aligned rows and fp32 [>=M]; temporaries when not
    given), then linear_w4a8 on them. x bf16 [M][K]; everything else as linear_w4a8. Every
    column of x enters its row's amax, so the answer differs from gemv_mxfp4's within the
    activation format's bound (tests/_fp8_oracle.round_trip_bound) unless the quantiser loses
    nothing."""
    M, K = x.shape
    if K % MXFP4_BLOCK:
        raise ValueError(f"linear_fwd_w4a8 takes K % {MXFP4_BLOCK} == 0")
    _rows(x, "x", torch.bfloat16)
    if xq is None:
        xq = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    if sx is None:
        sx = torch.empty(M, dtype=torch.float32, device=x.device)
    quant_rows_fp8(x, xq, sx)
    return linear_w4a8(xq[:M, :K], sx, q, e, bias, y, act, tile)


def linear_dgrad(dz, w, dx, y_prev=None, act_prev="linear", colsum=None, mask_prev=None,
                 wt=None, dxt=None):
    """dx[M][Kp] = (dz[M][Np] . w[Np][Kp]) * act_prev'(y_prev) (mask fused in the epilogue).
    ``colsum`` [M/bm][Kp] receives the bias-gradient partials of the PREVIOUS layer (column
    sums of dx), fused in the same epilogue. ``wt`` = w^T [Kp][Np] (the transposed weight
    shadow): the GEMM then reads both operands contraction-contiguous -- the forward's main
    loop, 1.2-1.25x faster than transposing w per tile (bench/layout_ab.py) -- with the same
    MFMA k order, so the result is bitwise identical."""
    M, N = dz.shape
    K = w.shape[1]
    if mask_prev is not None:  # relu derivative from the forward's 1-bit mask
        y_prev, act_prev = None, "relu"
    elif y_prev is None:
        act_prev = "linear"
    p = plan("dgrad", M, K, N)
    if mask_prev is None and dz.is_cuda and p.blas and \
            _blas_ok(dz, w, dx, False, False, M, K, N, None, False, False):
        blas_gemm(dz, w, dx, trans_a=False, trans_b=False, M=M, N=K, K=N, algo=p.blas_algo)
        n_part = -(-M // p.tiles[0])
        if y_prev is not None and _act(act_prev) != 0:
            dact_colsum(dx, y_prev, act_prev, colsum, n_part)
        elif colsum is not None:
            colsum_partial(dx, colsum, n_part)
        return dx
    b, layout_b = (wt, KMAJ) if wt is not None and dz.is_cuda else (w, MNMAJ)
    return gemm(dz, b, dx, layout_a=KMAJ, layout_b=layout_b, M=M, N=K, K=N, aux=y_prev,
                act=act_prev, colsum=colsum, mask_in=mask_prev, ct=dxt,
                **p.launch_args(mask=mask_prev is not None, ct=dxt is not None))


def linear_wgrad(dz, x, slabs, splits=1, accumulate=False, dzt=None, xt=None, upd=None,
                 wt=None):
    """slabs[s][Np][Kp] (+)= dz[rows_s]^T . x[rows_s] over the batch rows of split s (fp32).
    ``dzt`` / ``xt`` (bf16 [Np][R] / [Kp][R], written transposed by the producing GEMMs'
    epilogues): the contraction runs K-major on both operands (the forward's main loop,
    bench/layout_ab.py: 1.2x on 8192x8192 weights); same k order, same result bits.
    ``upd`` (one split): the epilogue applies the SGD step to the layer's weights (ops.gemm) and
    writes the new bf16 weights transposed into ``wt``. On the GPU the gradient itself is then
    NOT stored: ``slabs`` is left untouched (it only supplies the row stride that master / mom /
    shadow share). The CPU reference path does store it."""
    R, N = dz.shape
    K = x.shape[1]
    if upd is not None and (splits != 1 or accumulate):
        raise ValueError("the fused weight update needs one split and no accumulation")
    kmajor = dzt is not None and xt is not None and dz.is_cuda
    if not kmajor and (R % 64 or splits > R // 64):
        raise ValueError("rows must be a multiple of 64 with at least 64 rows per split")
    p = plan("wgrad", N, K, R, splits)
    if not kmajor and upd is None and splits == 1 and dz.is_cuda and p.blas and \
            _blas_ok(dz, x, slabs[0], True, False, N, K, R, None, False, accumulate):
        return blas_gemm(dz, x, slabs[0], trans_a=True, trans_b=False, M=N, N=K, K=R,
                         accumulate=accumulate, algo=p.blas_algo)
    a, b, layout = (dzt, xt, KMAJ) if kmajor else (dz, x, MNMAJ)
    return gemm(a, b, slabs, layout_a=layout, layout_b=layout, M=N, N=K, K=R, k_total=R,
                accumulate=accumulate, splits=splits, upd=upd, ct=wt,
                **p.launch_args(upd=upd is not None))


def linear_wgrad_group(items) -> list:
    """Several linear_wgrad calls -- items of (dz, x, slabs, splits, accumulate) -- with the
    items that share a one-tile 4-wave configuration (same tile, 2 stages, not persistent, not
    the library path) and that alone fill less than one round of the chip run as ONE grouped
    launch per configuration (gemm.hip gemm_group_kernel): small latency-bound weight gradients
    then run concurrently (batch-64 recipe step 0.034 -> 0.029 ms); big ones keep their own
    launch (grouping the mlp8 1024x1024 wgrads measured +0.4 %). Returns the indices it did NOT
    launch (the caller runs linear_wgrad for those)."""
    if not items or not items[0][0].is_cuda:
        return list(range(len(items)))
    groups, rest = {}, []
    for idx, (dz, x, slabs, splits, acc) in enumerate(items):
        R, N = dz.shape
        K = x.shape[1]
        p = plan("wgrad", N, K, R)
        bm, bn = p.tiles
        small = -(-N // bm) * -(-K // bn) * splits < int(
            switches.get("DNN_WGRAD_GROUP_MAX_WG"))  # under one round of the chip
        if (R % 64 or splits > R // 64 or p.splits != splits or p.persist or p.blas or
                (p.stages or GROUP_STAGES) != GROUP_STAGES or not small or
                (bm, bn) not in ((64, 64), (64, 128), (128, 64), (128, 128))):
            rest.append(idx)
            continue
        groups.setdefault((bm, bn), []).append(idx)
    for (bm, bn), idxs in groups.items():
        if len(idxs) < 2:
            rest += idxs
            continue
        for c0 in range(0, len(idxs), 8):
            probs = []
            for idx in idxs[c0:c0 + 8]:
                dz, x, slabs, splits, acc = items[idx]
                R, N = dz.shape
                K = x.shape[1]
                _rows(dz, "dz", torch.bfloat16)
                _rows(x, "x", torch.bfloat16)
                if slabs.dim() != 3 or slabs.shape[0] < splits or slabs.dtype != torch.float32 \
                        or slabs.shape[1] < N or slabs.shape[2] < K or slabs[0].stride(1) != 1:
                    raise ValueError("split-K output must be [splits][N][K] fp32")
                probs.append((_p(dz), dz.stride(0), _p(x), x.stride(0), _p(slabs),
                              slabs.stride(1), slabs.stride(0), N, K, R, R, int(acc), splits))
            native().gemm_bf16_group(probs, MNMAJ, MNMAJ, 1, bm, bn, GROUP_STAGES,
                                     _stream(items[0][0]))
    return sorted(rest)


STREAMK_WG = 2 * NUM_CU  # stream-K workgroups: two resident per CU, every CU equally loaded


def streamk_tiles(N: int, K: int) -> tuple[int, int]:
    """Output tile of the [N][K] weight gradient: largest tile that divides it."""
    for t in ((128, 128), (128, 64), (64, 128), (64, 64)):
        if N % t[0] == 0 and K % t[1] == 0:
            return t
    raise ValueError(f"weight shape [{N}][{K}] is not 64-aligned")


def streamk_partial_elems(N: int, K: int, nwg: int = STREAMK_WG) -> int:
    bm, bn = streamk_tiles(N, K)
    tiles = (N // bm) * (K // bn)
    return max(nwg, tiles) * 2 * bm * bn


def linear_wgrad_streamk(dz, x, grad_w, part, accumulate=False, nwg: int = STREAMK_WG):
    """grad_w[Np][Kp] (+)= dz^T . x over ALL rows, stream-K balanced; ``part`` is fp32 scratch
    of streamk_partial_elems(Np, Kp) elements."""
    R, N = dz.shape
    K = x.shape[1]
    if not dz.is_cuda:
        g = dz.float().t() @ x.float()
        if accumulate:
            grad_w += g
        else:
            grad_w.copy_(g)
        return grad_w
    _rows(dz, "dz", torch.bfloat16)
    _rows(x, "x", torch.bfloat16)
    _rows(grad_w, "grad_w", torch.float32)
    if x.shape[0] != R or grad_w.shape[0] < N or grad_w.shape[1] < K or R % 64:
        raise ValueError("wgrad shapes do not match")
    if part.dtype != torch.float32 or part.numel() < streamk_partial_elems(N, K, nwg):
        raise ValueError("stream-K partial buffer too small")
    bm, bn = streamk_tiles(N, K)
    native().gemm_bf16_streamk(_p(dz), dz.stride(0), _p(x), x.stride(0), _p(grad_w),
                               grad_w.stride(0), N, K, R, int(accumulate), MNMAJ, MNMAJ, bm, bn,
                               nwg, _p(part), _stream(dz))
    return grad_w


# ---- loss / reductions / optimizers ----------------------------------------------------------

XENT_ROWS_PER_BLOCK = 64  # csrc/kernels/elementwise.hip XENT_ROWS_PER_BLOCK


def xent_blocks(rows: int) -> int:
    """Number of per-block loss partials softmax_xent writes for ``rows`` rows."""
    return -(-rows // XENT_ROWS_PER_BLOCK)


def softmax_xent(logits, labels, dz, n_cls, scale, loss_part=None, correct=None, colsum=None):
    """dz = (softmax - onehot) * scale; per 64-row block: loss partial sum -> loss_part,
    #argmax==label -> correct (int32), and (optional) dz column sums -> colsum
    [xent_blocks(rows)][width] (bias-gradient partials).

    ``width`` = dz.shape[1] >= n_cls is any size: up to 256 columns a wave holds the row in
    registers (csrc/kernels/elementwise.hip), wider rows are swept (csrc/kernels/
    softmax_wide.hip) -- one contract, chosen inside the native launcher. Columns n_cls..width
    of dz are written as zeros; logits there, and in rows with a label < 0, are never used."""
    rows, width = dz.shape
    if rows <= 0 or not 0 < n_cls <= width:
        raise ValueError("softmax_xent: dz must be [rows][width] with 0 < n_cls <= width")
    if logits.dim() != 2 or logits.shape[0] < rows or logits.shape[1] < n_cls:
        raise ValueError("softmax_xent: logits need rows x n_cls entries")
    if loss_part is not None and loss_part.numel() < xent_blocks(rows):
        raise ValueError("loss_part needs xent_blocks(rows) entries")
    if correct is not None and (correct.dtype != torch.int32 or
                                correct.numel() < xent_blocks(rows)):
        raise ValueError("correct needs xent_blocks(rows) int32 entries")
    if colsum is not None and (colsum.dtype != torch.float32 or colsum.dim() != 2 or
                               colsum.shape[0] < xent_blocks(rows) or colsum.shape[1] < width
                               or colsum.stride(1) != 1):
        raise ValueError("colsum must be fp32 [xent_blocks(rows)][>=width]")
    if not logits.is_cuda:
        return ref.softmax_xent(logits, labels, dz, n_cls, scale, loss_part, correct,
                                XENT_ROWS_PER_BLOCK, colsum)
    _rows(logits, "logits", torch.float32)
    _rows(dz, "dz", torch.bfloat16)
    if labels.dtype != torch.int32 or labels.numel() < rows or logits.shape[0] < rows:
        raise ValueError("labels must be int32 with one entry per row")
    native().softmax_xent(_p(logits), logits.stride(0), _p(labels), _p(dz), dz.stride(0), rows,
                          n_cls, width, float(scale), _p(loss_part), _p(correct),
                          _stream(logits), _p(colsum),
                          colsum.stride(0) if colsum is not None else 0)


DENSE_LOSS_CODE = {"mse": 1, "bce": 2}  # csrc/kernels/dense_loss.hpp DenseLoss
DENSE_LOSS_ACTS = {"mse": ("linear", "relu", "sigmoid"), "bce": ("sigmoid",)}
DENSE_COLS_PER_CHUNK = 256  # csrc/kernels/dense_loss.hip DL_COLS


def dense_loss_row_blocks(rows: int) -> int:
    """Row blocks (64 rows, = xent_blocks) of one dense_loss launch over ``rows`` rows."""
    return xent_blocks(rows)


def dense_loss_col_chunks(width: int) -> int:
    """Column chunks (256 columns) of one dense_loss launch over a padded ``width``."""
    return -(-width // DENSE_COLS_PER_CHUNK)


def check_dense_loss(loss: str, act: str) -> None:
    """Raise unless ``act`` is an output activation the dense-target ``loss`` is defined for."""
    if loss not in DENSE_LOSS_ACTS:
        raise ValueError(f"unknown dense loss {loss!r} (allowed: {sorted(DENSE_LOSS_ACTS)})")
    if act not in DENSE_LOSS_ACTS[loss]:
        raise ValueError(f"loss {loss!r} needs a last activation in {DENSE_LOSS_ACTS[loss]}, "
                         f"got {act!r}")


def dense_loss(z, t, dz, n_out, scale, loss, act, row_ok=None, loss_part=None, colsum=None):
    """Dense-target loss of the output layer from its fp32 pre-activations z and bf16 targets t
    (first n_out columns; the rest is never read), y = act(z), n = n_out:
    ``mse``: loss_r = mean_c (y - t)^2, dz = (2 scale / n) (y - t) act'(z);
    ``bce`` (sigmoid, from the logits): loss_r = mean_c [max(z, 0) - t z + log1p(exp(-|z|))],
    dz = (scale / n) (sigmoid(z) - t). Rows with row_ok[r] < 0 (row_ok=None: none) are padding:
    dz = 0, no loss. dz columns n_out..width are written as 0. Per 64-row block rb and
    256-column chunk ch: loss partial -> loss_part[rb * chunks + ch]; column sums of the stored
    dz -> colsum[rb][:width] (bias-gradient partials)."""
    rows, width = dz.shape
    check_dense_loss(loss, act)
    nb, nc = dense_loss_row_blocks(rows), dense_loss_col_chunks(width)
    if rows <= 0 or width % 64 or not 0 < n_out <= width:
        raise ValueError("dense_loss: dz must be [rows][width], width a multiple of 64 >= n_out")
    if z.dim() != 2 or t.dim() != 2 or z.shape[0] < rows or t.shape[0] < rows or \
            z.shape[1] < n_out or t.shape[1] < n_out:
        raise ValueError("dense_loss: z and t need rows x n_out entries")
    if loss_part is not None and (loss_part.dtype != torch.float32 or
                                  loss_part.numel() < nb * nc):
        raise ValueError("loss_part needs dense_loss_row_blocks * dense_loss_col_chunks fp32 "
                         "entries")
    if colsum is not None and (colsum.dtype != torch.float32 or colsum.dim() != 2 or
                               colsum.shape[0] < nb or colsum.shape[1] < width
                               or colsum.stride(1) != 1):
        raise ValueError("colsum must be fp32 [xent_blocks(rows)][>=width]")
    if row_ok is not None and (row_ok.dtype != torch.int32 or row_ok.numel() < rows or
                               not row_ok.is_contiguous()):
        raise ValueError("row_ok must be int32 with one entry per row")
    if z.dtype != torch.float32 or t.dtype != torch.bfloat16 or dz.dtype != torch.bfloat16:
        raise ValueError("dense_loss: z fp32, t and dz bf16")
    if not z.is_cuda:
        return ref.dense_loss(z, t, dz, n_out, scale, DENSE_LOSS_CODE[loss], ACT_CODE[act],
                              row_ok, loss_part, colsum, XENT_ROWS_PER_BLOCK,
                              DENSE_COLS_PER_CHUNK)
    _rows(z, "z", torch.float32)
    _rows(t, "t", torch.bfloat16)
    _rows(dz, "dz", torch.bfloat16)
    native().dense_loss(_p(z), z.stride(0), _p(t), t.stride(0), _p(row_ok), _p(dz), dz.stride(0),
                        rows, n_out, width, DENSE_LOSS_CODE[loss], ACT_CODE[act], float(scale),
                        _p(loss_part), _p(colsum),
                        colsum.stride(0) if colsum is not None else 0, _stream(z))


TAIL_MAX_CLS = 16


def tail_supported(k3: int, n3: int, n4: int, n_cls: int) -> bool:
    """Geometries the fused classifier tail (csrc/kernels/mlp_tail.hip) handles."""
    return k3 in (64, 128, 256) and n3 in (64, 128) and n4 in (64, 128) and \
        1 <= n_cls <= TAIL_MAX_CLS


def tail_blocks(rows: int) -> int:
    """Partials (workgroups) of one mlp_tail launch over ``rows`` rows."""
    if rows <= 0 or rows % 16:
        raise ValueError("mlp_tail rows must be a positive multiple of 16")
    if torch.cuda.is_available():
        return int(native().mlp_tail_blocks(rows))
    return max(1, min(NUM_CU, -(-rows // ref.TAIL_BLOCK_ROWS)))


def mlp_tail(x, w3, b3, w4, b4, labels, h3, dz4, dz3, dz2, n_cls, scale, act3="relu",
             act2="relu", loss_part=None, correct=None, cs4=None, cs3=None, cs2=None):
    """The last two layers of a narrow classifier, forward AND backward, in one launch:
    h3 = act3(x.w3^T + b3); dz4 = (softmax(h3.w4^T + b4) - onehot) * scale;
    dz3 = (dz4.w4) * act3'(h3); dz2 = (dz3.w3) * act2'(x) (GPU: dz4 columns >= 16 are not
    written -- they stay the zeros the caller allocated); bias-gradient partials
    cs4/cs3/cs2 [tail_blocks(rows)][cols] and per-block loss / correct counts.
    CPU: the unfused kernels' reference path (same contract, partials per 64-row block)."""
    rows, k3 = x.shape
    n3, n4 = w3.shape[0], w4.shape[0]
    if not tail_supported(k3, n3, n4, n_cls) or w3.shape[1] != k3 or w4.shape[1] != n3:
        raise ValueError(f"mlp_tail: unsupported geometry K3={k3} N3={n3} N4={n4} "
                         f"classes={n_cls}")
    nb = tail_blocks(rows)
    for t, name, cols in ((cs4, "cs4", n4), (cs3, "cs3", n3), (cs2, "cs2", k3)):
        if t is None or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < nb or \
                t.shape[1] < cols or t.stride(1) != 1:
            raise ValueError(f"{name} must be fp32 [{nb}][>={cols}] row-major")
    if loss_part is None or loss_part.numel() < nb or correct is None or \
            correct.dtype != torch.int32 or correct.numel() < nb:
        raise ValueError(f"loss_part / correct (int32) need {nb} entries")
    if not x.is_cuda:
        ref.mlp_tail(x, w3, b3, w4, b4, labels, h3, dz4, dz3, dz2, n_cls, scale, _act(act3),
                     _act(act2), loss_part, correct, cs4, cs3, cs2, nb)
        return
    for t, name in ((x, "x"), (w3, "w3"), (w4, "w4"), (h3, "h3"), (dz4, "dz4"), (dz3, "dz3"),
                    (dz2, "dz2")):
        _rows(t, name, torch.bfloat16)
    if labels.dtype != torch.int32 or labels.numel() < rows:
        raise ValueError("labels must be int32 with one entry per row")
    native().mlp_tail(_p(x), x.stride(0), _p(w3), w3.stride(0), _p(b3), _p(w4), w4.stride(0),
                      _p(b4), _p(labels), _p(h3), h3.stride(0), _p(dz4), dz4.stride(0),
                      _p(dz3), dz3.stride(0), _p(dz2), dz2.stride(0), _p(loss_part),
                      _p(correct), _p(cs4), cs4.stride(0), _p(cs3), cs3.stride(0), _p(cs2),
                      cs2.stride(0), rows, k3, n3, n4, n_cls, float(scale), _act(act3),
                      _act(act2), _stream(x))


def softmax_rows(logits, out, n_cls, labels=None, pred=None, correct=None):
    """Inference softmax of the first n_cls columns (any n_cls; above 256 the sweeping kernel of
    csrc/kernels/softmax_wide.hip): probabilities -> out (optional, may be ``logits`` itself;
    nothing is written beyond column n_cls), argmax (lowest index on ties) -> pred (int32), and
    #argmax==label ADDED to correct[0] (int32)."""
    rows = logits.shape[0]
    if logits.dim() != 2 or rows <= 0 or not 0 < n_cls <= logits.shape[1]:
        raise ValueError("softmax_rows: logits must be [rows][>=n_cls], n_cls > 0")
    if out is not None and (out.dim() != 2 or out.shape[0] < rows or out.shape[1] < n_cls):
        raise ValueError("softmax_rows: out needs rows x n_cls entries")
    if not logits.is_cuda:
        return ref.softmax_rows(logits, out, n_cls, labels, pred, correct)
    _rows(logits, "logits", torch.float32)
    if out is not None:
        _rows(out, "out", torch.float32)
    for t, name, n in ((labels, "labels", rows), (pred, "pred", rows), (correct, "correct", 1)):
        if t is not None and (t.dtype != torch.int32 or t.numel() < n):
            raise ValueError(f"softmax_rows: {name} must be int32 with at least {n} entries")
    native().softmax_rows(_p(logits), logits.stride(0), _p(out),
                          out.stride(0) if out is not None else 0, rows, n_cls, _p(labels),
                          _p(pred), _p(correct), _stream(logits))


def colsum_partial(x, part, n_part=None):
    """part[n_part][cols] = partial column sums of x (row blocks)."""
    rows, cols = x.shape
    n_part = n_part or part.shape[0]
    if not x.is_cuda:
        return ref.colsum_partial(x, part, n_part)
    _rows(x, "x", torch.bfloat16)
    if part.dtype != torch.float32 or not part.is_contiguous() or part.numel() < n_part * cols:
        raise ValueError("part must be contiguous fp32 [n_part][cols]")
    native().colsum_partial(_p(x), x.stride(0), rows, cols, n_part, _p(part), _stream(x))


def reduce_slabs(src, n_src, stride, n, out, scale=1.0, accumulate=False):
    """out[:n] (+)= scale * sum_s src_flat[s*stride : s*stride+n]."""
    if not src.is_cuda:
        return ref.reduce_slabs(src, n_src, stride, n, out, scale, accumulate)
    if src.dtype != torch.float32 or out.dtype != torch.float32:
        raise TypeError("reduce_slabs works on fp32")
    if not (src.is_contiguous() and out.is_contiguous()):
        raise ValueError("reduce_slabs needs contiguous buffers")
    if (n_src - 1) * stride + n > src.numel() or out.numel() < n:
        raise ValueError("reduce_slabs range out of bounds")
    native().reduce_slabs(_p(src), stride, n_src, n, float(scale), _p(out), int(accumulate),
                          _stream(src))


def reduce_multi(jobs, sgd=None, max_blocks: int = 0):
    """Several reduce_slabs in ONE launch. jobs: iterable of
    (src, n_src, stride, n, out, scale, accumulate) with reduce_slabs' meaning; the results are
    bitwise identical to running reduce_slabs on each job.

    ``sgd`` (GPU): dict(grad=flat fp32 gradient the outputs live in, master=, mom=None,
    shadow=None, lr=, momentum=0, weight_decay=0, lr_dev=None) -- the same launch also applies
    the SGD step to every reduced element (bitwise equal to a following sgd_update over them).
    With adam=True (and v=, betas=, eps=, decoupled=, step_dev= as for adam_update; mom = the
    first moment) it applies the Adam / AdamW step instead, bitwise equal to adam_update; the
    caller advances step_dev afterwards.

    A job may carry an 8th element ``wt`` (GPU, fused update with a shadow only): the bf16
    W^T[cols][rows] of the layer whose [rows][cols] weight gradient the job reduces; the update
    writes it too (bitwise the transpose of the refreshed shadow).

    ``max_blocks`` (GPU, > 0): cap the launch at that many workgroups (each loops over the
    blocks; same results) -- for a reduction that runs beside other kernels."""
    jobs = [tuple(j) + (None,) * (8 - len(j)) for j in jobs]
    if not jobs:
        return
    if not jobs[0][0].is_cuda:
        for (src, n_src, stride, n, out, scale, acc, _wt) in jobs:
            ref.reduce_slabs(src, n_src, stride, n, out, scale, acc)
        if sgd is not None and sgd.get("adam"):
            adam_update(sgd["master"], sgd["grad"], sgd["mom"], sgd["v"], sgd.get("shadow"),
                        lr=sgd["lr"], betas=sgd["betas"], eps=sgd["eps"],
                        weight_decay=sgd.get("weight_decay", 0.0),
                        decoupled=sgd.get("decoupled", False), step=sgd.get("step", 1),
                        lr_dev=sgd.get("lr_dev"), step_dev=sgd.get("step_dev"))
        elif sgd is not None:
            sgd_update(sgd["master"], sgd["grad"], sgd.get("mom"), sgd.get("shadow"),
                       lr=sgd["lr"], momentum=sgd.get("momentum", 0.0),
                       weight_decay=sgd.get("weight_decay", 0.0), lr_dev=sgd.get("lr_dev"))
        return
    packed = []
    for (src, n_src, stride, n, out, scale, acc, wt) in jobs:
        if src.dtype != torch.float32 or out.dtype != torch.float32:
            raise TypeError("reduce_multi works on fp32")
        if not (src.is_contiguous() and out.is_contiguous()):
            raise ValueError("reduce_multi needs contiguous buffers")
        if (n_src - 1) * stride + n > src.numel() or out.numel() < n:
            raise ValueError("reduce_multi range out of bounds")
        if wt is not None:
            if sgd is None or sgd.get("shadow") is None:
                raise ValueError("reduce_multi: W^T output needs the fused update with a shadow")
            if wt.dtype != torch.bfloat16 or wt.dim() != 2 or not wt.is_contiguous() or \
                    wt.numel() != n or wt.shape[0] % 4:
                raise ValueError("reduce_multi: W^T must be contiguous bf16 [cols][rows] of the "
                                 "job's n elements, cols a multiple of 4")
        packed.append((_p(src), int(stride), int(n_src), int(n), _p(out), float(scale),
                       int(acc), _p(wt), int(wt.shape[0]) if wt is not None else 0))
    if sgd is None:
        native().reduce_multi(packed, _stream(jobs[0][0]), max_blocks=int(max_blocks))
        return
    g, m = sgd["grad"], sgd["master"]
    adam = bool(sgd.get("adam"))
    if adam and (sgd.get("mom") is None or sgd.get("v") is None):
        raise ValueError("fused Adam needs both moment buffers")
    for t in (m, sgd.get("mom"), sgd.get("v")):
        if t is not None and (t.dtype != torch.float32 or t.numel() != g.numel()):
            raise ValueError("fused SGD buffers must match the flat gradient")
    sh = sgd.get("shadow")
    if sh is not None and (sh.dtype != torch.bfloat16 or sh.numel() != g.numel()):
        raise ValueError("fused SGD shadow must be bf16 like the flat gradient")
    native().reduce_multi(packed, _stream(jobs[0][0]), grad_base=_p(g), master=_p(m),
                          mom=_p(sgd.get("mom")), shadow=_p(sh), lr=float(sgd["lr"]),
                          mu=float(sgd.get("momentum", 0.0)),
                          wd=float(sgd.get("weight_decay", 0.0)), lr_dev=_p(sgd.get("lr_dev")),
                          max_blocks=int(max_blocks), **(_adam_args(sgd) if adam else {}))


def _adam_args(sgd: dict) -> dict:
    b1, b2 = sgd["betas"]
    step = int(sgd.get("step", 1))
    sd = sgd.get("step_dev")
    if sd is not None and sd.dtype != torch.int32:
        raise TypeError("step_dev must be int32")
    return dict(adam=1, v=_p(sgd["v"]), b1=float(b1), b2=float(b2), eps=float(sgd["eps"]),
                decoupled=int(bool(sgd.get("decoupled", False))), step_dev=_p(sd),
                db1=float(b1), db2=float(b2), bc1=float(1.0 / (1.0 - b1 ** step)),
                bc2=float(1.0 / (1.0 - b2 ** step)))


def sgd_update(p, g, mom=None, shadow=None, lr=0.01, momentum=0.0, weight_decay=0.0,
               lr_dev=None):
    """Fused SGD over flat buffers. ``lr_dev`` (fp32 [1] device tensor): read the learning
    rate from device memory instead (replayable under an LR schedule)."""
    if not p.is_cuda:
        if lr_dev is not None:
            lr = float(lr_dev[0])
        return ref.sgd_update(p, g, mom, shadow, lr, momentum, weight_decay)
    n = p.numel()
    if g.numel() != n or (mom is not None and mom.numel() != n) or (
            shadow is not None and shadow.numel() != n):
        raise ValueError("sgd buffers must have equal sizes")
    native().sgd_update(_p(p), _p(g), _p(mom if momentum else None), _p(shadow), n, float(lr),
                        float(momentum), float(weight_decay), _stream(p), lr_dev=_p(lr_dev))


def adam_update(p, g, m, v, shadow=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                weight_decay=0.0, decoupled=False, step=1, lr_dev=None, step_dev=None):
    """Fused Adam/AdamW. ``step`` is the 1-based step of this update; with ``step_dev`` (int32
    [1] device tensor holding the number of PREVIOUS updates) and ``lr_dev`` the bias
    corrections and learning rate are taken from device memory (replayable); advance the
    counter with :func:`step_advance` after the update."""
    b1, b2 = betas
    if not p.is_cuda:
        if lr_dev is not None:
            lr = float(lr_dev[0])
        if step_dev is not None:
            step = int(step_dev[0]) + 1
        return ref.adam_update(p, g, m, v, shadow, lr, b1, b2, eps, weight_decay, decoupled,
                               1.0 / (1.0 - b1 ** step), 1.0 / (1.0 - b2 ** step))
    bc1 = 1.0 / (1.0 - b1 ** step)
    bc2 = 1.0 / (1.0 - b2 ** step)
    n = p.numel()
    if any(t.numel() != n for t in (g, m, v)):
        raise ValueError("adam buffers must have equal sizes")
    if step_dev is not None and step_dev.dtype != torch.int32:
        raise TypeError("step_dev must be int32")
    native().adam_update(_p(p), _p(g), _p(m), _p(v), _p(shadow), n, float(lr), float(b1),
                         float(b2), float(eps), float(weight_decay), int(decoupled), float(bc1),
                         float(bc2), _stream(p), lr_dev=_p(lr_dev), step_dev=_p(step_dev),
                         db1=float(b1), db2=float(b2))


def step_advance(step_dev):
    """step_dev += 1 on the device (after a device-step optimizer update)."""
    if not step_dev.is_cuda:
        step_dev += 1
        return
    native().step_advance(_p(step_dev), _stream(step_dev))


def pack_bf16(src, out):
    """fp32 [rows][cols] -> padded bf16 out [rows_p][cols_p] (zero padding)."""
    rows, cols = src.shape
    rows_p, cols_p = out.shape
    if not out.is_cuda:
        return ref.pack_bf16(src, out)
    if src.dtype != torch.float32 or out.dtype != torch.bfloat16:
        raise TypeError("pack_bf16: fp32 -> bf16")
    if src.stride(1) != 1 or out.stride(1) != 1:
        raise ValueError("pack_bf16 needs row-major tensors")
    native().pack_bf16(_p(src), src.stride(0), rows, cols, _p(out), out.stride(0), rows_p, cols_p,
                       _stream(out))


def bias_act_cast(x, bias, y, act="relu"):
    """y (bf16) = act(x (fp32) + bias): a row-parallel layer's epilogue after its all-reduce."""
    rows, cols = y.shape
    if not x.is_cuda:
        v = x[:rows, :cols] + (bias[:cols] if bias is not None else 0.0)
        y.copy_(ref.act_fwd(v, _act(act)).to(torch.bfloat16))
        return y
    _rows(x, "x", torch.float32)
    _rows(y, "y", torch.bfloat16)
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() < cols):
        raise ValueError("bias must be fp32 with >= cols entries")
    native().bias_act_cast(_p(x), x.stride(0), _p(bias), _act(act), _p(y), y.stride(0), rows,
                           cols, _stream(x))
    return y


def unpack_bf16(src, out):
    rows, cols = out.shape
    if not src.is_cuda:
        out.copy_(src[:rows, :cols].float())
        return
    native().unpack_bf16(_p(src), src.stride(0), rows, cols, _p(out), out.stride(0),
                         _stream(src))
