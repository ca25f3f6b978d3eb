"""PyTorch reference implementations with the kernels' numerics contract.

bf16 operands, fp32 accumulation, outputs rounded once to bf16 (or kept fp32). Used (a) as the
CPU execution path so the engine, pipeline schedules and DP logic run in CPU tests with gloo,
and (b) as the fp32 oracle for the GPU kernel tests.
"""
from __future__ import annotations

import torch

KMAJ, MNMAJ = 0, 1
_LINEAR, _RELU, _SIGMOID = 0, 1, 2


def act_fwd(v: torch.Tensor, act: int) -> torch.Tensor:
    if act == _RELU:
        return torch.clamp_min(v, 0.0)
    if act == _SIGMOID:
        return torch.sigmoid(v)
    return v


def act_bwd(g: torch.Tensor, y: torch.Tensor, act: int) -> torch.Tensor:
    if act == _RELU:
        return torch.where(y > 0, g, torch.zeros_like(g))
    if act == _SIGMOID:
        return g * y * (1.0 - y)
    return g


def _logical(a, b, layout_a, layout_b, M, N, Ktot):
    A = a[:M, :Ktot] if layout_a == KMAJ else a[:Ktot, :M].t()
    B = b[:N, :Ktot].t() if layout_b == KMAJ else b[:Ktot, :N]
    return A.float(), B.float()


def _colsum_blocks(vals, out, rows_per):
    nb = vals.shape[0] // rows_per
    out[:nb, :vals.shape[1]] = vals[:nb * rows_per].reshape(nb, rows_per, -1).sum(1)
    if vals.shape[0] % rows_per:  # partial edge tile: the kernels write its partial too
        out[nb, :vals.shape[1]] = vals[nb * rows_per:].sum(0)


def gemm(a, b, c, *, layout_a, layout_b, M, N, K, bias=None, aux=None, act=0, accumulate=False,
         splits=1, colsum=None, colsum_rows=0, k_total=0):
    ktot = k_total or K * splits
    A, B = _logical(a, b, layout_a, layout_b, M, N, ktot)
    out_f32 = c.dtype == torch.float32
    ks = ktot // 64
    for s in range(splits):
        if k_total:  # uneven split-K: same k-step ranges as the kernel
            k0, k1 = (s * ks // splits) * 64, ((s + 1) * ks // splits) * 64
        else:
            k0, k1 = s * K, (s + 1) * K
        acc = A[:, k0:k1] @ B[k0:k1, :]
        if bias is not None:
            acc = acc + bias[:N].float()
        if out_f32:
            dst = c[s] if c.dim() == 3 else c
            if accumulate:
                acc = acc + dst[:M, :N]
            else:
                acc = act_fwd(acc, act)
            dst[:M, :N] = acc
        else:
            if aux is not None:
                acc = act_bwd(acc, aux[:M, :N].float(), act)
            else:
                acc = act_fwd(acc, act)
            c[:M, :N] = acc.to(c.dtype)
            if colsum is not None:
                _colsum_blocks(c[:M, :N].float(), colsum, colsum_rows)
    return c


def e4m3_table() -> torch.Tensor:
    """fp64 value of each of the 256 OCP e4m3 codes, from the bit fields (1 sign, 4 exponent
    bits with bias 7, 3 mantissa bits, subnormals at exponent 0, 0x7F / 0xFF = NaN)."""
    c = torch.arange(256)
    s, e, m = c >> 7, (c >> 3) & 15, (c & 7).double()
    v = torch.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * torch.pow(2.0, (e - 7).double()))
    v = torch.where((e == 15) & (m == 7), torch.full_like(v, float("nan")), v)
    return torch.where(s == 1, -v, v)


_E4M3 = e4m3_table()


def gemv_fp8(x, q, scale, bias, y, M, N, K, act):
    """y[:M, :N] = act(fl32(scale * fl32(S)) + bias), S = x . dec(q)^T in fp64: the sum of the
    kernel without its summation error, then the kernel's fp32 epilogue."""
    S = x[:M, :K].double() @ _E4M3[q[:N, :K].long()].t()
    v = scale[:N].float() * S.float()
    if bias is not None:
        v = v + bias[:N].float()
    y[:M, :N] = act_fwd(v, act).to(y.dtype)
    return y


def e2m1_table() -> torch.Tensor:
    """fp64 value of each of the 16 e2m1 codes s|ee|m: exponent 0 is subnormal (0, 0.5), else
    (1 + m / 2) * 2^(ee - 1); bit 3 is the sign."""
    c = torch.arange(16)
    ee, m = (c >> 1) & 3, (c & 1).double()
    v = torch.where(ee == 0, m * 0.5, (1.0 + m * 0.5) * torch.pow(2.0, (ee - 1).double()))
    return torch.where(c >= 8, -v, v)


_E2M1 = e2m1_table()
MXFP4_TINY_EXP_FIELD = 17  # bf16 exponent field of 2^-110: blocks below it are zero blocks


def quant_rows_mxfp4(x, q, e):
    """The MXFP4 quantiser of csrc/kernels/mxfp4.hip on the bf16 bit fields and in fp64: E from
    the exponent field of the block's largest magnitude, t = |x| * 2^(127 - E) (exact), the
    code from the seven midpoints -- strict where the tie goes down to the even code, inclusive
    where it goes up."""
    rows, cols = x.shape
    nb = cols // 32
    bits = (x.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF).view(rows, nb, 32)
    ef = (bits & 0x7FFF).amax(2) >> 7
    send = ef >= MXFP4_TINY_EXP_FIELD
    E = torch.where(send, ef - 2, torch.zeros_like(ef))
    t = torch.ldexp(x.double().abs().view(rows, nb, 32), (127 - E)[:, :, None])
    code = ((t > 0.25).int() + (t >= 0.75).int() + (t > 1.25).int() + (t >= 1.75).int()
            + (t > 2.5).int() + (t >= 3.5).int() + (t > 5.0).int())
    code = torch.where(send[:, :, None], code | ((bits >> 12) & 8), torch.zeros_like(code))
    code = code.view(rows, cols)
    q[:rows, :cols // 2] = (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8)
    e[:rows, :nb] = E.to(torch.uint8)


def mxfp4_values(q, e, rows, cols) -> torch.Tensor:
    """fp64 [rows][cols]: dec(code) * 2^(E - 127), +0 for a block with E == 0."""
    b = q[:rows, :cols // 2].long()
    code = torch.stack([b & 15, b >> 4], dim=2).view(rows, cols)
    E = e[:rows, :cols // 32].long().repeat_interleave(32, dim=1)
    v = torch.ldexp(_E2M1[code], E - 127)
    return torch.where(E == 0, torch.zeros_like(v), v)


def dequant_rows_mxfp4(q, e, x):
    rows, cols = x.shape
    x.copy_(mxfp4_values(q, e, rows, cols).to(torch.bfloat16))  # exact for every E >= 15


def gemv_mxfp4(x, q, e, bias, y, M, N, K, act):
    """y[:M, :N] = act(fl32(S) + bias), S = x . (dec(q) * 2^(e - 127))^T in fp64: the sum of the
    kernel without its summation error, then the kernel's fp32 epilogue."""
    v = (x[:M, :K].double() @ mxfp4_values(q, e, N, K).t()).float()
    if bias is not None:
        v = v + bias[:N].float()
    y[:M, :N] = act_fwd(v, act).to(y.dtype)
    return y


def linear_w8a8(xq, sx, q, sw, bias, y, M, N, K, act):
    """y[:M, :N] = act(fl32(sx * fl32(sw * fl32(S))) + bias), S = dec(xq) . dec(q)^T in fp64: the
    sum of the kernel (csrc/kernels/linear_w8a8.hip) without its summation error, then the
    kernel's fp32 epilogue -- the weight scale first, the row scale second, each multiply
    rounded on its own."""
    S = _E4M3[xq[:M, :K].long()] @ _E4M3[q[:N, :K].long()].t()
    v = sx[:M].float()[:, None] * (sw[:N].float() * S.float())
    if bias is not None:
        v = v + bias[:N].float()
    y[:M, :N] = act_fwd(v, act).to(y.dtype)
    return y


def linear_w4a8(xq, sx, q, e, bias, y, M, N, K, act):
    """y[:M, :N] = act(fl32(sx * fl32(S)) + bias), S = dec(xq) . (dec(q) * 2^(e - 127))^T in
    fp64 with E == 0 blocks +0: the sum of the kernel (csrc/kernels/linear_w4a8.hip) without its
    summation error, then the kernel's fp32 epilogue -- the row scale one multiply rounded on
    its own."""
    S = _E4M3[xq[:M, :K].long()] @ mxfp4_values(q, e, N, K).t()
    v = sx[:M].float()[:, None] * S.float()
    if bias is not None:
        v = v + bias[:N].float()
    y[:M, :N] = act_fwd(v, act).to(y.dtype)
    return y


def softmax_xent(logits, labels, dz, n_cls, scale, loss_part=None, correct=None,
                 rows_per_block=64, colsum=None):
    rows, width = dz.shape
    lg = logits[:rows, :n_cls].float()
    lab = labels[:rows].long()
    valid = lab >= 0
    p = torch.softmax(lg, dim=1)
    g = p.clone()
    safe = lab.clamp_min(0)
    g[torch.arange(rows), safe] -= 1.0
    g = g * float(scale)
    g[~valid] = 0.0
    dz.zero_()
    dz[:, :n_cls] = g.to(dz.dtype)
    if loss_part is not None:
        logp = torch.log_softmax(lg, dim=1)
        nll = torch.where(valid, -logp[torch.arange(rows), safe], torch.zeros_like(lg[:, 0]))
        nb = -(-rows // rows_per_block)
        pad = torch.zeros(nb * rows_per_block)
        pad[:rows] = nll
        loss_part[:nb] = pad.view(nb, rows_per_block).sum(1).to(loss_part.dtype)
    if correct is not None:  # per-block partial counts (written, not accumulated)
        pred = torch.argmax(lg, dim=1)
        nb = -(-rows // rows_per_block)
        hit = torch.zeros(nb * rows_per_block, dtype=torch.int64)
        hit[:rows] = ((pred == lab) & valid).long()
        correct[:nb] = hit.view(nb, rows_per_block).sum(1).to(correct.dtype)
    if colsum is not None:
        nb = -(-rows // rows_per_block)
        pad = torch.zeros(nb * rows_per_block, width)
        pad[:rows] = dz.float()
        colsum[:nb, :width] = pad.view(nb, rows_per_block, width).sum(1)


def dense_loss(z, t, dz, n_out, scale, loss, act, row_ok=None, loss_part=None, colsum=None,
               rows_per_block=64, cols_per_chunk=256):
    """Dense-target losses (loss 1 = mse, 2 = bce on logits) with the kernel's contract and
    partial layout: fp32 arithmetic per element, dz rounded once to bf16, loss partials per
    (row block, column chunk), column sums of the stored dz per row block."""
    rows, width = dz.shape
    zz = z[:rows, :n_out].float()
    tt = t[:rows, :n_out].float()
    valid = torch.ones(rows, dtype=torch.bool) if row_ok is None else row_ok[:rows] >= 0
    zz = torch.where(valid[:, None], zz, torch.zeros_like(zz))  # padding rows may hold NaN
    tt = torch.where(valid[:, None], tt, torch.zeros_like(tt))
    coef = (2.0 if loss == 1 else 1.0) * float(scale) / n_out
    if loss == 2:
        y = torch.sigmoid(zz)
        term = torch.clamp_min(zz, 0.0) - tt * zz + torch.log1p(torch.exp(-zz.abs()))
        g = coef * (y - tt)
    else:
        y = act_fwd(zz, act)
        d = y - tt
        term = d * d
        if act == _SIGMOID:  # y (1 - y) from both tails: sigmoid(z) sigmoid(-z)
            g = coef * d * (y * torch.sigmoid(-zz))
        elif act == _RELU:
            g = torch.where(zz > 0, coef * d, torch.zeros_like(d))
        else:
            g = coef * d
    g = torch.where(valid[:, None], g, torch.zeros_like(g))
    term = torch.where(valid[:, None], term, torch.zeros_like(term))
    dz.zero_()
    dz[:, :n_out] = g.to(dz.dtype)
    nb = -(-rows // rows_per_block)
    nc = -(-width // cols_per_chunk)
    if loss_part is not None:
        pad = torch.zeros(nb * rows_per_block, nc * cols_per_chunk, dtype=torch.float64)
        pad[:rows, :n_out] = term.double()
        part = pad.view(nb, rows_per_block, nc, cols_per_chunk).sum((1, 3)) / n_out
        loss_part.view(-1)[:nb * nc] = part.reshape(-1).to(loss_part.dtype)
    if colsum is not None:
        pad = torch.zeros(nb * rows_per_block, width)
        pad[:rows] = dz.float()
        colsum[:nb, :width] = pad.view(nb, rows_per_block, width).sum(1)


def softmax_rows(logits, out, n_cls, labels=None, pred=None, correct=None):
    rows = logits.shape[0]
    lg = logits[:rows, :n_cls].float()
    if out is not None:
        out[:rows, :n_cls] = torch.softmax(lg, dim=1)
    am = torch.argmax(lg, dim=1)
    if pred is not None:
        pred[:rows] = am.to(pred.dtype)
    if correct is not None and labels is not None:
        correct += (am == labels[:rows].long()).sum().to(correct.dtype)


def colsum_partial(x, part, n_part):
    rows, cols = x.shape
    per = (rows + n_part - 1) // n_part
    xf = x.float()
    for i in range(n_part):
        part[i, :cols] = xf[i * per:min(rows, (i + 1) * per)].sum(0)


def reduce_slabs(src, n_src, stride, n, out, scale=1.0, accumulate=False):
    flat = src.reshape(-1)
    acc = flat[:n].clone()
    for s in range(1, n_src):
        acc += flat[s * stride:s * stride + n]
    acc *= scale
    o = out.reshape(-1)
    if accumulate:
        o[:n] += acc
    else:
        o[:n] = acc


def sgd_update(p, g, mom, shadow, lr, momentum, weight_decay):
    gv = g + weight_decay * p if weight_decay else g.clone()
    if momentum and mom is not None:
        mom.mul_(momentum).add_(gv)
        gv = mom
    p.sub_(lr * gv)
    if shadow is not None:
        shadow.copy_(p.to(shadow.dtype))


def adam_update(p, g, m, v, shadow, lr, b1, b2, eps, weight_decay, decoupled, bc1, bc2):
    gv = g.clone()
    if decoupled:
        p.mul_(1.0 - lr * weight_decay)
    elif weight_decay:
        gv += weight_decay * p
    m.mul_(b1).add_((1.0 - b1) * gv)
    v.mul_(b2).add_((1.0 - b2) * gv * gv)
    p.sub_(lr * (m * bc1) / (torch.sqrt(v * bc2) + eps))
    if shadow is not None:
        shadow.copy_(p.to(shadow.dtype))


def pack_bf16(src, out):
    rows, cols = src.shape
    out.zero_()
    out[:rows, :cols] = src.to(out.dtype)


TAIL_BLOCK_ROWS = 16  # rows per 16-row block; the mlp_tail grid is one workgroup per block,
# at most one per CU, blocks dealt round-robin


def tail_waves(act3: int, act2: int) -> int:
    """Waves per workgroup of csrc/kernels/mlp_tail.hip (16 rows each): 16 for ReLU/ReLU."""
    return 16 if act3 == _RELU and act2 == _RELU else 8


def mlp_tail(x, w3, b3, w4, b4, labels, h3, dz4, dz3, dz2, n_cls, scale, act3, act2,
             loss_part, correct, cs4, cs3, cs2, n_blocks):
    """Unfused reference of the fused classifier tail. Partials follow the kernel's row
    assignment: 16-row block rb belongs to workgroup rb % n_blocks."""
    rows, k3 = x.shape
    n3, n4 = w3.shape[0], w4.shape[0]
    gemm(x, w3, h3, layout_a=KMAJ, layout_b=KMAJ, M=rows, N=n3, K=k3, bias=b3, act=act3)
    logits = torch.zeros(rows, n4, dtype=torch.float32)
    gemm(h3, w4, logits, layout_a=KMAJ, layout_b=KMAJ, M=rows, N=n4, K=n3, bias=b4, act=0)
    lg = logits[:, :n_cls]
    lab = labels[:rows].long()
    valid = lab >= 0
    safe = lab.clamp_min(0)
    per_row_loss = torch.where(valid, -torch.log_softmax(lg, 1)[torch.arange(rows), safe],
                               torch.zeros(rows))
    hit = ((torch.argmax(lg, 1) == lab) & valid).long()
    softmax_xent(logits, labels, dz4, n_cls, scale)
    gemm(dz4, w4, dz3, layout_a=KMAJ, layout_b=MNMAJ, M=rows, N=n3, K=n4, aux=h3, act=act3)
    gemm(dz3, w3, dz2, layout_a=KMAJ, layout_b=MNMAJ, M=rows, N=k3, K=n3, aux=x, act=act2)
    owner = (torch.arange(rows) // 16) % n_blocks
    for t, src, cols in ((cs4, dz4, n4), (cs3, dz3, n3), (cs2, dz2, k3)):
        part = torch.zeros(n_blocks, cols)
        part.index_add_(0, owner, src[:rows, :cols].float())
        t[:n_blocks, :cols] = part
    loss_part[:n_blocks] = 0.0
    loss_part.index_add_(0, owner, per_row_loss.to(loss_part.dtype))
    correct[:n_blocks] = 0
    correct.index_add_(0, owner, hit.to(correct.dtype))
