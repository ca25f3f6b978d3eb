"""Stage-by-stage audit of one whole training step against fp64 oracles.

A Stage keeps everything a step produced (inputs, activations, dZ, masks, transposed copies,
gradients, masters, shadows, optimizer state, loss partials). ``collect`` copies all of it to the
CPU after a step, ``snapshot`` copies the parameters and optimizer state before it, and ``audit``
checks every stored quantity against the fp64 function of the engine's OWN stored operands that
feed it -- so an error never compounds from one stage of the step to the next, and each check runs
at the tolerance of the kernel oracle that already pins that kernel in isolation. ``audit`` works
on dicts of CPU tensors only: a test can corrupt a copy and see the named check reject it.

Checks (``stats[kind]`` keeps the worst error / bound of each; for the bitwise ones, M, T and
H, the number of comparisons that passed):

  F  acts[i] = act(input_of(i) @ wbf_i^T + b_i) with the PRE-update shadow and bias. bf16 outputs:
     2 bf16 ulps of the fp64 value + floor; fp32 logits: floor only. floor = 4 x the largest
     |fp32 - fp64| of the CPU reference arithmetic (ops/reference.py) on the same operands: the
     fp32 accumulation error scales with the sum of |terms|, not with the result. Padding columns
     must be exactly 0 (see "padding" below).
  M  relu_mask[i] (byte form or FragMask, unpacked by collect) == acts[i] > 0, bitwise, for the
     layers whose forward is a GEMM of the stage. Under DNN_RELU_MASK=1 a stage with the tail head
     also allocates the mask of layer L-2, whose forward and consumer both run inside the tail
     kernel: that kernel neither writes nor reads it, and no check looks at it.
  T  actT[i], dzT[i] and the W^T shadows (before and after the update) are bitwise transposes of
     acts[i], dz[i] and wbf_i.
  H  stage hops: the next stage's x_in == the previous stage's acts[-1], the previous stage's
     dz[-1] == the next stage's dx_send, bitwise; under the fp8 boundary (q / scale stored by
     collect) the received rows are dequant(quant(sent rows)) of tests/_fp8_oracle.py, bitwise.
  L  last stage: dz[L-1], loss_part, correct and Trainer.loss() (at the sum of the partials'
     bounds) against _loss_oracle.xent_ref
     (_wide_softmax_oracle's tight bounds beyond 256 padded columns) or _dense_loss_oracle, with
     scale = 1 / global_batch. Rows labelled -1 have dz exactly 0 and add nothing.
  B  dz[i-1] = act'(acts[i-1]) * (dz[i] @ wbf_i), and dx_send on non-first stages, as F.
  G  gb(i) = column sums of the stored dz[i] over all rows: rows * 2^-24 * sum|dz| per column;
     padding entries exactly 0.
  W  gw(i) = dz[i]^T @ input_of(i) over all micro-batches: (R + S) * 2^-24 * |dz|^T |x|
     (tests/_wgrad_oracle.py random_bound; S = partial sums added: the split count, x micro-batches
     for per-micro-batch accumulation, the workgroup count for stream-K). Padded rows and columns
     exactly 0.
  O  masters, momentum / m / v and the bf16 shadow against _opt_oracle.check_sgd / check_adam
     from the snapshot and the engine's own stored gradient; shadow == RN_bf16(master) bitwise;
     step counters and the device learning rate. The padding-unit biases of a sigmoid layer (see
     "padding" below) are pinned, not updated: they equal PAD_OFF_BIAS bitwise before and after
     the update, whatever the weight decay; their optimizer state is not checked.

Quantities a path never stores, and what is checked instead:

  * FusedXentHead and TailHead never store the logits. L recomputes them in fp64 from the stored
    input of the last layer; their own error d (the F floor of that product) moves the softmax by
    at most 2 d, so the dz bound is widened by |scale| * 2 d, a row's loss by 2 d (log-sum-exp and
    the label's logit are both 1-Lipschitz in max|dz|), and a row whose two largest logits lie
    within 2 d of each other may count as correct either way.
  * TailHead computes the forward of layer L-2 and the dgrads of layers L-1 and L-2 inside its
    kernel, but stores acts[L-2], dz[L-2] and dz[L-3]: F and B check them like any other layer.
  * A layer that updates in its wgrad epilogue (Stage.enable_fused_wgrad_update) does not store
    its weight gradient: W is skipped for it and O checks its weights (and momentum) from the
    fp64 gradient, with the W bound (times the factor the gradient enters with) added to the
    optimizer bound.
  * Padding. Padding columns of every activation and every dZ, padded rows / columns of every
    weight gradient and padding entries of every bias gradient must be exactly 0: only then do
    the padded weights stay 0 and the padded model equal the specified one. A sigmoid layer whose
    width is not a multiple of 64 keeps its padding units off through their bias
    (engine/params.py PAD_OFF_BIAS), so its padding columns are sigmoid(-huge) = 0, not sigmoid(0).

No tolerance here is tuned: each is a bound derived in an existing oracle module, or a floor
measured from the fp32 reference arithmetic on the same operands.
"""
from __future__ import annotations

import torch

import _act_oracle as ao
import _dense_loss_oracle as dlo
import _loss_oracle as lo
import _opt_oracle as oo
import _wide_softmax_oracle as ws

CPU = torch.device("cpu")
U = 2.0 ** -24
KINDS = ("F", "M", "T", "H", "L", "B", "G", "W", "O")
EXACT = ("M", "T", "H")  # bitwise checks: stats count the comparisons that passed


def new_stats() -> dict:
    """Worst error / bound per kind of check (count of passed comparisons for the bitwise
    kinds), and under "checks" the number of comparisons of every kind that ran."""
    return {**{k: 0 if k in EXACT else 0.0 for k in KINDS}, "checks": {k: 0 for k in KINDS}}


def statline(name: str, stats: dict) -> str:
    return "STEPSTAT " + name + " worst/bound " + " ".join(
        f"{k} {stats[k]:.3f}" for k in KINDS if k not in EXACT) + " bitwise checks " + " ".join(
        f"{k} {stats[k]}" for k in EXACT)


# ---- the two GEMM oracles: fp64 value and floor ----------------------------------------------

def _mm(a, b, dtype, dev):
    """a @ b in ``dtype`` (torch's own matmul) on ``dev``."""
    return a.to(dev, dtype) @ b.to(dev, dtype)


def fwd64(x, w, b, act, dev=CPU):
    """(fp64 value, floor) of act(x @ w^T + b): the floor is 4 x the largest |fp32 - fp64| of
    the reference arithmetic (ops/reference.py) on the same operands."""
    from docker_dist_nn_amd.models.mlp import ACT_CODE
    from docker_dist_nn_amd.ops import reference as ref

    want = ao.act_fwd(_mm(x, w.t(), torch.float64, dev) + b.to(dev).double(), act)
    f32 = ref.act_fwd(_mm(x, w.t(), torch.float32, dev) + b.to(dev).float(), ACT_CODE[act])
    return want, 4.0 * float((f32.double() - want).abs().max())


def dgrad64(dz, w, y, act, dev=CPU):
    """(fp64 value, floor) of (dz @ w) * act'(y), the floor as in fwd64."""
    from docker_dist_nn_amd.models.mlp import ACT_CODE
    from docker_dist_nn_amd.ops import reference as ref

    want = ao.act_bwd(_mm(dz, w, torch.float64, dev), y.to(dev), act)
    f32 = ref.act_bwd(_mm(dz, w, torch.float32, dev), y.to(dev).float(), ACT_CODE[act])
    return want, 4.0 * float((f32.double() - want).abs().max())


def assert_dgrad_fp64(name, got, dz, w, y, act):
    """A dgrad output against fp64 evaluated from the kernel's OWN stored inputs: 2 bf16 ulps
    (the single rounding of the result, and slack for a rounding boundary) plus an absolute
    floor for the fp32 accumulation, whose error scales with the sum of |terms|, not with the
    result: 4 x the largest |fp32 - fp64| of the CPU reference path (ops/reference.py) on the
    same inputs. Returns the floor. (Also used by tests/test_mlp_tail_gpu.py; check B of the
    audit applies the same value and bound.)"""
    dz, w, y, got = (t.detach().cpu() for t in (dz, w, y, got))
    want, floor = dgrad64(dz, w, y, act)
    excess = (got.double() - want).abs() - (2.0 * ao.bf16_ulp(want) + floor)
    assert not torch.isnan(got.float()).any()
    assert float(excess.max()) <= 0.0, (name, act, float(excess.max()), floor)
    return floor


# ---- collect / snapshot ----------------------------------------------------------------------

def _c(t):
    return None if t is None else t.detach().to(CPU).clone()


def _params(st) -> dict:
    p = st.params
    n = len(st.geoms)
    opt = p.opt
    return dict(master=_c(p.master), shadow=_c(p.shadow), state=[_c(s) for s in p.state],
                w32=[_c(p.w32(i)) for i in range(n)], b32=[_c(p.b32(i)) for i in range(n)],
                wbf=[_c(p.wbf(i)) for i in range(n)], wt={i: _c(t) for i, t in p.wt.items()},
                step_count=opt.step_count,
                step_dev=None if opt.step_dev is None else int(opt.step_dev.item()),
                lr_dev=None if opt.lr_dev is None else float(opt.lr_dev.item()))


def snapshot(trainer) -> dict:
    """Before a step: masters, biases, bf16 shadows, W^T shadows, optimizer state, step count
    and the learning rate the step is to run at (the optimizer configuration's)."""
    return dict(stages=[_params(st) for st in trainer.stages], lr=float(trainer.optim.lr))


def _mask_bits(st, i):
    from docker_dist_nn_amd import ops

    m = st.relu_mask[i]
    if m is None:
        return None
    if isinstance(m, ops.FragMask):
        return _c(m.bits())
    return _c(ops.relu_mask_bits(m, st.rows, st.geoms[i].np_))


def collect(trainer) -> dict:
    """After ``trainer.flush()`` and a device synchronize: every per-stage tensor of the step on
    the CPU, and what the engine chose (head, masks, transposed copies, splits, fused layers)."""
    from docker_dist_nn_amd import ops

    out = dict(stages=[], loss=trainer.loss(), correct=trainer.correct(),
               rows=trainer.micro_batch * trainer.num_micro, lr=float(trainer.optim.lr),
               device=trainer.device.type)
    for st in trainer.stages:
        L = len(st.geoms)
        acts = list(st.acts)
        if getattr(st, "h0_double", False) and st._h0_flip == 1:
            acts[0] = st._h0_alt  # the layer-0 buffer the audited step wrote
        head = st.head
        p = st.params
        d = _params(st)
        d.update(
            geoms=[dict(np_=g.np_, kp=g.kp, out_dim=g.spec.out_dim, in_dim=g.spec.in_dim,
                        act=g.spec.activation) for g in st.geoms],
            mb=st.mb, nm=st.nm, rows=st.rows, first=st.first, last=st.last,
            prev_act=st.prev_act, n_cls=st.n_cls, global_batch=st.global_batch, loss=st.loss,
            head=type(head).__name__ if head else None, fwd_from=st.fwd_from,
            dgrad_from=st.dgrad_from, w_splits=list(st.w_splits), wgrad_algo=st.wgrad_algo,
            wgrad_mode=st.wgrad_mode, fused_layers=sorted(p.fused_layers),
            mask_kind=[None if m is None else type(m).__name__ for m in st.relu_mask],
            x_in=_c(st.x_in), acts=[_c(a) for a in acts], dz=[_c(t) for t in st.dz],
            dx_send=_c(st.dx_send), mask_bits=[_mask_bits(st, i) for i in range(L)],
            actT={i: _c(t) for i, t in st.actT.items()},
            dzT={i: _c(t) for i, t in st.dzT.items()},
            bpart=[_c(t) for t in st.bpart], slabs=[_c(t) for t in st.slabs],
            grad=_c(p.grad), gw=[_c(p.gw(i)).view(g.np_, g.kp) for i, g in enumerate(st.geoms)],
            gb=[_c(p.gb(i)) for i in range(L)], w_off=list(p.w_off), b_off=list(p.b_off),
            fp8={k: _c(getattr(st, k)) for k in ("q_out", "s_out", "q_gin", "s_gin", "q_in",
                                                 "s_in", "q_dx", "s_dx") if hasattr(st, k)},
            streamk_wg=ops.STREAMK_WG)
        if head is not None:
            d.update(labels=_c(head.labels.cur), loss_part=_c(head.loss_part),
                     correct=_c(head.correct), blocks=head.blocks, chunks=head.chunks,
                     logits_stored=bool(head.logits),
                     targets=_c(head.targets.cur) if head.targets is not None else None)
            if d["head"] == "FusedXentHead":
                d["rows_per_part"] = st.mb // head.blocks
        out["stages"].append(d)
    return out


# ---- comparators -----------------------------------------------------------------------------

class _Ctx:
    def __init__(self, stats, dev):
        self.stats = stats if stats is not None else new_stats()
        self.dev = dev  # where the oracles' matrix products and comparisons run

    def fail(self, kind, s, i, msg):
        where = f"stage {s}" + ("" if i is None else f" layer {i}")
        raise AssertionError(f"[{kind}] {where}: {msg}")

    def close(self, kind, s, i, what, got, want, bound):
        got, want = got.to(self.dev).double(), want.to(self.dev)
        if bool(torch.isnan(got).any()):
            self.fail(kind, s, i, f"{what}: NaN at {torch.isnan(got).nonzero()[:4].tolist()}")
        err = (got - want).abs()
        bound = torch.as_tensor(bound, dtype=torch.float64).to(self.dev).expand_as(err)
        ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
        self.stats[kind] = max(self.stats[kind], ratio)
        self.stats["checks"][kind] += 1
        bad = err > bound
        if bool(bad.any()):
            self.fail(kind, s, i, f"{what} off by {ratio:.3g} x the bound at "
                                  f"{bad.nonzero()[:4].tolist()}")

    def exact(self, kind, s, i, what, got, want):
        if got.shape != want.shape:
            self.fail(kind, s, i, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}")
        if got.dtype == torch.bfloat16:  # bit for bit, not value for value
            got, want = got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)
        bad = got != want
        if bool(bad.any()):
            self.fail(kind, s, i, f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, "
                                  f"first at {bad.nonzero()[:4].tolist()}")
        self.stats["checks"][kind] += 1
        if kind in EXACT:
            self.stats[kind] += 1

    def zero(self, kind, s, i, what, t):
        bad = t != 0
        if bool(bad.any()):
            self.fail(kind, s, i, f"{what} not exactly 0 at {bad.nonzero()[:4].tolist()}")

    def wrapped(self, kind, s, i, fn, *a, **kw):
        self.stats["checks"][kind] += 1
        try:
            return fn(*a, **kw)
        except AssertionError as e:
            self.fail(kind, s, i, str(e))


def _input(d, i):
    return d["x_in"] if i == 0 else d["acts"][i - 1]


def _check_forward(cx, s, d, b4):
    L = len(d["geoms"])
    for i, g in enumerate(d["geoms"]):
        y = d["acts"][i]
        if y.numel() == 0:
            continue  # logits never in memory: L recomputes them
        head_out = d["head"] is not None and i == L - 1
        act = "linear" if head_out else g["act"]
        want, floor = fwd64(_input(d, i), b4["wbf"][i], b4["b32"][i], act, cx.dev)
        if y.dtype == torch.float32:
            cx.close("F", s, i, "logits", y, want, floor)
        else:
            cx.close("F", s, i, "acts", y, want, 2.0 * ao.bf16_ulp(want) + floor)
        if not (head_out and d["loss"] != "softmax_ce" and g["act"] == "sigmoid"):
            cx.zero("F", s, i, "padding columns of acts", y[:, g["out_dim"]:])


def _check_masks(cx, s, d):
    for i, bits in enumerate(d["mask_bits"]):
        if bits is not None and i < d["fwd_from"]:  # written by the stage's own forward GEMM
            cx.exact("M", s, i, "relu mask", bits, d["acts"][i] > 0)


def _check_transposes(cx, s, d, b4):
    for i, t in d["actT"].items():
        cx.exact("T", s, i, "actT", t, d["acts"][i].t())
    for i, t in d["dzT"].items():
        cx.exact("T", s, i, "dzT", t, d["dz"][i].t())
    for i, t in b4["wt"].items():
        cx.exact("T", s, i, "W^T before the update", t, b4["wbf"][i].t())
    for i, t in d["wt"].items():
        cx.exact("T", s, i, "W^T after the update", t, d["wbf"][i].t())


def _fp8_round_trip(x):
    import _fp8_oracle as fo

    q, sc, _ = fo.quant_ref(x)
    return q, sc, fo.dequant_ref(q, sc)


def _check_hops(cx, after):
    st = after["stages"]
    for s in range(len(st) - 1):
        a, b = st[s], st[s + 1]
        if a["fp8"] or b["fp8"]:
            import numpy as np

            for kind, src, dst, qk, sk in (("activation", a["acts"][-1], b["x_in"], "q_in", "s_in"),
                                           ("gradient", b["dx_send"], a["dz"][-1], "q_gin",
                                            "s_gin")):
                q, sc, y = _fp8_round_trip(src)
                owner = b if kind == "activation" else a
                cx.exact("H", s, None, f"fp8 {kind} codes", owner["fp8"][qk],
                         torch.from_numpy(np.asarray(q)).view(torch.uint8).reshape(src.shape))
                cx.exact("H", s, None, f"fp8 {kind} scales", owner["fp8"][sk],
                         torch.from_numpy(np.asarray(sc, dtype=np.float32)).reshape(-1))
                cx.exact("H", s, None, f"fp8 {kind} hop", dst, y.to(torch.bfloat16))
        else:
            cx.exact("H", s, None, "activation hop", b["x_in"], a["acts"][-1])
            cx.exact("H", s, None, "gradient hop", a["dz"][-1], b["dx_send"])


def _owners(d):
    """Loss / correct partial of every row, and the partial count."""
    R, mb = d["rows"], d["mb"]
    r = torch.arange(R)
    j, rr = r // mb, r % mb
    if d["head"] == "TailHead":  # 16-row blocks dealt round-robin over the workgroups
        own = j * d["blocks"] + (rr // 16) % d["blocks"]
    elif d["head"] == "FusedXentHead":
        own = j * d["blocks"] + rr // d["rows_per_part"]
    else:
        own = r // lo.XENT_BLOCK_ROWS
    return own, d["blocks"] * d["nm"]


def _check_loss(cx, s, d, b4, after):
    L = len(d["geoms"])
    i = L - 1
    g = d["geoms"][i]
    n_cls, scale = d["n_cls"], 1.0 / d["global_batch"]
    labels, dz = d["labels"], d["dz"][i]
    R = d["rows"]
    pad_rows = labels[:R] < 0
    cx.zero("L", s, i, "dz of rows labelled -1", dz[pad_rows])
    if d["loss"] != "softmax_ce":
        z = d["acts"][i]
        case = dict(rows=R, n_out=n_cls, z=z[:, :n_cls].double(),
                    t=d["targets"][:, :n_cls].double(), ok=labels[:R])
        ref = dlo.dense_ref(case, d["loss"], g["act"], scale, True)
        st = dlo.new_stats()
        cx.wrapped("L", s, i, dlo.assert_dz, dz, ref, g["np_"], st, "dense dz")
        cx.wrapped("L", s, i, dlo.assert_loss_partials, d["loss_part"], ref, R, g["np_"], st,
                   "dense loss")
        cx.stats["L"] = max(cx.stats["L"], st["dz"], st["loss"])
        want_loss = float(ref["term"].sum())
        total_bound = 76 * U * want_loss + float(ref["valid"].sum()) * n_cls * ref["C"] * U / n_cls
    else:
        wide = g["np_"] > 256
        depth = None if after["device"] == "cuda" else n_cls - 1
        if d["logits_stored"]:
            z64, delta = d["acts"][i][:, :n_cls].double(), 0.0
        else:
            want, floor = fwd64(_input(d, i), b4["wbf"][i], b4["b32"][i], "linear", cx.dev)
            z64, delta = want[:, :n_cls].to(CPU), floor
        ref = lo.xent_ref(z64, labels, scale)
        terms = ws.p_terms(n_cls, depth) if wide else n_cls + 8
        bound = ao.bf16_ulp(ref["dz"]) + abs(scale) * terms * U + abs(scale) * 2.0 * delta
        cx.close("L", s, i, "dz", dz[:, :n_cls], ref["dz"], bound)
        cx.zero("L", s, i, "padding columns of dz", dz[:, n_cls:])
        own, n_part = _owners(d)
        got = d["loss_part"].double()[:n_part]
        want = torch.zeros(n_part, dtype=torch.float64).index_add_(0, own, ref["loss"])
        nval = torch.zeros(n_part, dtype=torch.float64).index_add_(0, own, ref["valid"].double())
        if wide:
            lb = 18 * U * want + nval * ws.loss_terms(n_cls, depth) * U
        else:
            lb = 2.0 ** -18 * want + nval * (n_cls + 8) * U
        lb = lb + nval * 2.0 * delta
        cx.zero("L", s, i, "loss partial of an all-padding block", got[nval == 0])
        if bool((nval > 0).any()):
            cx.close("L", s, i, "loss partial", got[nval > 0], want[nval > 0], lb[nval > 0])
        # correct counts: exact, except rows whose two largest logits the recomputation cannot
        # tell apart (never with stored logits: delta = 0)
        top = torch.topk(z64, min(2, n_cls), dim=1).values
        amb = ref["valid"] & ((top[:, 0] - top[:, -1]) <= 2.0 * delta) if n_cls > 1 and delta \
            else torch.zeros(R, dtype=torch.bool)
        wc = torch.zeros(n_part, dtype=torch.float64).index_add_(
            0, own, (ref["correct"] & ~amb).double())
        slack = torch.zeros(n_part, dtype=torch.float64).index_add_(0, own, amb.double())
        gc = d["correct"].double()[:n_part]
        bad = (gc < wc) | (gc > wc + slack)
        if bool(bad.any()):
            cx.fail("L", s, i, f"correct counts {gc.tolist()[:8]} != {wc.tolist()[:8]} at "
                               f"{bad.nonzero()[:4].tolist()}")
        want_loss, total_bound = float(ref["loss"].sum()), float(lb.sum())
    # Trainer.loss(): the mean over the step's rows of the oracle's row losses, at the sum of
    # the partials' bounds (its own sum of the partials is a fixed-order fp64 sum)
    if after["loss"] is None:
        cx.fail("L", s, None, "Trainer.loss() is None on the last stage")
    cx.close("L", s, None, "Trainer.loss() x rows", torch.tensor([after["loss"] * after["rows"]]),
             torch.tensor([want_loss], dtype=torch.float64),
             total_bound + 1e-12 * max(1.0, want_loss))


def _check_backward(cx, s, d, b4):
    L = len(d["geoms"])
    for i in range(L - 1, -1, -1):
        if i == 0 and d["first"]:
            break
        got = d["dz"][i - 1] if i > 0 else d["dx_send"]
        y = d["acts"][i - 1] if i > 0 else d["x_in"]
        act = d["geoms"][i - 1]["act"] if i > 0 else d["prev_act"]
        act = "linear" if act == "softmax" else act
        want, floor = dgrad64(d["dz"][i], b4["wbf"][i], y, act, cx.dev)
        what = "dz" if i > 0 else "dx_send"
        cx.close("B", s, i - 1 if i > 0 else None, what, got, want,
                 2.0 * ao.bf16_ulp(want) + floor)
        cx.zero("B", s, i - 1 if i > 0 else None, f"padding columns of {what}",
                got[:, d["geoms"][i]["in_dim"]:])


def _wgrad64(cx, d, i):
    dz, x = d["dz"][i], _input(d, i)
    S = d["w_splits"][i] * (d["nm"] if d["wgrad_mode"] != "batched" else 1)
    if d["wgrad_algo"] == "streamk":
        S = d["streamk_wg"] * (d["nm"] if d["wgrad_mode"] != "batched" else 1)
    f64 = torch.float64
    return _mm(dz.t(), x, f64, cx.dev), \
        (d["rows"] + S) * U * _mm(dz.abs().t(), x.abs(), f64, cx.dev)


def _check_grads(cx, s, d):
    for i, g in enumerate(d["geoms"]):
        dz = d["dz"][i].double()
        cx.close("G", s, i, "gb", d["gb"][i], dz.sum(0), d["rows"] * U * dz.abs().sum(0))
        cx.zero("G", s, i, "padding entries of gb", d["gb"][i][g["out_dim"]:])
        if i in d["fused_layers"] and d["device"] == "cuda":
            continue  # updated in the wgrad epilogue: the gradient is never stored (see O)
        want, bound = _wgrad64(cx, d, i)
        cx.close("W", s, i, "gw", d["gw"][i], want, bound)
        cx.zero("W", s, i, "padded rows of gw", d["gw"][i][g["out_dim"]:])
        cx.zero("W", s, i, "padded columns of gw", d["gw"][i][:, g["in_dim"]:])


def _check_update(cx, s, d, b4, cfg, lr):
    name = cfg.name
    sgd = name == "sgd"
    if d["step_count"] != b4["step_count"] + 1:
        cx.fail("O", s, None, f"step count {b4['step_count']} -> {d['step_count']}")
    if d["step_dev"] is not None and not sgd and d["step_dev"] != d["step_count"]:
        cx.fail("O", s, None, f"device step counter {d['step_dev']} != {d['step_count']}")
    if d["lr_dev"] is not None and d["lr_dev"] != oo.f32(lr):
        cx.fail("O", s, None, f"device learning rate {d['lr_dev']} != {lr}")
    fused = d["fused_layers"] if d["device"] == "cuda" else []
    keep = torch.ones(d["master"].numel(), dtype=torch.bool)
    for i in fused:
        g = d["geoms"][i]
        keep[d["w_off"][i]:d["w_off"][i] + g["np_"] * g["kp"]] = False
    # padding-unit biases of sigmoid layers are pinned after every update, not updated
    from docker_dist_nn_amd.engine.params import PAD_OFF_BIAS

    for i, g in enumerate(d["geoms"]):
        if g["act"] == "sigmoid" and g["np_"] > g["out_dim"]:
            lo_, hi_ = d["b_off"][i] + g["out_dim"], d["b_off"][i] + g["np_"]
            keep[lo_:hi_] = False
            pin = torch.full((hi_ - lo_,), PAD_OFF_BIAS)
            for what, t in (("before", b4["master"]), ("after", d["master"])):
                cx.exact("O", s, i, f"padding-unit biases {what} the update", t[lo_:hi_], pin)
            cx.exact("O", s, i, "bf16 shadow of the padding-unit biases", d["shadow"][lo_:hi_],
                     pin.to(torch.bfloat16))
    st = oo.new_stats()
    sel = lambda t: t[keep]  # noqa: E731
    if sgd:
        mom = bool(cfg.momentum)
        old = dict(p=sel(b4["master"]), mom=sel(b4["state"][0]) if mom else None)
        got = dict(p=sel(d["master"]), mom=sel(d["state"][0]) if mom else None,
                   shadow=sel(d["shadow"]))
        cx.wrapped("O", s, None, oo.check_sgd, old, sel(d["grad"]), got, lr=lr,
                   momentum=cfg.momentum, weight_decay=cfg.weight_decay, stats=st, what="sgd")
    else:
        old = dict(p=sel(b4["master"]), m=sel(b4["state"][0]), v=sel(b4["state"][1]))
        got = dict(p=sel(d["master"]), m=sel(d["state"][0]), v=sel(d["state"][1]),
                   shadow=sel(d["shadow"]))
        cx.wrapped("O", s, None, oo.check_adam, old, sel(d["grad"]), got, lr=lr,
                   betas=cfg.betas, eps=cfg.eps, weight_decay=cfg.weight_decay,
                   decoupled=cfg.decoupled or name == "adamw", t=b4["step_count"] + 1, stats=st,
                   what=name)
    worst = max(st[k] for k in ("p", "mom", "m", "v"))
    if not sgd and st["p_cpu"] > 0.25:  # check_adam's own slack: 4 x the CPU path's ratio
        worst = max(max(st[k] for k in ("mom", "m", "v")), st["p"] / max(1.0, 4.0 * st["p_cpu"]))
    cx.stats["O"] = max(cx.stats["O"], worst)
    for i in fused:  # SGD only (Stage.enable_fused_wgrad_update): from the fp64 gradient
        g64, gbound = (t.to(CPU) for t in _wgrad64(cx, d, i))
        mu, wd = float(cfg.momentum), float(cfg.weight_decay)
        p0 = b4["w32"][i].double()
        l2 = wd * p0
        if mu:
            off, n = d["w_off"][i], p0.numel()
            m0 = b4["state"][0][off:off + n].view_as(p0).double()
            m1 = d["state"][0][off:off + n].view_as(p0)
            cx.close("O", s, i, "momentum (fused update)", m1, mu * m0 + g64 + l2,
                     oo.U22 * ((mu * m0).abs() + g64.abs() + l2.abs()) + gbound)
            upd, ub = m1.double(), 0.0
        else:
            upd, ub = g64 + l2, lr * gbound
        cx.close("O", s, i, "master (fused update)", d["w32"][i], p0 - lr * upd,
                 oo.U22 * (p0.abs() + (lr * upd).abs()) + ub)
        cx.exact("O", s, i, "bf16 shadow (fused update)", d["wbf"][i],
                 d["w32"][i].to(torch.bfloat16))


# ---- the audit -------------------------------------------------------------------------------

def audit(before: dict, after: dict, cfg, stats: dict | None = None, oracle_device=None) -> None:
    """Check every stored quantity of the step between ``before`` (snapshot) and ``after``
    (collect) against its fp64 oracle; ``cfg`` is the step's OptimConfig, whose ``lr`` the
    snapshot recorded. Raises an AssertionError naming the check, stage, layer and the first
    offending indices; keeps the worst error / bound of each kind of check in ``stats``.
    ``oracle_device``: run the oracles' matrix products (torch.matmul in fp64 / fp32, nothing of
    this project) there instead of on the CPU -- for the few cases of tens of thousands of rows."""
    cx = _Ctx(stats, CPU if oracle_device is None else oracle_device)
    lr = before["lr"]
    _check_hops(cx, after)
    for s, (d, b4) in enumerate(zip(after["stages"], before["stages"])):
        d["device"] = after["device"]
        _check_forward(cx, s, d, b4)
        _check_masks(cx, s, d)
        _check_transposes(cx, s, d, b4)
        if d["head"] is not None:
            _check_loss(cx, s, d, b4, after)
        _check_backward(cx, s, d, b4)
        _check_grads(cx, s, d)
        _check_update(cx, s, d, b4, cfg, lr)


# ---- models and batches of the audit tests ---------------------------------------------------

def spec_of(widths, acts):
    from docker_dist_nn_amd import MLPSpec
    from docker_dist_nn_amd.models.mlp import LayerSpec

    n = len(acts)
    return MLPSpec(tuple(LayerSpec(widths[i], widths[i + 1], acts[i],
                                   "output" if i == n - 1 else "hidden") for i in range(n)),
                   "-".join(map(str, widths)))


def batch(rows, mb, in_dim, kp, out_dim, seed, dense):
    """Inputs, labels and (dense losses) targets. Labels are -1 on scattered rows, on the whole
    second 64-row block and on the entire last half of the last micro-batch."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(rows, kp, dtype=torch.bfloat16)
    x[:, :in_dim] = torch.randn(rows, in_dim, generator=g).to(torch.bfloat16)
    y = torch.randint(0, out_dim, (rows,), generator=g, dtype=torch.int32)
    y[3::7] = -1
    y[64:128] = -1
    y[rows - mb // 2:] = -1
    t = None
    if dense:
        y = torch.where(y < 0, y, torch.zeros_like(y))
        t = (torch.randint(0, 9, (rows, out_dim), generator=g).float() / 8).to(torch.bfloat16)
    return x, y, t


class Fp8Pair:
    """Two pipeline stages in one process joined by the fp8 hop format: per stage exactly what a
    rank of a two-rank Trainer(boundary="fp8") job runs (Stage.pack_* / unpack_* around its
    forward and backward), with the transport replaced by plain copies of the codes and scales
    (a single-process Trainer has no hop to compress and refuses the fp8 boundary). Offers what
    snapshot / collect read off a Trainer."""

    def __init__(self, spec, split, *, micro_batch, num_micro, optim, device, native=False):
        from docker_dist_nn_amd.engine.stage import Stage

        L = len(spec.layers)
        self.stages = [Stage(spec, a, b, micro_batch=micro_batch, num_micro=num_micro,
                             device=device, global_batch=micro_batch * num_micro, optim=optim,
                             stage_index=k, num_stages=2)
                       for k, (a, b) in enumerate(((0, split), (split, L)))]
        for st in self.stages:
            st.params.init_default(0)
        self.stages[0].enable_fp8_boundary(False, True)
        self.stages[1].enable_fp8_boundary(True, False)
        if native:
            for st in self.stages:
                st.compile_native()
        self.optim, self.device = optim, device
        self.micro_batch, self.num_micro = micro_batch, num_micro

    def set_batch(self, x, labels, targets=None):
        self.stages[0].set_batch(x, None)
        self.stages[1].head.set_batch(labels, targets)

    def step(self):
        a, b = self.stages
        for st in self.stages:
            st.begin_step()
        for j in range(self.num_micro):
            r = a.rows_of(j)
            a.forward(j)
            a.pack_fwd(j)
            b.q_in[r].copy_(a.q_out[r])
            b.s_in[r].copy_(a.s_out[r])
            b.unpack_fwd(j)
            b.forward(j)
        for j in range(self.num_micro):
            r = a.rows_of(j)
            b.backward(j)
            b.pack_bwd(j)
            a.q_gin[r].copy_(b.q_dx[r])
            a.s_gin[r].copy_(b.s_dx[r])
            a.unpack_bwd(j)
            a.backward(j)
        for st in self.stages:
            st.wgrad()
            st.finalize_grads()
            st.optimizer_step()

    def flush(self):
        pass

    def loss(self):
        return self.stages[1].loss_sum() / (self.micro_batch * self.num_micro)

    def correct(self):
        return self.stages[1].head.correct_sum()


DECAY_OPTS = [dict(name="sgd", lr=0.5, weight_decay=1.0),
              dict(name="sgd", lr=0.5, momentum=0.5, weight_decay=1.0),
              dict(name="adamw", lr=0.5, weight_decay=1.0),
              dict(name="adam", lr=0.5, weight_decay=1.0)]
DECAY_IDS = ["sgd", "momentum", "adamw", "adam-l2"]


def check_padding_pinned(device, opt):
    """64 steps of a 70-72-10 sigmoid model at lr * weight_decay = 0.5 (see the callers)."""
    from docker_dist_nn_amd.engine import OptimConfig, Trainer
    from docker_dist_nn_amd.engine.params import PAD_OFF_BIAS

    assert PAD_OFF_BIAS * 0.5 ** 50 > -104  # the test crosses the threshold
    tr = Trainer(spec_of([70, 72, 10], ("sigmoid", "softmax")), micro_batch=64, num_micro=1,
                 optim=OptimConfig(**opt), device=device)
    st = tr.stages[0]
    x, y, _ = batch(64, 64, 70, st.x_in.shape[1], 10, 1, False)
    x, y = x.to(device), y.to(device)
    for _ in range(64):
        tr.set_batch(x, y)
        tr.step()
    tr.flush()
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    p = st.params
    assert bool((p.b32(0)[72:] == PAD_OFF_BIAS).all())
    assert torch.equal(p.shadow, p.master.to(torch.bfloat16))
    assert bool((st.acts[0][:, 72:] == 0).all())
    assert bool((p.w32(1)[:, 72:] == 0).all()) and bool((p.gw(1).view(64, 128)[:, 72:] == 0).all())
    assert bool(torch.isfinite(p.master).all()) and all(bool(torch.isfinite(t).all())
                                                        for t in p.state)
