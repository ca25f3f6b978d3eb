"""Cases and recorder of the GEMM launch record (tests/golden/gemm_launches.json).

Every case drives the public ``ops.linear_*`` entry points on operands that only look like GPU
tensors (``torch.empty`` storage viewed as a Tensor subclass whose ``is_cuda`` is True) with the
native extension replaced by a recorder: nothing is launched, and each native call is kept as
``[case, call, name, args, kwargs]`` with every scalar as is and every pointer reduced to the
name of the operand it addresses. The record says which configuration (tile, split-K, stage
code, persistent form, library path) every product gets under the default switches, for every
signature of the tuned table and a set of untuned shapes, and under the GEMM switches for a
fixed subset.

``python tests/_gemm_launch_cases.py`` rewrites the golden file from the tree it runs in; the
test only reads it.
"""
from __future__ import annotations

import contextlib
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from docker_dist_nn_amd import ops  # noqa: E402
from docker_dist_nn_amd.ops import kernels, tuning  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_launches.json")
BF16, F32, U8, I32 = torch.bfloat16, torch.float32, torch.uint8, torch.int32


class _Gpu(torch.Tensor):
    is_cuda = True


def _switch_home():
    """The module that holds the parsed DNN_GEMM_STAGES / DNN_GEMM_PERSIST dicts."""
    try:
        from docker_dist_nn_amd.ops import gemm_plan
        return gemm_plan
    except ImportError:
        return kernels


class Operands:
    """Fake GPU tensors of one call, and the map from their addresses back to their names."""

    def __init__(self):
        self.names, self.keep = {}, []

    def __call__(self, name, *shape, dtype=BF16):
        t = torch.empty(*shape, dtype=dtype).as_subclass(_Gpu)
        self.names[t.data_ptr()] = name
        self.keep.append(t)
        return t

    def scrub(self, v):
        if isinstance(v, (list, tuple)):
            return [self.scrub(e) for e in v]
        if isinstance(v, dict):
            return {k: self.scrub(e) for k, e in v.items()}
        if isinstance(v, bool):
            return int(v)
        if isinstance(v, int) and v in self.names:
            return self.names[v]
        assert isinstance(v, (int, float, str)) and not (isinstance(v, int) and v > 1 << 32), v
        return v


class Recorder:
    """Stands in for the native extension: answers the two library-path questions as the case
    says and appends every other call to ``calls``."""

    def __init__(self, built: bool, supported: bool):
        self.built, self.supported, self.calls, self.operands = built, supported, [], None

    def blas_available(self):
        return self.built

    def __getattr__(self, name):
        def call(*args, **kwargs):
            self.calls.append([name, self.operands.scrub(args), self.operands.scrub(kwargs)])
            return self.supported if name == "blas_supported" else None
        return call


@contextlib.contextmanager
def patched(rec: Recorder, setting: dict):
    """Recorder in place of the extension, stream 0, and the case's switches."""
    home = _switch_home()
    mods = {kernels, home}
    saved_native = {m: m.native for m in mods if hasattr(m, "native")}
    saved_stream = kernels._stream
    saved_env = {k: os.environ.get(k) for k in ("DNN_TUNED", "DNN_BLAS")}
    saved_dicts = (dict(home.STAGES), dict(home.PERSIST))
    try:
        for m in saved_native:
            m.native = lambda: rec
        kernels._stream = lambda t: 0
        kernels._BLAS_OK.clear()
        for k in saved_env:
            os.environ.pop(k, None)
        os.environ.update(setting.get("env", {}))
        home.STAGES.update(setting.get("stages", {}))
        home.PERSIST.update(setting.get("persist", {}))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            yield
    finally:
        for m, f in saved_native.items():
            m.native = f
        kernels._stream = saved_stream
        kernels._BLAS_OK.clear()
        for k, v in saved_env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        home.STAGES.update(saved_dicts[0])
        home.PERSIST.update(saved_dicts[1])


# ---- settings ------------------------------------------------------------------------------

ALL3 = {"fwd": 3, "dgrad": 3, "wgrad": 3, "xent": 3}
DEFAULT = {"id": "default"}
SETTINGS = [
    {"id": "tuned0", "env": {"DNN_TUNED": "0"}},
    {"id": "stages3", "stages": ALL3},
    {"id": "stages-fwd9-dgrad2", "stages": {"fwd": 9, "dgrad": 2}},
    {"id": "persist0", "persist": {"fwd": 0, "dgrad": 0, "wgrad": 0}},
    {"id": "persist1", "persist": {"fwd": 1, "dgrad": 1, "wgrad": 1}},
    {"id": "persist-fwd300", "persist": {"fwd": 300}},
    {"id": "blas1-built", "env": {"DNN_BLAS": "1"}, "built": True},
    {"id": "blas1-unbuilt", "env": {"DNN_BLAS": "1"}},
    {"id": "blas-wgrad1-built", "env": {"DNN_BLAS": "wgrad=1"}, "built": True},
    {"id": "blas-wgrad1-unbuilt", "env": {"DNN_BLAS": "wgrad=1"}},
    # the library is built and asked for, but has no algorithm for the problem
    {"id": "blas1-built-unsupported", "env": {"DNN_BLAS": "1"}, "built": True,
     "supported": False},
]

# ---- shapes: (kind, M, N, K) in the signatures of ops/tuning.py -----------------------------


def table_signatures():
    out = []
    for key in sorted(tuning.load_table(tuning.DEFAULT_PATH)):
        kind, dims = key.split(":")
        out.append((kind, *map(int, dims.split("x"))))
    return out


# layers (input width, output width) of the untuned shapes
LAYERS = [(832, 128), (1024, 1024), (256, 192), (2048, 2048)]
ROWS = [64, 192, 1024, 4096]


def untuned_signatures():
    out = []
    for rows in ROWS:
        for k_in, n_out in LAYERS:
            out += [("fwd", rows, n_out, k_in), ("dgrad", rows, k_in, n_out),
                    ("wgrad", n_out, k_in, rows)]
        out += [("xent", rows, 64, 128), ("xent", rows, 128, 256)]
    out += [("fwd", 8, 128, 832), ("fwd", 8, 1024, 1024)]  # serving rows: the GEMV branch
    out += [("xent", 65536, 64, 128), ("xent", 65536, 128, 256)]
    return out


# table hits and misses of every kind, run under every entry of SETTINGS
SWITCH_SUBSET = [
    ("fwd", 65536, 512, 832), ("fwd", 65536, 1024, 1024), ("fwd", 4096, 1024, 1024),
    ("fwd", 192, 192, 256),
    ("dgrad", 131072, 512, 256), ("dgrad", 65536, 1024, 1024), ("dgrad", 4096, 1024, 1024),
    ("dgrad", 1024, 832, 128),
    ("wgrad", 1024, 1024, 65536), ("wgrad", 8192, 8192, 16384), ("wgrad", 1024, 1024, 4096),
    ("wgrad", 128, 832, 64),
    ("xent", 65536, 64, 128),
]
# call variants of the switch runs: a reduced set (the golden file stays small); the default
# run takes every variant but "one", the plain one-split wgrad that only the library path takes
SWITCH_VARIANTS = {"fwd": ("plain", "yt", "mask"), "dgrad": ("wt+cs", "mask", "dxt"),
                   "wgrad": ("s", "s+1", "one", "upd"), "xent": ("xent",)}
DEFAULT_SKIPS = ("one",)

WIDTHS = (64, 128, 192, 256, 512, 832, 1024, 2048, 8192)

# which per-launch features a call variant switches on (GemmPlan.launch_args)
FEATURES = {"yt": {"ct": True}, "mask": {"mask": True}, "dxt": {"ct": True},
            "upd": {"upd": True, "ct": True}}


# ---- the calls -----------------------------------------------------------------------------

def _frag_pair(M, N, fixed, fixed_is_k):
    """First (K, N_next) around a [M][N] activation for which a fragment mask exists."""
    for other in WIDTHS:
        k, n_next = (fixed, other) if fixed_is_k else (other, fixed)
        tiles = ops.frag_mask_tiles(M, N, k, n_next)
        if tiles is not None:
            return tiles
    return None


def fwd_calls(M, N, K):
    def base(o, ydt=BF16):
        return o("x", M, K), o("w", N, K), o("bias", N, dtype=F32), o("y", M, N, dtype=ydt)

    def plain(o):
        ops.linear_fwd(*base(o), act="relu")

    def f32(o):
        ops.linear_fwd(*base(o, F32), act="linear")

    def yt(o):
        ops.linear_fwd(*base(o), act="relu", yt=o("yt", N, M))

    def bmask(o):
        ops.linear_fwd(*base(o), act="relu", mask=o("mask", M, -(-N // 8), dtype=U8))

    calls = {"plain": plain, "f32": f32}
    if M > ops.GEMV_MAX_ROWS:
        tiles = _frag_pair(M, N, K, True)

        def fmask(o):
            buf = o("fragmask", ops.FragMask.nbytes(M, N, tiles), dtype=U8)
            ops.linear_fwd(*base(o), act="relu", mask=ops.FragMask(buf, tiles, M, N))
        # the fragment-order mask where the layer pair has one, else row-block-major bytes
        calls.update(yt=yt, mask=bmask if tiles is None else fmask)
    return calls


def dgrad_calls(M, N, K):
    """[M][N] input gradient from an [M][K] output gradient (w is [K][N])."""
    def base(o):
        return o("dz", M, K), o("w", K, N), o("dx", M, N)

    def colsum(o):
        return o("colsum", -(-M // ops.dgrad_tiles(M, N, K)[0]), N, dtype=F32)

    def w(o):
        ops.linear_dgrad(*base(o), o("y_prev", M, N), "relu")

    def wt_cs(o):
        ops.linear_dgrad(*base(o), o("y_prev", M, N), "relu", colsum=colsum(o),
                         wt=o("wt", N, K))

    def bmask(o):
        ops.linear_dgrad(*base(o), colsum=colsum(o), wt=o("wt", N, K),
                         mask_prev=o("mask", M, -(-N // 8), dtype=U8))

    def dxt(o):
        ops.linear_dgrad(*base(o), o("y_prev", M, N), "relu", colsum=colsum(o),
                         wt=o("wt", N, K), dxt=o("dxt", N, M))

    tiles = _frag_pair(M, N, K, False)

    def fmask(o):
        buf = o("fragmask", ops.FragMask.nbytes(M, N, tiles), dtype=U8)
        ops.linear_dgrad(*base(o), colsum=colsum(o), wt=o("wt", N, K),
                         mask_prev=ops.FragMask(buf, tiles, M, N))
    return {"w": w, "wt+cs": wt_cs, "mask": bmask if tiles is None else fmask, "dxt": dxt}


def wgrad_calls(M, N, K):
    """[M][N] weight gradient contracted over K batch rows."""
    R, s = K, ops.pick_splits(M, N, K)

    def rowmajor(o, splits):
        return o("dz", R, M), o("x", R, N), o("slabs", splits, M, N, dtype=F32)

    def upd(o):
        return dict(master=o("master", M, N, dtype=F32), mom=o("mom", M, N, dtype=F32),
                    shadow=o("shadow", M, N), lr_dev=o("lr", 1, dtype=F32), momentum=0.9,
                    weight_decay=1e-4)

    return {
        "s": lambda o: ops.linear_wgrad(*rowmajor(o, s), splits=s),
        "s+1": lambda o: ops.linear_wgrad(*rowmajor(o, s + 1), splits=s + 1),
        "acc": lambda o: ops.linear_wgrad(*rowmajor(o, s), splits=s, accumulate=True),
        "kk": lambda o: ops.linear_wgrad(*rowmajor(o, s), splits=s, dzt=o("dzt", M, R),
                                         xt=o("xt", N, R)),
        "kk-s+1": lambda o: ops.linear_wgrad(*rowmajor(o, s + 1), splits=s + 1,
                                             dzt=o("dzt", M, R), xt=o("xt", N, R)),
        "one": lambda o: ops.linear_wgrad(*rowmajor(o, 1), splits=1),
        "upd": lambda o: ops.linear_wgrad(*rowmajor(o, 1), splits=1, dzt=o("dzt", M, R),
                                          xt=o("xt", N, R), upd=upd(o), wt=o("wt", N, M)),
    }


def xent_calls(M, N, K):
    def xent(o):
        bm = ops.xent_tiles(M, N)[0]
        ops.linear_fwd_xent(o("x", M, K), o("w", N, K), o("bias", N, dtype=F32), o("dz", M, N),
                            o("labels", M, dtype=I32), 10, 1.0 / M,
                            loss_part=o("loss", M // bm, dtype=F32),
                            correct=o("correct", M // bm, dtype=I32),
                            colsum=o("colsum", M // bm, N, dtype=F32))
    return {"xent": xent}


CALLS = {"fwd": fwd_calls, "dgrad": dgrad_calls, "wgrad": wgrad_calls, "xent": xent_calls}

# (output width, input width) of the weight gradients of the batch-64 recipe model 784-128-64-10
RECIPE_ROWS, RECIPE = 64, [(128, 832), (64, 128), (64, 64)]
# eligible small items among a big one, a persistent / register-direct table entry, an item
# whose splits differ from the chosen ones and one with fewer than 64 rows per split
MIXED = [(4096, 128, 256, 0), (4096, 1024, 1024, 0), (4096, 64, 128, 0), (65536, 128, 256, 0),
         (4096, 128, 256, 1), (4096, 64, 64, 0), (64, 64, 64, 1), (4096, 128, 832, 0)]


def group_calls():
    def run(o, shapes):
        items = []
        for i, (R, N, K, extra) in enumerate(shapes):
            s = ops.pick_splits(N, K, R) + extra
            items.append((o(f"dz{i}", R, N), o(f"x{i}", R, K), o(f"slabs{i}", s, N, K, dtype=F32),
                          s, bool(i % 2)))
        return ops.linear_wgrad_group(items)

    return {"recipe": lambda o: run(o, [(RECIPE_ROWS, n, k, 0) for n, k in RECIPE]),
            "mixed": lambda o: run(o, MIXED)}


def helper_values(kind, M, N, K):
    """Return values of the sizing helpers for one signature."""
    def val(f, *a):
        try:
            r = f(*a)
            return list(r) if isinstance(r, tuple) else r
        except ValueError:
            return "ValueError"

    def frag(args):  # over the candidate widths of the other layer; None results left out
        got = {str(w): val(ops.frag_mask_tiles, *args(w)) for w in WIDTHS}
        return {w: t for w, t in got.items() if t is not None}

    if kind == "fwd":
        return {"pick_tiles": val(ops.pick_tiles, M, N),
                "frag_mask_tiles": frag(lambda n: (M, N, K, n))}
    if kind == "dgrad":
        return {"pick_tiles": val(ops.pick_tiles, M, N), "dgrad_tiles": val(ops.dgrad_tiles, M, N, K),
                "dgrad_tiles_noN": val(ops.dgrad_tiles, M, N),
                "frag_mask_tiles": frag(lambda k: (M, N, k, K))}
    if kind == "wgrad":
        s = val(ops.pick_splits, M, N, K)
        return {"pick_splits": s, "wgrad_config": val(ops.wgrad_config, M, N, K),
                "pick_splits_max8": val(ops.pick_splits, M, N, K, 8),
                "pick_tiles": val(ops.pick_tiles, M, N, s if isinstance(s, int) else 1)}
    return {"xent_tiles": val(ops.xent_tiles, M, N)}


# ---- running -------------------------------------------------------------------------------

def sig_id(sig):
    kind, M, N, K = sig
    return f"{kind}:{M}x{N}x{K}"


def cases():
    """[(case id, setting, signature or None = the grouped launches, variants or None = all
    but DEFAULT_SKIPS)]."""
    out = [(f"default|{sig_id(s)}", DEFAULT, s, None)
           for s in table_signatures() + untuned_signatures()]
    out.append(("default|group", DEFAULT, None, None))
    for st in SETTINGS:
        out += [(f"{st['id']}|{sig_id(s)}", st, s, SWITCH_VARIANTS[s[0]]) for s in SWITCH_SUBSET]
        out.append((f"{st['id']}|group", st, None, None))
    return out


def run_case(case):
    """Records of one case: [case id, call, native name, args, kwargs] per native call, a
    ``raises`` record for a call that raised, and one ``helpers`` record per signature."""
    cid, setting, sig, only = case
    out = []
    rec = Recorder(setting.get("built", False), setting.get("supported", True))
    with patched(rec, setting):
        calls = group_calls() if sig is None else CALLS[sig[0]](*sig[1:])
        for label, fn in calls.items():
            if label in DEFAULT_SKIPS if only is None else label not in only:
                continue
            rec.calls, rec.operands = [], Operands()
            try:
                returned = fn(rec.operands)
                if sig is None:  # linear_wgrad_group: the items it did not launch
                    rec.calls.append(["returned", [returned], {}])
            except ValueError:
                rec.calls.append(["raises", ["ValueError"], {}])
            out += [[cid, label, *c] for c in rec.calls]
        if sig is not None:
            out.append([cid, "helpers", "values", [], helper_values(*sig)])
    return out


def run_all():
    return [r for c in cases() for r in run_case(c)]


def load_golden():
    """Records of the golden file, with the interned kwargs names expanded."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    return [[*r[:4], dict(zip(doc["kwargs"][r[4]], r[5]))] for r in doc["records"]]


def record(path=GOLDEN):
    """Write the golden file: one record per line."""
    dumps = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
    names, lines = [], []
    for *head, kwargs in run_all():  # kwargs names are interned: a record holds index + values
        keys = sorted(kwargs)
        if keys not in names:
            names.append(keys)
        lines.append(dumps([*head, names.index(keys), [kwargs[k] for k in keys]]))
    with open(path, "w") as f:
        f.write('{"kwargs":' + dumps(names) + ',\n"records":[\n' + ",\n".join(lines)
                + "\n]}\n")


if __name__ == "__main__":
    record(*sys.argv[1:])
    print(os.path.getsize(sys.argv[1] if len(sys.argv) > 1 else GOLDEN), "bytes")
