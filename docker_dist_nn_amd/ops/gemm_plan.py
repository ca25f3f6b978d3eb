"""How a GEMM runs: the one place that chooses.

:func:`plan` resolves a product -- kind and the signature of :mod:`.tuning` -- into a
:class:`GemmPlan`: tile, split-K factor, main-loop form (stage code), persistent form and
whether the library path takes it. Its sources are the tuned table, the switches
``DNN_GEMM_STAGES`` / ``DNN_GEMM_PERSIST`` / ``DNN_BLAS`` (``DNN_TUNED`` inside the table lookup)
and the analytic fallbacks below; nothing else in the package reads them. :mod:`.kernels`
launches what a plan says, and the engine sizes its buffers (bias-gradient partials, split-K
slabs, fragment-order masks, loss partials) through the helpers at the end of this module, which
are views of the same plans -- so sizing and launch cannot disagree.
"""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass

from ..utils.native import native
from . import tuning
from .. import switches

KINDS = ("fwd", "dgrad", "wgrad", "xent")

# Main-loop forms of the native launcher (gemm_error_string -12 in csrc/kernels/gemm.hip)
STAGE_CODES = {
    0: "kernel default of the tile",
    2: "2-stage LDS pipeline", 3: "3-stage LDS pipeline", 4: "4-stage LDS pipeline",
    5: "A3/B2 ring (one-tile form, no fused xent)",
    6: "register-prefetched 2-deep ring, staged epilogue",
    8: "ping-pong half-tile-streamed 256x256 (gemm_pp.hip)",
    9: "register-prefetched 2-deep ring, register-direct epilogue (no ct / fused update)",
    11: "A3/B2 ring, register-direct epilogue (256x256, 256x128, 128x128)",
}
RP_STAGED, RP_DIRECT, RING_DIRECT = 6, 9, 11
DIRECT_STAGES = (RP_DIRECT, RING_DIRECT)  # take fragment-order masks; with ct / upd: RP_STAGED
GROUP_STAGES = 2  # the grouped launch is the 2-stage one-tile form

GEMV_MAX_ROWS = 8  # a forward of <= 8 rows is the GEMV kernel: no plan

# wave grid (WM, WN) of the register-direct tiles that take fragment-order masks (NB >= 4 bytes
# per lane; gemm_rp.hip pick_rp)
FRAG_WAVES = {(256, 256): (4, 2), (256, 128): (4, 2), (128, 128): (2, 2), (128, 64): (2, 2)}


def parse_kinds(name: str, spec: str, kinds, unset, conv=int, strict: bool = True) -> dict:
    """A per-kind switch: "" (every kind ``unset``), "v" (every kind v) or "kind=v,kind=v"
    (the others ``unset``); ``strict`` raises on a kind not in ``kinds``."""
    out = dict.fromkeys(kinds, unset)
    spec = spec.strip()
    if not spec:
        return out
    if "=" not in spec:
        return dict.fromkeys(kinds, conv(spec))
    for part in spec.split(","):
        k, v = part.split("=")
        if k.strip() in out:
            out[k.strip()] = conv(v)
        elif strict:
            raise ValueError(f"{name}: unknown GEMM kind {k!r}")
    return out


# DNN_GEMM_STAGES: stage code per kind, 0 = the table's / the kernel default. Read at import.
STAGES = parse_kinds("DNN_GEMM_STAGES", switches.get("DNN_GEMM_STAGES"), KINDS, 0)
# DNN_GEMM_PERSIST: None = the table decides, 0 / 1 = off / on, > 1 = an explicit workgroup
# count (csrc/kernels/gemm_persist.hip). Read at import.
PERSIST = parse_kinds("DNN_GEMM_PERSIST", switches.get("DNN_GEMM_PERSIST"), KINDS[:3], None)


def _persist(kind: str, entry) -> int:
    """Native `persist` argument: 0 = one tile per workgroup, -1 = one resident round of
    persistent workgroups, > 1 = that many workgroups."""
    v = PERSIST[kind] if PERSIST[kind] is not None else (entry or {}).get("persist", 0)
    return -1 if v == 1 else int(v)


def _blas_requested(kind: str, entry) -> bool:
    """Is the library (hipBLASLt) GEMM requested for this product? DNN_BLAS (read at every
    call): "" / "table" = the tuned table's ``blas`` flag, "0" = never, "1" = every product the
    library path supports, or per kind ("fwd=1,dgrad=0,wgrad=1"; unknown kinds are ignored, and
    blanks around a kind name are, as in the other two switches)."""
    spec = switches.get("DNN_BLAS").strip()
    if spec in ("", "table"):
        return bool((entry or {}).get("blas", 0))
    return parse_kinds("DNN_BLAS", spec, KINDS, "0", conv=str, strict=False)[kind] == "1"


_BLAS_WARNED = []


def blas_built() -> bool:
    """The library path exists only in the comparison build (``_build --blas``); the product
    build links no vendor GEMM library."""
    return bool(native().blas_available())


def _blas(kind: str, entry) -> bool:
    """Library GEMM for this product: requested (``_blas_requested``) AND built in."""
    if not _blas_requested(kind, entry):
        return False
    if blas_built():
        return True
    if not _BLAS_WARNED:
        _BLAS_WARNED.append(1)
        warnings.warn("DNN_BLAS asks for the hipBLASLt path, which is only in the comparison "
                      "build (python -m docker_dist_nn_amd._build --blas): own kernels run")
    return False


# Tile model: relative per-CU throughput of the 4-wave tile shapes (LDS/regs admit 2 128x128,
# 3 128x64 / 64x128 or 4 64x64 workgroups per CU; the 8-wave 256-row/-column tiles one).
_TILE_EFF = {(128, 128): 1.0, (128, 64): 0.82, (64, 128): 0.82, (64, 64): 0.62}
NUM_CU = 256


def pick_tiles(M: int, N: int, splits: int = 1) -> tuple[int, int]:
    """Tile for a [M][N] output (fwd / dgrad, M = batch rows).

    The 8-wave 256-row tiles stage half the LDS bytes per FLOP of the 128x128 tile and win
    whenever they still give >= 2 workgroups per CU (bench/stage_sweep.py on MI355X): 256x256
    for outputs >= 1024 wide, 256x64 for 128..1023. Otherwise: the 4-wave tile minimising
    modelled time = rounds of resident tiles x per-tile cost."""
    if splits == 1 and M % 256 == 0:
        if N % 256 == 0 and N >= 1024 and (M // 256) * (N // 256) >= 2 * NUM_CU:
            return 256, 256
        if N % 64 == 0 and N >= 128 and (M // 256) * (N // 64) >= 2 * NUM_CU:
            return 256, 64
    best, best_t = None, math.inf
    for (bm, bn) in _TILE_EFF:  # calibrated tiles only
        if M % bm or N % bn:
            continue
        tiles = (M // bm) * (N // bn) * splits
        # tiles resident on one CU share its matrix pipe: time ~ tiles per CU x tile cost
        t = math.ceil(tiles / NUM_CU) * bm * bn / _TILE_EFF[(bm, bn)]
        if t < best_t - 1e-9:
            best, best_t = (bm, bn), t
    if best is None:
        raise ValueError(f"no tile divides M={M}, N={N} (pad to multiples of 64)")
    return best


def _split_k_model(M: int, N: int, K_total: int, max_splits: int) -> tuple[int, int, int]:
    """Joint (bm, bn, splits) of the batch-contraction GEMM where the table has no entry.

    Splits may be uneven (k-ranges differ by at most one 64-step), so any S works. Resident
    workgroups share a CU, so time ~ ceil(tiles*S / CUs) / S tile-times (wave quantisation);
    each extra split adds an fp32 slab of M*N to write and re-read. E.g. 52 tiles: S=8 puts 2
    workgroups on 160 CUs and 1 on 96 (81% busy); S=14 gives 2-3 per CU (95%)."""
    ksteps = K_total // 64
    slab_cost = 2.0 * M * N * 4 / 5.0e12 * 0.6e15 / NUM_CU  # slab bytes in tile-FLOP units
    best, best_c = None, math.inf
    for (bm, bn), eff in _TILE_EFF.items():
        if M % bm or N % bn:
            continue
        tiles = (M // bm) * (N // bn)
        tile_flops = 2.0 * bm * bn * K_total / eff
        for s in range(1, min(max_splits, ksteps) + 1):
            c = math.ceil(tiles * s / NUM_CU) / s * tile_flops + (s > 1) * s * slab_cost
            if c < best_c * 0.995:
                best, best_c = (bm, bn, s), c
    if best is None:
        raise ValueError(f"no tile divides [{M}][{N}]")
    return best


@dataclass(frozen=True)
class GemmPlan:
    kind: str    # "fwd" | "dgrad" | "wgrad" | "xent"
    M: int       # the GEMM as the kernel sees it (the signatures of ops/tuning.py)
    N: int
    K: int
    tiles: tuple[int, int]
    splits: int
    stages: int  # STAGE_CODES key handed to the native launcher
    persist: int  # native persist argument, before a launch's features switch it off
    blas: bool   # library path requested AND built (the launch still probes the algorithm)
    blas_algo: int

    def launch_args(self, mask: bool = False, ct: bool = False, upd: bool = False) -> dict:
        """``gemm()`` keywords of one launch: the persistent form has no mask, transposed-copy
        or fused-update epilogue, so a launch with one of them is not persistent."""
        return dict(tiles=self.tiles, stages=self.stages,
                    persist=0 if (mask or ct or upd) else self.persist)


def plan(kind: str, M: int, N: int, K: int, splits: int | None = None,
         max_splits: int = 48) -> GemmPlan:
    """The configuration of one product. ``splits`` (wgrad): the split count the caller's slabs
    were sized for; the table's tile / stage code / persist flag were measured with the chosen
    count and apply only to it, another count runs ``pick_tiles`` on the kernel default.

    ``blas`` is resolved for every product, also for a launch that cannot take the library (a
    mask, the fused update, several splits, CPU tensors): when DNN_BLAS asks for the library,
    such a call now asks the extension whether it is built and may issue the once-only warning.
    No launch depends on it."""
    if kind == "xent":  # the whole padded row in one tile (bn == N)
        if N not in (64, 128):
            raise ValueError(f"fused cross-entropy supports 64 or 128 padded classes, got {N}")
        bm = 128 if M % 128 == 0 and M // 128 >= NUM_CU // 2 else 64
        if M % bm:
            raise ValueError("rows must be a multiple of 64")
        return GemmPlan(kind, M, N, K, (bm, N), 1, STAGES[kind], 0, False, 0)
    t = tuning.lookup(kind, M, N, K)
    blas = _blas(kind, t)
    algo = t.get("blas_algo", 0) if t else 0  # whatever split count the caller asks for
    if kind != "wgrad" or blas:  # the library GEMM contracts all rows in one fp32 output
        tiles, chosen = tuple(t["tile"]) if t else pick_tiles(M, N), 1
    elif t:
        tiles, chosen = tuple(t["tile"]), t["splits"]
    else:
        bm, bn, chosen = _split_k_model(M, N, K, max_splits)
        tiles = bm, bn
    if splits is not None and splits != chosen:  # not the measured configuration
        tiles, chosen, t = pick_tiles(M, N, splits), splits, None
    return GemmPlan(kind, M, N, K, tiles, chosen, STAGES[kind] or (t.get("stages", 0) if t else 0),
                    _persist(kind, t), blas, algo)


# ---- sizing: what the engine allocates from, before anything is launched -------------------

def pick_splits(M: int, N: int, K_total: int, max_splits: int = 48) -> int:
    """Split-K factor of the batch-contraction (wgrad) GEMM: the slab count."""
    return plan("wgrad", M, N, K_total, max_splits=max_splits).splits


def wgrad_config(M: int, N: int, K_total: int, max_splits: int = 48) -> tuple[int, int, int]:
    """(bm, bn, splits) of the batch-contraction GEMM."""
    p = plan("wgrad", M, N, K_total, max_splits=max_splits)
    return (*p.tiles, p.splits)


def dgrad_tiles(M: int, K: int, N: int = 0) -> tuple[int, int]:
    """Tile of linear_dgrad for an [M][K] output from an [M][N] gradient (fixes the colsum
    partial count); without N, the analytic rule alone."""
    return plan("dgrad", M, K, N).tiles if N else pick_tiles(M, K, 1)


def xent_tiles(M: int, N: int) -> tuple[int, int]:
    """Tile of the fused linear+softmax-CE GEMM (fixes the loss partial count)."""
    return plan("xent", M, N, 0).tiles


def frag_mask_tiles(M: int, N: int, K: int, N_next: int) -> tuple[int, int] | None:
    """Tile of a fragment-order mask between the forward [M][N] (contraction K) of a ReLU layer
    and the dgrad that produces its dZ from the next layer's [M][N_next] gradient, or None when
    those two GEMMs do not both run one register-direct tile shape."""
    f, d = plan("fwd", M, N, K), plan("dgrad", M, N, N_next)
    ok = (M > GEMV_MAX_ROWS and f.tiles == d.tiles and f.tiles in FRAG_WAVES and
          f.stages in DIRECT_STAGES and d.stages in DIRECT_STAGES and M % f.tiles[0] == 0 and
          not f.blas and not d.blas)
    return f.tiles if ok else None
