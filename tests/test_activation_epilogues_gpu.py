"""Activation epilogues of the GEMM kernels (every tile x stage-code form) and the two
elementwise epilogues of tensor parallelism, against an fp64 oracle (tests/_act_oracle.py).

Exact-product method: integer operands make the GEMM itself exact, so what is stored may differ
from fp64 only by the activation arithmetic and one bf16 rounding -- linear / ReLU bit for bit,
sigmoid within 1 bf16 ulp of RN_bf16(fp64). That pins the non-ReLU branches no other test
reaches: the register-direct aux epilogue (stage codes 9 / 11 and the persistent form: 8-byte
activation loads with clamped edge addresses, shift / mask unpack of bf16 pairs), the staged
act_bwd path, and the fp32-output forward activation.

Shapes: M = bm + 24, N = bn + 40 (one full and one partial tile each way, N a multiple of 8 but
not of 16), K = 64 and 192, plus one tile-multiple shape per form. aux and the output are views
into wider, taller buffers: aux padded with NaN, the output with a sentinel."""
import pytest
import torch

import _act_oracle as ao
from docker_dist_nn_amd.ops import KMAJ, MNMAJ

pytestmark = pytest.mark.gpu

TILES = [(128, 128), (128, 64), (64, 128), (64, 64), (256, 256), (256, 128), (128, 256),
         (256, 64)]
# register-prefetched forms: the RP list of tests/test_kernels_gpu.py
RP = [((256, 256), 6), ((256, 128), 6), ((128, 128), 6), ((128, 64), 6), ((64, 64), 6),
      ((256, 256), 9), ((256, 128), 9), ((128, 128), 9), ((128, 64), 9), ((64, 64), 9),
      ((256, 256), 11), ((256, 128), 11), ((128, 128), 11)]
# every (tile, stage code) gemm_bf16 accepts for these products; none of them rejects aux +
# sigmoid (gemm_check has no activation-specific rule), so there is no ValueError case
FORMS = ([(t, dict(stages=2)) for t in TILES] + [(t, dict(stages=5)) for t in TILES] +
         [(t, dict(stages=c)) for t, c in RP] + [(t, dict(persist=-1)) for t in TILES])
IDS = [f"{t[0]}x{t[1]}-" + "-".join(f"{k}{v}" for k, v in f.items()) for t, f in FORMS]
# one tile per stage family for the forward's layout sweep
FAMILIES = [dict(stages=2), dict(stages=5), dict(stages=6), dict(stages=9), dict(stages=11),
            dict(persist=-1)]

STATS = ao.new_stats()


def _seed(*parts):
    return sum((i + 1) * 7919 * int(p) for i, p in enumerate(parts)) % (2 ** 31)


def _report(name):
    s = STATS
    print(f"\nACTSTAT {name} sigmoid-bf16-differing fwd {s['fwd_diff']:.0f}/{s['fwd_elems']} "
          f"bwd {s['bwd_diff']:.0f}/{s['bwd_elems']} fp32-max-rel {s['f32_rel']:.3e} "
          f"fp32-max-rel/bound {s['f32_ratio']:.3f}")


@pytest.mark.parametrize("tiles,form", FORMS, ids=IDS)
def test_forward_activations_fp64(dev, tiles, form):
    bm, bn = tiles
    for (M, N, K) in ((bm + 24, bn + 40, 64), (bm + 24, bn + 40, 192), (2 * bm, 2 * bn, 64)):
        case = ao.fwd_case(M, N, K, KMAJ, KMAJ, _seed(M, N, K, form.get("stages", 1)))
        ao.check_fwd(case, dev, STATS, tiles=tiles, **form)
    _report("forward")


@pytest.mark.parametrize("la,lb", [l for l in ao.LAYOUTS if l != (KMAJ, KMAJ)])
@pytest.mark.parametrize("form", FAMILIES, ids=lambda f: "-".join(f"{k}{v}" for k, v in f.items()))
def test_forward_activations_layouts_fp64(dev, la, lb, form):
    bm, bn = 128, 128
    case = ao.fwd_case(bm + 24, bn + 40, 192, la, lb, _seed(la, lb, form.get("stages", 1)))
    ao.check_fwd(case, dev, STATS, tiles=(bm, bn), **form)


@pytest.mark.parametrize("tiles,form", FORMS, ids=IDS)
def test_backward_activations_fp64(dev, tiles, form):
    bm, bn = tiles
    for lb in (MNMAJ, KMAJ):  # w as stored / the transposed weight shadow
        for (M, N, K) in ((bm + 24, bn + 40, 64), (bm + 24, bn + 40, 192), (2 * bm, 2 * bn, 64)):
            case = ao.bwd_case(M, N, K, lb, _seed(M, N, K, lb, form.get("stages", 1)))
            ao.check_bwd(case, dev, tiles, STATS, **form)
    _report("backward")


@pytest.mark.parametrize("act", ao.ACTS)
@pytest.mark.parametrize("rows,cols,n_part", [(200, 192, 3), (64, 64, 1), (333, 128, 7)])
def test_dact_colsum_fp64(dev, act, rows, cols, n_part):
    """The library-GEMM dgrad's epilogue in the product build: rows no multiple of 32 nor of
    n_part, ld > cols on x and aux, with and without partials."""
    case = ao.dact_case(rows, cols, _seed(rows, cols, n_part))
    share = ao.check_dact_colsum(case, act, dev, n_part)
    ao.check_dact_colsum(case, act, dev, n_part, with_part=False)  # part = None: no write
    print(f"\nACTSTAT dact_colsum {act} {rows}x{cols} differing-share {share:.5f}")


@pytest.mark.parametrize("act", ao.ACTS)
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("rows,cols", [(200, 68), (37, 192)])
def test_bias_act_cast_fp64(dev, act, with_bias, rows, cols):
    """The row-parallel layer's epilogue: cols only a multiple of 4, ld > cols on x and y."""
    case = ao.bias_case(rows, cols, _seed(rows, cols))
    share = ao.check_bias_act_cast(case, act, dev, with_bias)
    print(f"\nACTSTAT bias_act_cast {act} {rows}x{cols} differing-share {share:.5f}")
