"""Random layers for the mxfp4 device-side chain tests, and a CPU emulation of the two lane
orders of gemv_mxfp4_kernel, so that the tests which claim to pin the order can be shown to see
it.

The comparisons that pin the order are made on fp32 outputs of a linear layer: rounding the sum
to bf16 (8 significant bits) hides a difference in the last bits of an fp32 sum, and on the
operands below the two orders then agree in every bf16 output.

emulate(x, q, e, bias, B): lane l owns columns k0 + 64 B u + B l .. + B - 1 of every chunk of
64 B columns, chunks ascending, columns ascending, each product (exact in fp32) added to the
lane's fp32 accumulator; then wave_sum's butterfly (v += v[lane ^ o], o = 32 .. 1); then the
bias. B = 32 is the whole-block unit (1 and 2 rows at K >= 2048), B = 16 the half-block unit.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import _gemv_mxfp4_cases as gc
import _mxfp4_oracle as mo
from docker_dist_nn_amd import ops

# (N, K) of the random layers the GPU tests use
FUSED = [(1024, 832), (64, 2080)]
FOLDED = (1024, 1024)
LDS_LIMIT = (64, 4096)


def unit(rows: int, K: int) -> int:
    """Columns of a lane per chunk in gemv_mxfp4_kernel at this request size."""
    return 32 if rows <= 2 and K >= 2048 else 16


@functools.lru_cache(maxsize=None)
def random_layer(N: int, K: int):
    """_gemv_mxfp4_cases.layer_case(N, K, 8) quantised on the CPU by ops.quant_rows_mxfp4 (bit
    for bit the oracle, as the GPU quantiser is): (x bf16 [8][K], q, e uint8, bias fp32)."""
    w, b, x = gc.layer_case(N, K, 8)
    q = torch.empty(N, K // 2, dtype=torch.uint8)
    e = torch.empty(N, K // 32, dtype=torch.uint8)
    ops.quant_rows_mxfp4(w, q, e)
    return x, q, e, b


def emulate(x: torch.Tensor, q: torch.Tensor, e: torch.Tensor, bias: torch.Tensor,
            B: int) -> np.ndarray:
    """fp32 [rows][N]: the linear layer summed in the lane order of unit B."""
    w = mo.values(q.numpy(), e.numpy()).astype(np.float32)  # exact: two significant bits
    xf = x.float().numpy()
    M, K = xf.shape
    N = w.shape[0]
    chunk = 64 * B
    chunks = -(-K // chunk)
    wp = np.zeros((N, chunks * chunk), np.float32)
    xp = np.zeros((M, chunks * chunk), np.float32)
    wp[:, :K], xp[:, :K] = w, xf  # (a lane past K adds nothing: + 0 is exact)
    wp = wp.reshape(N, chunks, 64, B)
    xp = xp.reshape(M, chunks, 64, B)
    acc = np.zeros((M, N, 64), np.float32)
    for c in range(chunks):
        for j in range(B):
            prod = xp[:, None, c, :, j] * wp[None, :, c, :, j]  # exact in fp32
            acc = (acc + prod).astype(np.float32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[:, :, lanes ^ o]).astype(np.float32)
    return (acc[:, :, 0] + bias.numpy()[None, :N].astype(np.float32)).astype(np.float32)
