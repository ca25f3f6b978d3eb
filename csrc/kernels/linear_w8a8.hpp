// Forward layer with e4m3 codes on BOTH operands (csrc/kernels/linear_w8a8.hip): activations
// quantised per row by quant_rows_fp8 (elementwise.hpp) times fp8 weight rows of the same
// format, on the block-scaled fp8 MFMA of gfx950.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dnn {

// y[m][n] = act(fl32(sx[m] * fl32(sw[n] * S[m][n])) + bias[n]), S[m][n] = sum_k e4m3(xq[m][k]) *
// e4m3(q[n][k]), for m < M, n < N; xq [M][ldxq] and q [N][ldq] e4m3 codes, sx fp32 [M], sw fp32
// [N], bias fp32 [N] or null, y bf16 or fp32 (out_f32), act linear / relu / sigmoid. K % 16 == 0,
// ldxq % 16 == 0, ldq % 16 == 0, xq and q 16-byte aligned. Returns 0, or -1 (sizes), -2 (leading
// dimensions), -3 (null operand), -4 (activation), -5 (xq / q alignment), -6 (y alignment), -7
// (more row tiles than a grid holds), -8 (tile), -9 (launch failed).
// tile: 0 = chosen from M and N (linear_w8a8.hip); 1 / 2 force BM x BN = 64 x 64 / 128 x 128 (the
// tests and the benchmark's sweep; both give the same sums on exact operands, not necessarily
// the same rounding on others).
constexpr int LINEAR_W8A8_TILES = 2;
int linear_w8a8(const unsigned char* xq, long ldxq, const float* sx, const unsigned char* q,
                long ldq, const float* sw, const float* bias, void* y, long ldy, int M, int N,
                int K, int act, int out_f32, int tile, hipStream_t stream);

}  // namespace dnn
