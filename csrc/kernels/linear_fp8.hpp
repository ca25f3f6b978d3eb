// Forward layer over fp8 weight rows for any number of input rows (csrc/kernels/linear_fp8.hip):
// the MFMA counterpart of gemv_fp8 (gemv_fp8.hpp), same weight format, same definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dnn {

// y[m][n] = act(fl32(scale[n] * sum_k x[m][k] * e4m3(q[n][k])) + bias[n]) for m < M, n < N;
// x [M][ldx] bf16, q [N][ldq] e4m3 codes (nn.Linear layout), scale fp32 [N], bias fp32 [N] or
// null, y bf16 or fp32 (out_f32), act linear / relu / sigmoid. K % 16 == 0, ldq % 16 == 0,
// ldx % 8 == 0, x and q 16-byte aligned. Returns 0, or -1 (sizes), -2 (leading dimensions),
// -3 (null operand), -4 (activation), -5 (x / q alignment), -6 (y alignment), -7 (more row
// tiles than a grid holds), -8 (tile), -9 (launch failed).
// tile: 0 = chosen from M and N (linear_fp8.hip); 1 .. 4 force BM x BN = 64 x 64, 64 x 32,
// 128 x 128, 128 x 64 (the tests and the benchmark's sweep; every tile gives the same sums on
// exact operands, not the same rounding on others).
int linear_fp8(const uint16_t* x, long ldx, const unsigned char* q, long ldq, const float* scale,
               const float* bias, void* y, long ldy, int M, int N, int K, int act, int out_f32,
               int tile, hipStream_t stream);

}  // namespace dnn
