// Serving-size forward layer (1..GEMV_MAX_ROWS rows) over MXFP4 weight rows
// (csrc/kernels/gemv_mxfp4.hip): the weight format is that of quant_rows_mxfp4 (mxfp4.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dnn {

// y[m][n] = act(sum_k x[m][k] * e2m1(q[n][k]) * 2^(E[n][k / 32] - 127) + bias[n]) for m < M; x
// [M][ldx] bf16, q [N][ldq] bytes of two e2m1 codes (column 2j in the low nibble of byte j), e
// [N][lde] e8m0 block scales (a block with E == 0 adds nothing), y bf16 or fp32 (out_f32).
// K % 32 == 0, ldq >= K / 2, ldq % 16 == 0, lde >= K / 32, ldx >= K, ldx % 8 == 0, x and q
// 16-byte aligned. Error returns as gemv_fp8's.
int gemv_mxfp4(const uint16_t* x, long ldx, const unsigned char* q, long ldq,
               const unsigned char* e, long lde, const float* bias, void* y, long ldy, int M,
               int N, int K, int act, int out_f32, hipStream_t stream);

}  // namespace dnn
