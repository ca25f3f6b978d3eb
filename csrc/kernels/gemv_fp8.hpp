// Serving-size forward layer (1..GEMV_MAX_ROWS rows) over fp8 weight rows
// (csrc/kernels/gemv_fp8.hip): the weight format is the row-scaled OCP e4m3 of quant_rows_fp8.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dnn {

// y[m][n] = act(fl32(scale[n] * sum_k x[m][k] * e4m3(q[n][k])) + bias[n]) for m < M; x [M][ldx]
// bf16, q [N][ldq] e4m3 codes (nn.Linear layout), scale fp32 [N], y bf16 or fp32 (out_f32).
// K % 16 == 0, ldq % 16 == 0, ldx % 8 == 0, x and q 16-byte aligned.
int gemv_fp8(const uint16_t* x, long ldx, const unsigned char* q, long ldq, const float* scale,
             const float* bias, void* y, long ldy, int M, int N, int K, int act, int out_f32,
             hipStream_t stream);

}  // namespace dnn
