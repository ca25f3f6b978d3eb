// Forward layer over bf16 weight rows on the weight-streaming GEMM (csrc/kernels/linear_stream.hip):
// the serving counterpart of the training GEMM for buckets of 9 .. ~1000 rows, where a wide
// layer is bound by the bytes of W and not by the MFMA.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dnn {

// Forced tiles 1 .. LINEAR_STREAM_TILES (BM x BN, K split, waves):
//   1: 64 x 64 unsplit, 4    2: 64 x 32 2-way, 4    3: 64 x 32 4-way, 8
//   4: 128 x 128 unsplit, 8  5: 128 x 64 2-way, 8   6: 128 x 32 4-way, 8
constexpr int LINEAR_STREAM_TILES = 6;

// y[m][n] = act(sum_k x[m][k] * w[n][k] + bias[n]) for m < M, n < N; x [M][ldx] bf16, w [N][ldw]
// bf16 (nn.Linear layout), bias fp32 [N] or null, y bf16 or fp32 (out_f32) with any ldy >= N, act
// linear / relu / sigmoid. K % 32 == 0, ldx % 8 == 0, ldw % 8 == 0, x and w 16-byte aligned.
// Returns 0, or -1 (sizes), -2 (leading dimensions), -3 (null operand), -4 (activation), -5 (x / w
// alignment), -6 (y alignment), -7 (more row tiles than a grid holds), -8 (tile), -9 (launch
// failed).
// tile: 0 = chosen from M and N (linear_stream.hip); 1 .. LINEAR_STREAM_TILES force one (the
// tests and the benchmark's sweep; every tile gives the same sums on exact operands, not the same
// rounding on others).
int linear_stream(const uint16_t* x, long ldx, const uint16_t* w, long ldw, const float* bias,
                  void* y, long ldy, int M, int N, int K, int act, int out_f32, int tile,
                  hipStream_t stream);

}  // namespace dnn
