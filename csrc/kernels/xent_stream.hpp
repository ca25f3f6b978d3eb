// Last layer + softmax cross-entropy for ANY class count without a logits matrix
// (csrc/kernels/xent_stream.hip): one workgroup per 64 rows sweeps the class tiles twice on the
// bf16 MFMA, weights streamed from global memory into the operand registers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dnn {

constexpr int XENT_STREAM_ROWS = 64;     // rows per workgroup = rows per partial
constexpr int XENT_STREAM_MAX_K = 1024;  // the block's x tile [64][K] bf16 stays in LDS: 128 KiB

// z = x[M][K] . w[N][K]^T + bias (never stored); over the first n_cls columns of every row with
// labels[row] >= 0:
//   dz[M][N] bf16 = (softmax(z) - onehot(label)) * scale, zeros in columns n_cls .. N and in rows
//   with a label < 0; loss_part[M / 64] = sum of the block's row losses; correct[M / 64] = rows
//   whose argmax (lowest column on ties) is the label; colsum[M / 64][>= N] (row stride
//   ld_colsum) = fp32 column sums of the block's STORED dz. loss_part, correct and colsum are
//   written, not accumulated, and each may be null.
// M % 64 == 0, N % 64 == 0, K % 64 == 0, 64 <= K <= XENT_STREAM_MAX_K, 0 < n_cls <= N; x and w
// 16-byte aligned with ldx % 8 == 0 and ldw % 8 == 0; bias fp32 [N]. Rows n_cls .. N of w and of
// bias may hold anything.
// Returns 0, or -1 (sizes), -2 (leading dimensions), -3 (null operand), -5 (alignment), -9
// (launch failed).
int xent_stream(const uint16_t* x, long ldx, const uint16_t* w, long ldw, const float* bias,
                const int* labels, uint16_t* dz, long ld_dz, int M, int N, int K, int n_cls,
                float scale, float* loss_part, int* correct, float* colsum, long ld_colsum,
                hipStream_t stream);

}  // namespace dnn
