// Forward layer over MXFP4 weight rows against e4m3 activations (csrc/kernels/linear_w4a8.hip):
// activations quantised per row by quant_rows_fp8 (elementwise.hpp) times the e2m1 codes and
// e8m0 block scales of quant_rows_mxfp4 (mxfp4.hpp), on the block-scaled MFMA of gfx950 in its
// mixed form (fp4 on one operand, fp8 on the other).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dnn {

// y[m][n] = act(fl32(sx[m] * S[m][n]) + bias[n]), S[m][n] = sum_k e4m3(xq[m][k]) * e2m1(q[n][k])
// * 2^(e[n][k / 32] - 127), a block with scale byte 0 contributing nothing, for m < M, n < N;
// xq [M][ldxq] e4m3 codes, sx fp32 [M], q [N][ldq] two e2m1 codes to a byte (column 2j in the
// low nibble), e [N][lde] one e8m0 byte per 32 columns (any alignment, any lde >= K / 32), bias
// fp32 [N] or null, y bf16 or fp32 (out_f32), act linear / relu / sigmoid. K % 32 == 0, ldxq %
// 16 == 0, ldq % 16 == 0, xq and q 16-byte aligned. Scale bytes 1..14 and 253..255 (never
// written by the quantiser) are not specified. Returns 0, or -1 (sizes), -2 (leading
// dimensions), -3 (null operand), -4 (activation), -5 (xq / q alignment), -6 (y alignment), -7
// (more row tiles than a grid holds), -8 (tile), -9 (launch failed).
// tile: 0 = chosen from M and N (linear_w4a8.hip); 1 / 2 force BM x BN = 64 x 64 / 128 x 128 (the
// tests and the benchmark's sweep; both give the same sums on exact operands, not necessarily
// the same rounding on others).
constexpr int LINEAR_W4A8_TILES = 2;
int linear_w4a8(const unsigned char* xq, long ldxq, const float* sx, const unsigned char* q,
                long ldq, const unsigned char* e, long lde, const float* bias, void* y, long ldy,
                int M, int N, int K, int act, int out_f32, int tile, hipStream_t stream);

}  // namespace dnn
