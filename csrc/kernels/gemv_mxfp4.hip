// Skinny forward layer for serving (batch 1..8) over MXFP4 weight rows:
//   y[m][n] = act(S[m][n] + b[n]),  S[m][n] = sum_k x[m][k] * e2m1(q[n][k]) * 2^(E[n][k/32] - 127).
//
// The structure is gemv_fp8.hip's: one WAVE owns one output neuron and streams its weight row,
// whose bytes are the kernel's time. Here the row is the format of quant_rows_mxfp4 (mxfp4.hpp):
// 4-bit e2m1 codes, two to a byte, plus one e8m0 scale byte per 32 columns -- 17/32 of a byte
// per weight. The codes are decoded by the hardware conversion (v_cvt_scalef32_pk_f32_fp4: one
// byte of two codes to two fp32, the low nibble in element 0), which takes the block scale as
// an fp32 operand with the bit pattern E << 23 and applies it for free. dec * scale is exact
// (two significant bits, an exponent inside fp32's range for every E the quantiser writes), and
// its product with a bf16 x has at most 10 significant bits: exact in fp32. So there is no scale
// multiply and no rounding after the reduction; the error model is summation only. A block with
// E == 0 adds nothing whatever its codes hold: its code words are cleared before the
// conversion (one select per 8 columns), so the rule does not rest on what the conversion
// makes of a zero scale operand.
//
// The unit of a lane is half a block or a whole block, chosen by registers and by K:
//   half   8 bytes of codes (16 columns), the block's scale byte (two neighbouring lanes read the
//          same one), 16 bf16 of each input row with two 16-byte loads: the 16-column unit of
//          gemv_fp8.hip, a chunk of 64 x 16 = 1024 columns; 2 + 1 + 8 M registers per chunk.
//   whole  16 bytes of codes, the scale byte, 32 bf16 of each row with four loads; a chunk of
//          2048 columns; 4 + 1 + 16 M registers per chunk.
// At equal columns per sweep the two hold the same bytes in flight; the whole block needs half
// the load instructions and address registers. At 8 rows a whole block is 133 registers per
// chunk, so an unroll of 2 (266) cannot fit in the 256 a wave can address, and with one chunk
// per sweep it measured SLOWER than the half block at 4 and 8 rows (37.6 / 73.9 us against
// 33.7 / 61.4 us on a cold 8192 x 8192 layer). At 1 and 2 rows it is faster (13.0 / 22.1 us
// against 17.0 / 23.0): the 1-row instantiation drops from 71 to 64 VGPRs, 8 waves per SIMD,
// which is what 8192 rows need to be resident at once on 256 CUs. Below 2048 columns half the
// lanes of a whole-block wave would idle, so such rows keep the half block at any row count.
// All loads of a sweep are issued before any is used.
//
// Registers (hipcc -O3 for gfx950, kernel-resource-usage remark; no instantiation has scratch;
// out_f32 and bf16 output are the same):
//   rows M   K        unit         chunk   unroll U   in flight per lane   VGPRs   waves/SIMD
//     1      >= 2048  32 columns   2048       2       (5 + 16 M) U =  42     64        8
//     2      >= 2048  32 columns   2048       2                       74    122        4
//     1      <  2048  16 columns   1024       4       (3 +  8 M) U =  44     71        7
//     2      <  2048  16 columns   1024       4                       76    128        4
//     4      any      16 columns   1024       2                       70    132        3
//     8      any      16 columns   1024       2                      134    212        2
// A sweep of the k loop is therefore 4096 columns for 1 or 2 rows and 2048 for 3 to 8, as in
// gemv_fp8.hip.
#include "common.hpp"
#include "gemv.hpp"
#include "gemv_mxfp4.hpp"

namespace dnn {

constexpr int GEMV4_WAVES = 4;  // waves (= output neurons) per 256-thread block
// 1 and 2 rows: a lane takes a whole block from this K on (one full chunk of 64 blocks)
constexpr int GEMV4_WHOLE_BLOCK_MIN_K = 2048;

typedef float f32x2_t __attribute__((ext_vector_type(2)));
template <int W>
using qword_t = unsigned __attribute__((ext_vector_type(W)));  // W code words: one 8 W-byte load

// M = compile-time row capacity (1, 2, 4, 8); rows = actual rows (<= M): rows beyond `rows`
// are never read or written.
// B = columns per lane and chunk: 16 (half a block) or 32 (a whole block); a chunk is 64 B columns.
template <int M, int U, int B, bool OUT_F32>
__global__ __launch_bounds__(256) void gemv_mxfp4_kernel(
    const u16* __restrict__ x, long ldx, const unsigned char* __restrict__ q, long ldq,
    const unsigned char* __restrict__ e, long lde, const float* __restrict__ bias,
    void* __restrict__ y, long ldy, int rows, int N, int K, int act) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * GEMV4_WAVES + (threadIdx.x >> 6);
  if (n >= N) return;  // whole wave exits together
  const unsigned char* qr = q + (long)n * ldq;
  const unsigned char* er = e + (long)n * lde;
  constexpr int CHUNK = 64 * B, W = B / 8;  // W: code words = 8-column x vectors of a unit
  float acc[M];
#pragma unroll
  for (int m = 0; m < M; ++m) acc[m] = 0.f;
  // K is a multiple of 32: a lane's B columns are inside K or wholly outside
  for (int k0 = 0; k0 < K; k0 += CHUNK * U) {
    qword_t<W> qv[U];
    unsigned ev[U];
    bf16x8_t xv[U][M][W];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + u * CHUNK + lane * B;
      if (k < K) {
        qv[u] = *(const qword_t<W>*)(qr + (k >> 1));
        ev[u] = er[k >> 5];
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
          for (int j = 0; j < W; ++j)
            xv[u][m][j] = m < rows ? *(const bf16x8_t*)(x + m * ldx + k + 8 * j) : bf16x8_t{};
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + u * CHUNK + lane * B;
      if (k < K) {
        const float scale = __uint_as_float(ev[u] << 23);  // 2^(E - 127)
#pragma unroll
        for (int j = 0; j < W; ++j) {  // word j holds columns k + 8 j .. k + 8 j + 7
          const unsigned word = ev[u] ? qv[u][j] : 0u;  // a block with E == 0 adds nothing
          const f32x2_t d[4] = {__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, scale, 0),
                                __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, scale, 1),
                                __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, scale, 2),
                                __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, scale, 3)};
#pragma unroll
          for (int c = 0; c < 8; ++c) {  // byte c / 2 of the word: its low nibble first
            const float we = d[c >> 1][c & 1];
#pragma unroll
            for (int m = 0; m < M; ++m) acc[m] += we * bf2f((u16)xv[u][m][j][c]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < M; ++m) acc[m] = wave_sum(acc[m]);
  if (lane < rows) {
    float v = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m)
      if (m == lane) v = acc[m];
    v += bias ? bias[n] : 0.f;
    v = act_fwd(v, act);
    if constexpr (OUT_F32)
      ((float*)y)[(long)lane * ldy + n] = v;
    else
      ((u16*)y)[(long)lane * ldy + n] = f2bf(v);
  }
}

int gemv_mxfp4(const uint16_t* x, long ldx, const unsigned char* q, long ldq,
               const unsigned char* e, long lde, const float* bias, void* y, long ldy, int M,
               int N, int K, int act, int out_f32, hipStream_t stream) {
  if (M < 1 || M > GEMV_MAX_ROWS || N < 1 || K < 32 || K % 32) return -1;
  if (ldx < K || ldq < K / 2 || lde < K / 32 || ldy < N || ldx % 8 || ldq % 16) return -2;
  if (!e || !y) return -3;
  if ((((uintptr_t)x) | ((uintptr_t)q)) & 15) return -5;
  const dim3 grid((N + GEMV4_WAVES - 1) / GEMV4_WAVES), block(256);
#define DNN_GEMV4(MM, UU, BB)                                                                  \
  if (out_f32)                                                                                 \
    hipLaunchKernelGGL((gemv_mxfp4_kernel<MM, UU, BB, true>), grid, block, 0, stream, x, ldx,  \
                       q, ldq, e, lde, bias, y, ldy, M, N, K, act);                            \
  else                                                                                         \
    hipLaunchKernelGGL((gemv_mxfp4_kernel<MM, UU, BB, false>), grid, block, 0, stream, x, ldx, \
                       q, ldq, e, lde, bias, y, ldy, M, N, K, act);
  switch (M) {
    case 1:
      if (K >= GEMV4_WHOLE_BLOCK_MIN_K) { DNN_GEMV4(1, 2, 32) } else { DNN_GEMV4(1, 4, 16) }
      break;
    case 2:
      if (K >= GEMV4_WHOLE_BLOCK_MIN_K) { DNN_GEMV4(2, 2, 32) } else { DNN_GEMV4(2, 4, 16) }
      break;
    case 3:  // rows 3..4 on the 4-row kernel, 5..8 on the 8-row one (guarded by `rows`)
    case 4: DNN_GEMV4(4, 2, 16) break;
    default: DNN_GEMV4(8, 2, 16) break;
  }
#undef DNN_GEMV4
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

}  // namespace dnn
