// Skinny forward layer for serving (batch 1..8) over fp8 weight rows:
//   y[m][n] = act(fl32(scale[n] * S[m][n]) + b[n]),  S[m][n] = sum_k x[m][k] * e4m3(q[n][k]).
//
// The structure is gemv.hip's: one WAVE owns one output neuron and streams its weight row,
// whose bytes are the kernel's time. Here the row is OCP e4m3 codes with one fp32 scale -- the
// format of quant_rows_fp8 (elementwise.hip), whose row is exactly this wave's row -- so the
// row is half the bytes and the scale multiplies the reduced sum once per output, never per
// element. A lane reads 16 codes with one 16-byte load (a chunk is 64 x 16 = 1024 columns) and
// the matching 16 bf16 of each input row with two; all loads of U chunks are issued before
// any is used. The codes are decoded by the hardware conversion (v_cvt_pk_f32_fp8: OCP on
// gfx950; 0x7F / 0xFF decode to NaN). dec * x is exact in fp32 (4 x 8 significant bits), so
// the accumulation has the error model of the bf16 kernel; the scale multiply is one more
// rounding (kept apart from the bias add: no fused multiply-add there).
//
// Registers (hipcc -O3 for gfx950, kernel-resource-usage remark; no instantiation has scratch;
// out_f32 and bf16 output are the same):
//   rows capacity M   unroll U   in flight per lane (4 + 8 M) U   VGPRs   waves/SIMD
//         1              4                48                        64        8
//         2              4                80                       126        4
//         4              2                72                       132        3
//         8              2               136                       212        2
// (the counts exceed what is in flight because the compiler widens bf16 x values to fp32
// ahead of their use, as it does in gemv.hip: 46 / 82 / 148 / 248 there. 8 rows at U = 4 would
// hold 272 registers in flight: more than the 256 a wave can address without spilling.) A
// sweep of the k loop is therefore 4096 columns for 1 or 2 rows and 2048 for 3 to 8.
#include "common.hpp"
#include "gemv.hpp"
#include "gemv_fp8.hpp"

namespace dnn {

constexpr int GEMV8_WAVES = 4;     // waves (= output neurons) per 256-thread block
constexpr int GEMV8_CHUNK = 1024;  // columns per chunk: 64 lanes x 16 codes

typedef float f32x2_t __attribute__((ext_vector_type(2)));

// M = compile-time row capacity (1, 2, 4, 8); rows = actual rows (<= M): rows beyond `rows`
// are never read or written.
template <int M, int U, bool OUT_F32>
__global__ __launch_bounds__(256) void gemv_fp8_kernel(const u16* __restrict__ x, long ldx,
                                                       const unsigned char* __restrict__ q,
                                                       long ldq, const float* __restrict__ scale,
                                                       const float* __restrict__ bias,
                                                       void* __restrict__ y, long ldy, int rows,
                                                       int N, int K, int act) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * GEMV8_WAVES + (threadIdx.x >> 6);
  if (n >= N) return;  // whole wave exits together
  const unsigned char* qr = q + (long)n * ldq;
  float acc[M];
#pragma unroll
  for (int m = 0; m < M; ++m) acc[m] = 0.f;
  // K is a multiple of 16: a lane's 16 columns are inside K or wholly outside
  for (int k0 = 0; k0 < K; k0 += GEMV8_CHUNK * U) {
    uint4 qv[U];
    bf16x8_t xv[U][M][2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + u * GEMV8_CHUNK + lane * 16;
      if (k < K) {
        qv[u] = *(const uint4*)(qr + k);
#pragma unroll
        for (int m = 0; m < M; ++m) {
          xv[u][m][0] = m < rows ? *(const bf16x8_t*)(x + m * ldx + k) : bf16x8_t{};
          xv[u][m][1] = m < rows ? *(const bf16x8_t*)(x + m * ldx + k + 8) : bf16x8_t{};
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + u * GEMV8_CHUNK + lane * 16;
      if (k < K) {
        const unsigned word[4] = {qv[u].x, qv[u].y, qv[u].z, qv[u].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // word j holds columns k + 4 j .. k + 4 j + 3
          const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8(word[j], false);
          const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8(word[j], true);
          const float we[4] = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int e = 4 * j + c;
#pragma unroll
            for (int m = 0; m < M; ++m) acc[m] += we[c] * bf2f((u16)xv[u][m][e >> 3][e & 7]);
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
    v = __fmul_rn(scale[n], v);  // one rounding of its own; a zero row (scale 0) gives act(bias)
    v += bias ? bias[n] : 0.f;
    v = act_fwd(v, act);
    if constexpr (OUT_F32)
      ((float*)y)[(long)lane * ldy + n] = v;
    else
      ((u16*)y)[(long)lane * ldy + n] = f2bf(v);
  }
}

int gemv_fp8(const uint16_t* x, long ldx, const unsigned char* q, long ldq, const float* scale,
             const float* bias, void* y, long ldy, int M, int N, int K, int act, int out_f32,
             hipStream_t stream) {
  if (M < 1 || M > GEMV_MAX_ROWS || N < 1 || K < 16 || K % 16) return -1;
  if (ldx < K || ldq < K || ldy < N || ldx % 8 || ldq % 16) return -2;
  if (!scale || !y) return -3;
  if ((((uintptr_t)x) | ((uintptr_t)q)) & 15) return -5;
  const dim3 grid((N + GEMV8_WAVES - 1) / GEMV8_WAVES), block(256);
#define DNN_GEMV8(MM, UU)                                                                     \
  if (out_f32)                                                                                \
    hipLaunchKernelGGL((gemv_fp8_kernel<MM, UU, true>), grid, block, 0, stream, x, ldx, q,    \
                       ldq, scale, bias, y, ldy, M, N, K, act);                               \
  else                                                                                        \
    hipLaunchKernelGGL((gemv_fp8_kernel<MM, UU, false>), grid, block, 0, stream, x, ldx, q,   \
                       ldq, scale, bias, y, ldy, M, N, K, act);
  switch (M) {
    case 1: DNN_GEMV8(1, 4) break;
    case 2: DNN_GEMV8(2, 4) break;
    case 3:  // rows 3..4 on the 4-row kernel, 5..8 on the 8-row one (guarded by `rows`)
    case 4: DNN_GEMV8(4, 2) break;
    default: DNN_GEMV8(8, 2) break;
  }
#undef DNN_GEMV8
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

}  // namespace dnn
