// MXFP4 weight rows (mxfp4.hpp has the format): the quantiser that runs once per layer at load
// and the dequantiser that a bucket of more than GEMV_MAX_ROWS rows runs per layer into the
// serving stage's bf16 scratch. Both are memory-bound and row-parallel: one wave per row, one
// LANE per 32-column block, so a block's amax and scale need no cross-lane traffic. A lane moves
// its block with 16-byte accesses only: four loads of bf16 and one store of codes in the
// quantiser, one load of codes and four stores of bf16 in the dequantiser, plus the scale byte.
//
// The arithmetic is on the bf16 bit fields and exact, so both kernels equal the oracle bit for
// bit: t = x * 2^(127 - E) is the value 1.m * 2^(ef - E) (ef = exponent field of x, at most
// E + 2), rebuilt as an fp32 and compared with the seven midpoints; the comparison is strict
// where the tie goes down to the even code (0.25, 1.25, 2.5, 5) and inclusive where it goes up
// (0.75, 1.75, 3.5). Anything above 5, the saturating interval (6, 8) included, is code 7. The
// hardware conversion v_cvt_scalef32_pk_fp4_bf16 is not used: it has not been compared with the
// oracle on every bf16 value, and this kernel runs once per layer.
#include "common.hpp"
#include "mxfp4.hpp"

namespace dnn {

// 4-bit code of the bf16 bits b in a block of scale byte E (>= 15).
__device__ __forceinline__ unsigned mxfp4_code(unsigned b, int E) {
  const unsigned sign = (b >> 12) & 8u;
  const int d = (int)((b >> 7) & 0xFFu) - E;  // t = 1.m * 2^d, d <= 2
  if (d < -3) return sign;  // t < 2^-2 (bf16 subnormals too: their field is 0): magnitude 0
  const float t = __uint_as_float(((unsigned)(d + 127) << 23) | ((b & 0x7Fu) << 16));
  const unsigned mag = (unsigned)(t > 0.25f) + (unsigned)(t >= 0.75f) + (unsigned)(t > 1.25f) +
                       (unsigned)(t >= 1.75f) + (unsigned)(t > 2.5f) + (unsigned)(t >= 3.5f) +
                       (unsigned)(t > 5.f);
  return sign | mag;
}

__global__ __launch_bounds__(256) void quant_rows_mxfp4_kernel(const u16* __restrict__ x, long ldx,
                                                               int rows, int cols,
                                                               unsigned char* __restrict__ q,
                                                               long ldq,
                                                               unsigned char* __restrict__ e,
                                                               long lde) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform
  const u16* xr = x + (long)row * ldx;
  unsigned char* qr = q + (long)row * ldq;
  unsigned char* er = e + (long)row * lde;
  for (int blk = lane; blk < cols / MXFP4_BLOCK; blk += 64) {
    uint4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = *(const uint4*)(xr + blk * MXFP4_BLOCK + 8 * i);
    const u16* b = (const u16*)v;
    unsigned amax = 0;  // magnitudes of finite bf16 values order like their low 15 bits
#pragma unroll
    for (int k = 0; k < 32; ++k) amax = max(amax, (unsigned)b[k] & 0x7FFFu);
    const int ef = (int)(amax >> 7);
    const bool send = ef >= MXFP4_TINY_EXP_FIELD;  // false for a zero block too
    const int E = send ? ef - 2 : 0;
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (send) {
#pragma unroll
      for (int k = 0; k < 32; ++k) w[k >> 3] |= mxfp4_code(b[k], E) << (4 * (k & 7));
    }
    *(uint4*)(qr + blk * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    er[blk] = (unsigned char)E;
  }
}

// bf16 bits of dec(c) * 2^(E - 127), E >= 1: one fp32 multiply of two exact factors and the
// rounding of f2bf, which changes nothing wherever the product is a bf16 value (every E >= 15).
__device__ __forceinline__ u16 mxfp4_value(unsigned c, float scale) {
  const unsigned m = c & 7u;
  // codes 2..7 are normal, (1 + m / 2) * 2^(ee - 1); 1 is the one subnormal, 0.5
  const float mag = m > 1u ? __uint_as_float(((126u + (m >> 1)) << 23) | ((m & 1u) << 22))
                           : 0.5f * (float)m;
  return (u16)(f2bf(mag * scale) | ((c & 8u) << 12));
}

__global__ __launch_bounds__(256) void dequant_rows_mxfp4_kernel(
    const unsigned char* __restrict__ q, long ldq, const unsigned char* __restrict__ e, long lde,
    int rows, int cols, u16* __restrict__ x, long ldx) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const unsigned char* qr = q + (long)row * ldq;
  const unsigned char* er = e + (long)row * lde;
  u16* xr = x + (long)row * ldx;
  for (int blk = lane; blk < cols / MXFP4_BLOCK; blk += 64) {
    const uint4 c = *(const uint4*)(qr + blk * 16);
    const unsigned E = er[blk];
    const float scale = __uint_as_float(E << 23);
    const unsigned w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // word i holds columns 8 i .. 8 i + 7 of the block
      uint4 out = make_uint4(0u, 0u, 0u, 0u);  // E == 0: +0 whatever the nibbles hold
      if (E) {
        u16* o = (u16*)&out;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = mxfp4_value(w[i] >> (4 * k), scale);
      }
      *(uint4*)(xr + blk * MXFP4_BLOCK + 8 * i) = out;
    }
  }
}

static int mxfp4_check(const void* x, long ldx, int rows, int cols, const void* q, long ldq,
                       const void* e, long lde) {
  if (rows <= 0 || cols <= 0 || cols % MXFP4_BLOCK) return -1;
  if (ldx < cols || ldq < cols / 2 || lde < cols / MXFP4_BLOCK || ldx % 8 || ldq % 16) return -2;
  if (!x || !q || !e) return -3;
  if ((((uintptr_t)x) | ((uintptr_t)q)) & 15) return -5;
  return 0;
}

int quant_rows_mxfp4(const uint16_t* x, long ldx, int rows, int cols, unsigned char* q, long ldq,
                     unsigned char* e, long lde, hipStream_t stream) {
  if (const int rc = mxfp4_check(x, ldx, rows, cols, q, ldq, e, lde)) return rc;
  hipLaunchKernelGGL(quant_rows_mxfp4_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, x, ldx,
                     rows, cols, q, ldq, e, lde);
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

int dequant_rows_mxfp4(const unsigned char* q, long ldq, const unsigned char* e, long lde,
                       int rows, int cols, uint16_t* x, long ldx, hipStream_t stream) {
  if (const int rc = mxfp4_check(x, ldx, rows, cols, q, ldq, e, lde)) return rc;
  hipLaunchKernelGGL(dequant_rows_mxfp4_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, q,
                     ldq, e, lde, rows, cols, x, ldx);
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

}  // namespace dnn
