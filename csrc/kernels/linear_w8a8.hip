// Forward layer with e4m3 codes on both operands (w8a8), for the serving buckets over 8 rows:
//   y[m][n] = act(fl32(sx[m] * fl32(sw[n] * S[m][n])) + b[n]),
//   S[m][n] = sum_k e4m3(xq[m][k]) * e4m3(q[n][k]),
// xq / sx the rows of quant_rows_fp8 (elementwise.hip), q / sw the fp8 weight rows of the same
// format. The products run on v_mfma_scale_f32_16x16x128_f8f6f4, which takes the codes of both
// operands undecoded (cbsz = blgp = 0: e4m3 on A and B) at twice the bf16 MFMA rate; its block
// scales are the constant E8M0 1.0 (0x7F in every byte, op_sel 0) -- the real scales are fp32,
// one per data row and one per neuron, and are applied once per output in the epilogue.
//
// Structure (linear_fp8.hip's, without the decode; 4 waves, grid (ceil(N / BN), ceil(M / BM))):
//   * a wave owns NG groups of 16 output neurons (BN = 64 NG). For each group lane (i = lane &
//     15, g = lane >> 4) reads the 32 codes q[n0 + i][k + 32 g .. + 31] with two 16-byte loads
//     straight into registers: they ARE the A fragment (8 VGPRs) of one MFMA, so a k-step is
//     128 columns = one MFMA per (neuron group, 16-row block). The loads of 4 stages (512
//     columns) are in flight ahead of their use in a register ring that the k loop, unrolled by
//     one ring, indexes statically;
//   * the x tile [BM][128 columns], one byte per element, is what the waves share: global_load
//     -> registers -> ds_write into one of two LDS buffers, one barrier per stage, x fetched as
//     far ahead as the codes (loads complete in issue order). A 16-byte chunk c of row r sits at
//     chunk c ^ ((r >> 1) & 7) of its 128-byte LDS row: two rows fill the 64 banks, and the 16
//     lanes i of a ds_read_b128 (rows 16 f + i, one chunk) then hit 16 different bank groups.
//     Lane (i, g) reads x[16 f + i][k + 32 g .. + 31] (chunks 2 g, 2 g + 1): the B fragment,
//     read once and used by the wave's NG MFMAs. Both operands give lane (i, g) the same 32
//     columns in the same order, so slot j of a lane is the same column on both sides whatever
//     the instruction's internal k map (the exact-sum test establishes the rest of the map);
//   * no branch and no select in the k loop: every load is unconditional from a clamped address
//     and columns past K become zeros where x is written to LDS;
//   * SWAPPED operands, mfma(W fragment, x fragment): a lane holds 4 consecutive output
//     features n0 + 4 g .. + 3 of ONE data row 16 f + i, so a row's 4 values leave in one
//     16-byte (fp32) or 8-byte (bf16) store (element stores where y's leading dimension or base
//     does not allow it, and at the N edge);
//   * epilogue: __fmul_rn(sx, __fmul_rn(sw, S)) (two roundings of their own, weight scale
//     first, nothing fused), + bias, act_fwd, store.
// No atomics and no split of K anywhere: the summation order is fixed by (M, N, K, tile).
//
// Tiles (BM x BN; tile = 1, 2), chosen in the launcher by M and N: 64 x 64 (NG = 1) while
// ceil(N / 64) ceil(M / 64) <= 512 (at most two of its workgroups per CU), or M <= 64; else 128 x
// 128 (NG = 2), which fetches W once per 128 rows and reads an x fragment from LDS once per two
// MFMAs. Measured (bench/linear_fp8_bench.py --w8a8-tiles 1,2, graph replay, the GEMM alone):
// this picks the faster tile at every point of both layers, rows 64 .. 65536 -- on 8192 x 8192
// read cold 27 / 27 / 46 us at 64 / 128 / 256 rows against 47 / 52 / 52 for 128 x 128, then 53
// us at 512 rows against 85 for 64 x 64 and 1.4 ms at 16384 rows against 2.4; on the resident
// 1024 x 1024 layer 64 x 64 up to 2048 rows (10.2 against 14.6 us), 128 x 128 from 4096 (16.1
// against 17.9) (profiles/linear_w8a8/).
// Longest accumulation chain: one accumulator takes one MFMA (128 products) per 128 columns, so
// 128 ceil(K / 128) additions, the same for every tile.
//
// Registers (hipcc -O3 for gfx950, kernel-resource-usage remark; ScratchSize 0 and no spill in
// every instantiation; fp32 and bf16 output are the same):
//   tile   BM x BN     NG   waves/WG   VGPRs   AGPRs   LDS bytes   waves/SIMD (remark)
//    1     64 x 64      1      4         98      16      16384         4
//    2     128 x 128    2      4        170      64      32768         2
// The k loop's load counters are exact (tile 1: s_waitcnt vmcnt(15) / (14) / (12) with 16 loads
// in flight) because a slot of codes is refilled AFTER its MFMAs: the codes are the A fragments
// themselves, and a refill before them goes to other registers that the compiler copies into
// the ring at the loop's end behind a wait that drains it.
// Measured and not kept: a 128 x 256 tile (NG = 4, 2 stages in flight; 166 VGPRs + 128 AGPRs, one
// wave per SIMD). On 8192 x 8192 it was within 3 % of 128 x 128 from 1024 rows up (ahead by more
// than the spreads at 1024 rows only, 91.6 against 94.0 us), on 1024 x 1024 9 - 16 % slower at
// 16384 and 65536 rows: at these sizes the LDS reads of x are not what bounds the kernel.
#include "common.hpp"
#include "linear_w8a8.hpp"

namespace dnn {

constexpr int LW8_BK = 128;  // columns per stage = per k-step = per MFMA; bytes of an LDS row
constexpr int LW8_NT = 256;  // threads: 4 waves
constexpr int LW8_XD = 4;    // stages of x and of codes in flight in registers
constexpr int LW8_CUS = 256;  // CUs of an MI355X
constexpr int LW8_ONE = 0x7F7F7F7F;  // E8M0 1.0 in every byte: the MFMA's block scales

typedef int lw8_i32x4_t __attribute__((ext_vector_type(4)));
typedef int lw8_i32x8_t __attribute__((ext_vector_type(8)));

// 2 x 16 codes -> the 32-code MFMA fragment (8 VGPRs), slot j = code j
__device__ __forceinline__ lw8_i32x8_t lw8_frag(lw8_i32x4_t lo, lw8_i32x4_t hi) {
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// BM = rows of the x tile (FM = BM / 16 row blocks per wave); NG = groups of 16 neurons per wave.
template <int BM, int NG, bool OUT_F32>
__global__ __launch_bounds__(LW8_NT) void linear_w8a8_kernel(
    const unsigned char* __restrict__ xq, long ldxq, const float* __restrict__ sx,
    const unsigned char* __restrict__ q, long ldq, const float* __restrict__ sw,
    const float* __restrict__ bias, void* __restrict__ y, long ldy, int M, int N, int K, int act,
    int vec) {
  constexpr int FM = BM / 16;                    // 16-row blocks (accumulators per neuron group)
  constexpr int XJ = BM * (LW8_BK / 16) / LW8_NT;  // 16-byte chunks of x per thread and stage
  constexpr int XR = LW8_NT / 8;                 // rows between a thread's chunks: 32
  constexpr int STAGE = BM * LW8_BK;
  constexpr int XD = LW8_XD;
  static_assert(XD % 2 == 0, "the LDS buffer of a ring slot is fixed");
  static_assert(XJ >= 1 && (XR / 2) % 8 == 0, "a thread's x rows share (row >> 1) & 7");
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.y * BM;
  const int n0 = (blockIdx.x * 4 + wave) * NG * 16;  // the wave's first neuron
  const unsigned char* qr[NG];
#pragma unroll
  for (int e = 0; e < NG; ++e) qr[e] = q + (long)min(n0 + 16 * e + i, N - 1) * ldq;
  // stages, rounded up to whole trips of the unrolled loop (the extra ones are zeros x zeros)
  const int S = (K + LW8_BK * XD - 1) / (LW8_BK * XD) * XD;

  // Every load is unconditional from a clamped (valid) address (linear_fp8.hip: a branch or a
  // select around a load makes the compiler wait for ALL loads at every use). What is outside
  // the operands is made harmless where x is written to LDS: columns past K are zeros there,
  // so the codes a lane re-reads for them (K % 16 == 0: each 16-byte half of its 32 columns is
  // inside K or wholly outside, where it takes the row's last 16) meet zeros; rows past M and
  // neurons past N (row M - 1 / N - 1 re-read) only reach outputs that are never stored. (A
  // re-read NaN code times zero is NaN, in a neuron whose real last 16 codes hold that NaN:
  // its outputs are NaN by definition.)
  auto load_w = [&](int s, lw8_i32x4_t (&wr)[NG][2]) {
    const int k = s * LW8_BK + 32 * g;
#pragma unroll
    for (int e = 0; e < NG; ++e) {
      wr[e][0] = *(const lw8_i32x4_t*)(qr[e] + min(k, K - 16));
      wr[e][1] = *(const lw8_i32x4_t*)(qr[e] + min(k + 16, K - 16));
    }
  };
  // x chunks of a stage: thread -> rows (tid >> 3) + 32 j, chunk tid & 7
  const int xrow = tid >> 3, xch = tid & 7;
  const int xsw = (xch ^ ((xrow >> 1) & 7)) << 4;  // the same for all of the thread's rows
  auto load_x = [&](int s, uint4 (&xr)[XJ]) {
    const int k = min(s * LW8_BK + xch * 16, K - 16);
#pragma unroll
    for (int j = 0; j < XJ; ++j)
      xr[j] = *(const uint4*)(xq + (long)min(m0 + xrow + XR * j, M - 1) * ldxq + k);
  };
  auto store_x = [&](int s, char* buf, const uint4 (&xr)[XJ]) {
    const bool in = s * LW8_BK + xch * 16 < K;
#pragma unroll
    for (int j = 0; j < XJ; ++j)
      *(uint4*)(buf + (xrow + XR * j) * LW8_BK + xsw) =
          make_uint4(in ? xr[j].x : 0u, in ? xr[j].y : 0u, in ? xr[j].z : 0u, in ? xr[j].w : 0u);
  };

  f32x4_t acc[NG][FM];
#pragma unroll
  for (int e = 0; e < NG; ++e)
#pragma unroll
    for (int f = 0; f < FM; ++f) acc[e][f] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  uint4 xr[XD][XJ];
  lw8_i32x4_t wr[XD][NG][2];
#pragma unroll
  for (int d = 0; d < XD; ++d) {
    load_x(d, xr[d]);
    load_w(d, wr[d]);
    __builtin_amdgcn_sched_barrier(0);  // keep the issue order of the loop
  }

  // the lane's two x chunks of a k-step, swizzled: (16 f + i) >> 1 & 7 == (i >> 1) & 7
  const int rsw0 = ((2 * g) ^ ((i >> 1) & 7)) << 4, rsw1 = ((2 * g + 1) ^ ((i >> 1) & 7)) << 4;
  for (int s0 = 0; s0 < S; s0 += XD) {
#pragma unroll
    for (int u = 0; u < XD; ++u) {
      __builtin_amdgcn_sched_barrier(0);  // nothing moves across k-steps: loads keep their order
      const int s = s0 + u;  // stage; its ring slot is u, its LDS buffer u & 1
      char* buf = lds + (u & 1) * STAGE;
      // this buffer was last read in stage s - 2, which every wave left before it passed the
      // barrier of stage s - 1
      store_x(s, buf, xr[u]);
      __syncthreads();
      load_x(s + XD, xr[u]);
      lw8_i32x8_t a[NG];
#pragma unroll
      for (int e = 0; e < NG; ++e) a[e] = lw8_frag(wr[u][e][0], wr[u][e][1]);
#pragma unroll
      for (int f = 0; f < FM; ++f) {
        const char* row = buf + (16 * f + i) * LW8_BK;
        const lw8_i32x8_t b = lw8_frag(*(const lw8_i32x4_t*)(row + rsw0),
                                       *(const lw8_i32x4_t*)(row + rsw1));
#pragma unroll
        for (int e = 0; e < NG; ++e)
          acc[e][f] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              a[e], b, acc[e][f], 0, 0, 0, LW8_ONE, 0, LW8_ONE);
      }
      // refill the slot after its MFMAs: the codes ARE the A fragments, so only now can the new
      // loads take the same registers (a load into other registers has to be copied into the
      // ring at the loop's end, after a wait that drains the ring)
      load_w(s + XD, wr[u]);
    }
  }

  float sxm[FM];
#pragma unroll
  for (int f = 0; f < FM; ++f) sxm[f] = sx[min(m0 + 16 * f + i, M - 1)];
#pragma unroll
  for (int e = 0; e < NG; ++e) {
    const int n = n0 + 16 * e + 4 * g;  // this lane's 4 output features of the group
    if (n0 + 16 * e >= N) break;        // (wave-uniform) the group stores nothing
    float sc[4], bi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sc[r] = n + r < N ? sw[n + r] : 0.f;
      bi[r] = (bias && n + r < N) ? bias[n + r] : 0.f;
    }
    const bool whole = vec && n + 3 < N;
#pragma unroll
    for (int f = 0; f < FM; ++f) {
      const int m = m0 + 16 * f + i;
      if (m >= M) continue;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // two roundings of their own; a zero scale on either side gives act(bias)
        float z = __fmul_rn(sxm[f], __fmul_rn(sc[r], acc[e][f][r]));
        z += bi[r];
        v[r] = act_fwd(z, act);
      }
      if constexpr (OUT_F32) {
        float* o = (float*)y + (long)m * ldy + n;
        if (whole) {
          *(f32x4_t*)o = f32x4_t{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n + r < N) o[r] = v[r];
        }
      } else {
        u16* o = (u16*)y + (long)m * ldy + n;
        if (whole) {
          bf16x4_t p;
#pragma unroll
          for (int r = 0; r < 4; ++r) p[r] = (short)f2bf(v[r]);
          *(bf16x4_t*)o = p;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n + r < N) o[r] = f2bf(v[r]);
        }
      }
    }
  }
}

int linear_w8a8(const unsigned char* xq, long ldxq, const float* sx, const unsigned char* q,
                long ldq, const float* sw, const float* bias, void* y, long ldy, int M, int N,
                int K, int act, int out_f32, int tile, hipStream_t stream) {
  if (M < 1 || N < 1 || K < 16 || K % 16) return -1;
  if (ldxq < K || ldq < K || ldy < N || ldxq % 16 || ldq % 16) return -2;
  if (!xq || !sx || !q || !sw || !y) return -3;
  if (act != ACT_LINEAR && act != ACT_RELU && act != ACT_SIGMOID) return -4;
  if ((((uintptr_t)xq) | ((uintptr_t)q)) & 15) return -5;
  const int esz = out_f32 ? 4 : 2;
  if (((uintptr_t)y) % esz) return -6;
  if (tile < 0 || tile > LINEAR_W8A8_TILES) return -8;
  // Tile choice (measured: header): 64 x 64 while it gives at most two workgroups per CU.
  const long wg64 = ((long)(N + 63) / 64) * (((long)M + 63) / 64);
  if (!tile) tile = (M <= 64 || wg64 <= 2 * LW8_CUS) ? 1 : 2;
  const int bm = tile == 1 ? 64 : 128, bn = bm;
  const long tiles_m = ((long)M + bm - 1) / bm;
  if (tiles_m > 65535) return -7;
  // 4 consecutive outputs of a row in one store: every row's n0 + 4 g must be 4-element aligned
  const int vec = ldy % 4 == 0 && ((uintptr_t)y) % (4 * esz) == 0;
  const dim3 grid((N + bn - 1) / bn, (unsigned)tiles_m), block(LW8_NT);
#define DNN_LW8(BM_, NG_)                                                                     \
  if (out_f32)                                                                                \
    hipLaunchKernelGGL((linear_w8a8_kernel<BM_, NG_, true>), grid, block, 0, stream, xq, ldxq, \
                       sx, q, ldq, sw, bias, y, ldy, M, N, K, act, vec);                      \
  else                                                                                        \
    hipLaunchKernelGGL((linear_w8a8_kernel<BM_, NG_, false>), grid, block, 0, stream, xq,     \
                       ldxq, sx, q, ldq, sw, bias, y, ldy, M, N, K, act, vec);
  if (tile == 1) { DNN_LW8(64, 1) } else { DNN_LW8(128, 2) }
#undef DNN_LW8
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

}  // namespace dnn
