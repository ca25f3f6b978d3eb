// Forward layer over fp8 weight rows for more rows than the GEMV takes (serving buckets 64 ..):
//   y[m][n] = act(fl32(scale[n] * S[m][n]) + b[n]),  S[m][n] = sum_k x[m][k] * e4m3(q[n][k]),
// the definition of gemv_fp8.hip for any M >= 1, with the products on v_mfma_f32_16x16x32_bf16.
// The weight operand IS the codes: no bf16 copy of W is written anywhere.
//
// Structure (BM / 16 waves: 4 for the 64-row tile, 8 for the 128-row one; grid
// (ceil(N / BN), ceil(M / BM))):
//   * a wave owns 16 output neurons. Lane (i = lane & 15, g = lane >> 4) reads the 16 codes
//     q[n0 + i][k + 16 g .. + 15] with one 16-byte load straight into registers (a weight row is
//     used by this wave only, so LDS buys nothing for it); a k-step is therefore 64 columns.
//     The loads of 4 stages (512 columns: 8 k-steps = 8 KiB per wave without the K split, 4 with
//     it) are in flight ahead of their use, in a register ring that the k loop, unrolled by one
//     ring, indexes statically;
//   * the codes are decoded by the hardware conversion (v_cvt_pk_f32_fp8: OCP on gfx950, 0x7F /
//     0xFF give NaN). An e4m3 value has 4 significant bits, so the high half of its fp32 form is
//     its bf16 form exactly: one v_perm_b32 packs two of them, no rounding, no table. Codes
//     0..7 of the lane make the A fragment of one MFMA, codes 8..15 that of a second one;
//   * the x tile [BM][128 columns] is what the waves share: global_load -> registers -> ds_write
//     into one of two LDS buffers, one barrier per stage. Loads complete in issue order, so x is
//     fetched as far ahead as the codes (4 stages, 4 x 16 bytes per thread each): waiting for a
//     nearer stage of x would wait for every code load issued before it. A 16-byte chunk c of
//     row r sits at chunk c ^ (r & 15) of its 256-byte LDS row, so the 16 lanes of a
//     ds_read_b128 hit 16 different bank groups. Lane (i, g) reads x[16 f + i][k + 16 g .. + 15]
//     (32 bytes): slot 8 g + j of the first MFMA is column k + 16 g + j on both operands, of the
//     second k + 16 g + 8 + j;
//   * no branch and no select in the k loop: every load is unconditional from a clamped address
//     and columns past K become zeros where x is written to LDS (see load_w). With either, the
//     compiler waited for ALL outstanding loads once per loop trip; without, its counters are
//     exact (s_waitcnt vmcnt(19) / (23) with 24 loads in flight);
//   * SWAPPED operands, mfma(W fragment, x fragment) (mlp_tail.hip): a lane holds 4 consecutive
//     output features n0 + 4 g .. + 3 of ONE data row 16 f + i, so scale and bias are loaded
//     once per lane and a row's 4 values leave in one 16-byte (fp32) or 8-byte (bf16) store
//     (element stores where y's leading dimension or base does not allow it, and at the N edge);
//   * epilogue: __fmul_rn(scale, S) (a rounding of its own, not fused), + bias, act_fwd, store.
//
// Tiles, chosen in the launcher by M and N (BM x BN):
//   * wide, BN = BM: every wave sweeps all of K. Narrow, BN = BM / 2: a 2-way K split INSIDE
//     the workgroup -- the first half of the waves takes the first 64 columns of every stage,
//     the second half the other 64; the second half's accumulators go through LDS and are added
//     to the first's, (first) + (second), before the epilogue. No split through global memory,
//     no atomics: the summation order is fixed by (M, N, K).
//   * 64-row tiles while ceil(N / 64) ceil(M / 64) <= 256 (at most one 64 x 64 workgroup per
//     CU), or M <= 64; else 128-row tiles, which fetch W once per 128 rows. Then the wide tile
//     if it gives >= 256 workgroups, else the narrow one. An 8192-wide layer runs 64 rows on
//     256 workgroups of 64 x 32, 128 rows on 256 of 64 x 64, 256 rows on 256 of 128 x 64 and 512
//     on 256 of 128 x 128. This rule picks the fastest of the four tiles at every point of
//     bench/linear_fp8_bench.py --tiles 1,2,3,4 (both layers, rows 64 .. 1024).
// Longest accumulation chain: one accumulator takes 2 MFMAs (32 products each) per 64 columns,
// so 64 ceil(K / 64) additions, + 1 for the K split.
//
// Registers (hipcc -O3 for gfx950, kernel-resource-usage remark; ScratchSize 0 and no spill in
// every instantiation; fp32 and bf16 output are the same):
//   BM x BN     K split   waves/WG   VGPRs   AGPRs   LDS bytes   waves/SIMD (remark)
//   64 x 64       no          4       144      16      32768         3
//   64 x 32       yes         4       128      16      32768         3
//   128 x 128     no          8       174       0      65536         2
//   128 x 64      yes         8       154       0      65536         3
// Measured and not kept (8192 x 8192 cold, 64 rows, 32 us = 2.0 TB/s of codes, so not yet the
// bytes of W): 8 stages in flight on the 64-row tiles (240 VGPRs; no faster), each workgroup
// starting its K sweep at a stage of its own (no faster at 64 .. 256 rows, 10 % slower at 512
// and 1024), letting ALU / MFMA / LDS reads cross the k-step scheduling barriers (spills 20
// bytes on 128 x 128). At these grids a SIMD holds one wave, and its LDS read -> MFMA waits are
// not covered by another wave: the open lever.
#include "common.hpp"
#include "linear_fp8.hpp"

namespace dnn {

constexpr int LF8_BK = 128;    // columns of x per LDS stage
constexpr int LF8_KSTEP = 64;  // columns per wave k-step: 4 lane groups x 16 codes, two MFMAs
constexpr int LF8_XD = 4;      // stages of x (and of codes) in flight in registers
constexpr int LF8_ROWB = LF8_BK * 2;  // bytes of an LDS row
constexpr int LF8_CUS = 256;   // CUs of an MI355X: the narrow tile is taken below one WG per CU

typedef float lf8_f32x2_t __attribute__((ext_vector_type(2)));

// bf16 pair {lo, hi} from two fp32 whose low halves are zero (decoded e4m3): the high halves.
__device__ __forceinline__ unsigned lf8_pack(float lo, float hi) {
  return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u);
}

// 8 codes (two words) -> the bf16x8 MFMA fragment, element j = code j
__device__ __forceinline__ bf16x8_t lf8_decode8(unsigned w0, unsigned w1) {
  const lf8_f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8(w0, false);
  const lf8_f32x2_t b = __builtin_amdgcn_cvt_pk_f32_fp8(w0, true);
  const lf8_f32x2_t c = __builtin_amdgcn_cvt_pk_f32_fp8(w1, false);
  const lf8_f32x2_t d = __builtin_amdgcn_cvt_pk_f32_fp8(w1, true);
  return __builtin_bit_cast(bf16x8_t, make_uint4(lf8_pack(a[0], a[1]), lf8_pack(b[0], b[1]),
                                                 lf8_pack(c[0], c[1]), lf8_pack(d[0], d[1])));
}

// BM = rows of the x tile, 16 per wave: 64 (4 waves) or 128 (8 waves); KS = groups of waves that
// split a stage's columns (1, 2).
template <int BM, int KS, bool OUT_F32>
__global__ __launch_bounds__(BM * 4) void linear_fp8_kernel(
    const u16* __restrict__ x, long ldx, const unsigned char* __restrict__ q, long ldq,
    const float* __restrict__ scale, const float* __restrict__ bias, void* __restrict__ y,
    long ldy, int M, int N, int K, int act, int vec) {
  constexpr int NT = BM * 4;                     // threads
  constexpr int WN = NT / 64 / KS;               // neuron groups of 16 per workgroup
  constexpr int FM = BM / 16;                    // accumulators (16-row blocks) per wave
  constexpr int NS = LF8_BK / (LF8_KSTEP * KS);  // k-steps of a wave per stage: 2 or 1
  constexpr int U = LF8_XD * NS;                 // k-steps of code loads in flight per wave
  constexpr int XJ = BM * (LF8_BK / 8) / NT;     // 16-byte chunks of x per thread and stage: 4
  constexpr int STAGE = BM * LF8_ROWB;
  static_assert(LF8_XD % 2 == 0, "the LDS buffer of a ring slot is fixed");
  static_assert((NT / 16) % 16 == 0, "a thread's x rows share row & 15");
  static_assert(WN * FM * 1024 <= 2 * STAGE, "K-split reduction fits the x buffers");
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int wn = wave % WN, ks = wave / WN;
  const int m0 = blockIdx.y * BM;
  const int n0 = (blockIdx.x * WN + wn) * 16;
  const bool wlive = n0 < N;  // false: this wave stores nothing
  const unsigned char* qr = q + (long)min(n0 + i, N - 1) * ldq;
  // stages, rounded up to whole trips of the unrolled loop (the extra ones are zeros x zeros)
  const int S = (K + LF8_BK * LF8_XD - 1) / (LF8_BK * LF8_XD) * LF8_XD;
  const int T = S * NS;  // k-steps of this wave
  auto stage_k = [&](int s) { return s * LF8_BK; };  // first column of stage s

  // Every load is unconditional from a clamped (valid) address: a branch around a load makes
  // the compiler wait for ALL loads at every use, and so does a select on the loaded value that
  // it is free to hoist. What is outside the operands is made harmless where x is written to
  // LDS: columns past K are zeros there, so the codes a lane re-reads for them (K % 16 == 0:
  // its 16 columns are inside K or wholly outside, where it takes the row's last 16) meet
  // zeros; rows past M and neurons past N (row M - 1 / N - 1 re-read) only reach outputs that
  // are never stored. (A re-read NaN code times zero is NaN, in a neuron whose real last 16
  // codes hold that NaN: its outputs are NaN by definition.)
  auto load_w = [&](int t) {
    const int k = stage_k(t / NS) + (ks * NS + t % NS) * LF8_KSTEP + 16 * g;
    return *(const uint4*)(qr + min(k, K - 16));
  };
  // x chunks of a stage: thread -> rows (tid >> 4) + (NT / 16) j, chunk tid & 15
  const int xrow = tid >> 4, xch = tid & 15;
  auto load_x = [&](int s, uint4 (&xr)[XJ]) {
    const int k = min(stage_k(s) + xch * 8, K - 8);
#pragma unroll
    for (int j = 0; j < XJ; ++j)
      xr[j] = *(const uint4*)(x + (long)min(m0 + xrow + (NT / 16) * j, M - 1) * ldx + k);
  };
  auto store_x = [&](int s, char* buf, const uint4 (&xr)[XJ]) {
    const bool in = stage_k(s) + xch * 8 < K;
#pragma unroll
    for (int j = 0; j < XJ; ++j) {
      const int r = xrow + (NT / 16) * j;  // r & 15 == xrow & 15
      *(uint4*)(buf + r * LF8_ROWB + ((xch ^ (xrow & 15)) << 4)) =
          make_uint4(in ? xr[j].x : 0u, in ? xr[j].y : 0u, in ? xr[j].z : 0u, in ? xr[j].w : 0u);
    }
  };

  f32x4_t acc[FM];
#pragma unroll
  for (int f = 0; f < FM; ++f) acc[f] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  // Loads complete in issue order, so waiting for a stage of x also waits for every code load
  // issued before it: x is therefore fetched as far ahead as the codes (LF8_XD stages = U
  // k-steps), each stage of x issued just before the codes of its own k-steps.
  uint4 xq[LF8_XD][XJ];
  uint4 wq[U];
#pragma unroll
  for (int d = 0; d < LF8_XD; ++d) {
    load_x(d, xq[d]);
#pragma unroll
    for (int e = 0; e < NS; ++e) wq[d * NS + e] = load_w(d * NS + e);
    __builtin_amdgcn_sched_barrier(0);  // keep the issue order of the loop
  }

  for (int t0 = 0; t0 < T; t0 += U) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      __builtin_amdgcn_sched_barrier(0);  // nothing moves across k-steps: loads keep their order
      const int t = t0 + u;
      const int s = t / NS;  // stage; its ring slot is u / NS, its LDS buffer (u / NS) & 1
      char* buf = lds + ((u / NS) & 1) * STAGE;
      if (u % NS == 0) {  // first k-step of the stage (compile time)
        // this buffer was last read in stage s - 2, which every wave left before it passed
        // the barrier of stage s - 1
        store_x(s, buf, xq[u / NS]);
        __syncthreads();
        load_x(s + LF8_XD, xq[u / NS]);
      }
      // decode, then refill the slot: the new load can take the registers it frees (a load
      // into other registers has to be copied into the ring at the loop's end, after a wait)
      const bf16x8_t a0 = lf8_decode8(wq[u].x, wq[u].y), a1 = lf8_decode8(wq[u].z, wq[u].w);
      wq[u] = load_w(t + U);
      const int ch = (ks * NS + u % NS) * 8 + 2 * g;  // the lane's first x chunk of the k-step
#pragma unroll
      for (int f = 0; f < FM; ++f) {
        const char* row = buf + (16 * f + i) * LF8_ROWB;
        const bf16x8_t b0 = *(const bf16x8_t*)(row + ((ch ^ i) << 4));
        const bf16x8_t b1 = *(const bf16x8_t*)(row + (((ch + 1) ^ i) << 4));
        acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[f], 0, 0, 0);
        acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc[f], 0, 0, 0);
      }
    }
  }

  if constexpr (KS > 1) {  // fixed order: (columns of the first wave group) + (of the second)
    __syncthreads();       // the x buffers are free
    f32x4_t* red = (f32x4_t*)lds + (wn * FM) * 64 + lane;
    if (ks == 1) {
#pragma unroll
      for (int f = 0; f < FM; ++f) red[f * 64] = acc[f];
    }
    __syncthreads();
    if (ks == 1) return;
#pragma unroll
    for (int f = 0; f < FM; ++f) acc[f] += red[f * 64];
  }
  if (!wlive) return;

  const int n = n0 + 4 * g;  // this lane's 4 output features
  float sc[4], bi[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    sc[r] = n + r < N ? scale[n + r] : 0.f;
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
      float z = __fmul_rn(sc[r], acc[f][r]);  // one rounding of its own; scale 0 gives act(bias)
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

int linear_fp8(const uint16_t* x, long ldx, const unsigned char* q, long ldq, const float* scale,
               const float* bias, void* y, long ldy, int M, int N, int K, int act, int out_f32,
               int tile, hipStream_t stream) {
  if (M < 1 || N < 1 || K < 16 || K % 16) return -1;
  if (ldx < K || ldq < K || ldy < N || ldx % 8 || ldq % 16) return -2;
  if (!x || !q || !scale || !y) return -3;
  if (act != ACT_LINEAR && act != ACT_RELU && act != ACT_SIGMOID) return -4;
  if ((((uintptr_t)x) | ((uintptr_t)q)) & 15) return -5;
  const int esz = out_f32 ? 4 : 2;
  if (((uintptr_t)y) % esz) return -6;
  if (tile < 0 || tile > 4) return -8;
  // Tile choice (measured: header). 64-row tiles while they give at most one workgroup per CU
  // at BN = 64; past that the 128-row tiles, which fetch W once per 128 rows. Then the wide
  // tile (BN = BM) if it still gives a workgroup per CU, else the narrow one with the K split.
  int bm = (M <= 64 || ((long)(N + 63) / 64) * ((M + 63) / 64) <= LF8_CUS) ? 64 : 128;
  if (tile) bm = tile <= 2 ? 64 : 128;
  const long tiles_m = ((long)M + bm - 1) / bm;
  if (tiles_m > 65535) return -7;
  // 4 consecutive outputs of a row in one store: every row's n0 + 4 g must be 4-element aligned
  const int vec = ldy % 4 == 0 && ((uintptr_t)y) % (4 * esz) == 0;
  bool wide = ((long)(N + bm - 1) / bm) * tiles_m >= LF8_CUS;
  if (tile) wide = tile & 1;
  const int bn = wide ? bm : bm / 2;
  const dim3 grid((N + bn - 1) / bn, (unsigned)tiles_m), block(bm * 4);
#define DNN_LF8(BM_, KS_)                                                                      \
  if (out_f32)                                                                                 \
    hipLaunchKernelGGL((linear_fp8_kernel<BM_, KS_, true>), grid, block, 0, stream, x, ldx, q, \
                       ldq, scale, bias, y, ldy, M, N, K, act, vec);                           \
  else                                                                                         \
    hipLaunchKernelGGL((linear_fp8_kernel<BM_, KS_, false>), grid, block, 0, stream, x, ldx,   \
                       q, ldq, scale, bias, y, ldy, M, N, K, act, vec);
  if (bm == 64) {
    if (wide) { DNN_LF8(64, 1) } else { DNN_LF8(64, 2) }
  } else {
    if (wide) { DNN_LF8(128, 1) } else { DNN_LF8(128, 2) }
  }
#undef DNN_LF8
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

}  // namespace dnn
