// Forward layer over bf16 weight rows for serving buckets of 9 .. ~1000 rows:
//   y[m][n] = act(sum_k x[m][k] * w[n][k] + b[n]),
// the definition of gemm.hip's forward, on v_mfma_f32_16x16x32_bf16, built to STREAM W: at these
// row counts a wide layer is bound by the bytes of W, and the training tiles (both operands staged
// through LDS, 128 workgroups of 64 x 64 at 64 rows of an 8192-wide layer) are far from them.
//
// Structure (grid (ceil(N / BN), ceil(M / BM)), 4 or 8 waves):
//   * WEIGHTS NEVER TOUCH LDS. A wave owns 16 output neurons. Lane (i = lane & 15, g = lane >> 4)
//     reads w[n0 + i][c + 8 g .. + 7] with one 16-byte load, and that register IS the A fragment
//     of the MFMA (slot 8 g + j = column c + 8 g + j): no decode, no copy. A k-step is 32
//     columns; a weight row is used by this wave only, so a workgroup reads each weight byte
//     once per row tile;
//   * the loads run ahead in a register ring of LS_RING = 8 k-steps per wave (8 KiB of W per
//     wave, 16 KiB per SIMD where two waves share one: four times what linear_fp8.hip's split
//     tiles keep in flight per SIMD, for a row that is twice the bytes per column). The k loop is
//     unrolled by one ring, so every slot is indexed statically; a slot is refilled right after
//     the MFMAs that read it, into the same registers;
//   * K SPLIT INSIDE THE WORKGROUP, KS = 1, 2 or 4 groups of waves. An LDS stage is 128 columns
//     = 4 k-steps, and the groups take disjoint k-steps of every stage: NS = 4 / KS each. With
//     NS >= 2 a group's k-steps are adjacent, so a wave reads whole 128-byte lines of a weight
//     row with two consecutive loads. With KS = 4 (NS = 1) that is kept by pairing the stages:
//     stages 2 p and 2 p + 1 hold the columns 256 p + 64 q + 32 (s & 1) + [0, 32) of group q,
//     so a group still walks 64 adjacent columns over two consecutive k-steps (stage_col). The
//     groups' accumulators are added through LDS in a fixed order, ((g0 + g1) + g2) + g3, by
//     group 0, which runs the epilogue. No split through global memory, no atomics: the
//     summation order depends on (M, N, K, tile) only, and two runs are bit-identical. The 4-way
//     split on 8 waves was built to test linear_fp8.hip's open lever: at N = 8192 and 64 rows it
//     is 256 workgroups of 64 x 32 with TWO waves on every SIMD, so one wave's LDS read -> MFMA
//     waits could be covered by the other's. Measured, it is SLOWER than the 2-way split with
//     one wave per SIMD (below), so the launcher does not choose it at 64 rows;
//   * the x tile [BM][128 columns] is what the waves share: global_load -> registers ->
//     ds_write_b128 into one of two LDS buffers, one barrier per stage. Loads complete in issue
//     order, so x is fetched as far ahead as the weights (XD = LS_RING / NS stages: waiting for a
//     nearer stage of x would wait for every weight load issued before it). Layout: the XOR
//     chunk swizzle of linear_fp8.hip -- the 16-byte chunk c of row r sits at chunk c ^ (r & 15)
//     of its 256-byte LDS row. It is conflict-free for ds_read_b128 because the 16 lanes i = 0 ..
//     15 of one lane group read the SAME logical chunk 4 j + g of 16 rows whose r & 15 = i are
//     all different: the 16 physical chunks (4 j + g) ^ i are all different, i.e. 16 distinct
//     16-byte bank groups that together cover the 64 banks exactly once. The writes are the
//     mirror image (16 lanes write the 16 chunks of one row);
//   * no branch and no select in the k loop: every load is unconditional from a clamped address,
//     and columns past K become zeros where x is written to LDS (see load_w), so a ring slot past
//     K contributes zeros. That keeps the compiler's s_waitcnt vmcnt counts exact
//     (linear_fp8.hip documents what a branch or a select costs);
//   * SWAPPED operands, mfma(W fragment, x fragment) (linear_fp8.hip, stage_fwd.hip,
//     mlp_tail.hip): a lane holds 4 consecutive output features n0 + 4 g .. + 3 of ONE data row
//     16 f + i, so bias is loaded once per lane and a row's 4 values leave in one 16-byte (fp32)
//     or 8-byte (bf16) store (element stores at the N edge, or where y's leading dimension or
//     base does not allow vectors);
//   * epilogue: + bias, act_fwd, store. Rows past M and neurons past N are never stored.
//
// Tiles (tile = 1 .. LINEAR_STREAM_TILES; BN = 16 * waves / KS):
//   tile   BM x BN     K split   waves   k-steps / wave / stage   stages of x ahead
//    1     64 x 64       no        4              4                      2
//    2     64 x 32      2-way      4              2                      4
//    3     64 x 32      4-way      8              1                      8
//    4    128 x 128      no        8              4                      2
//    5    128 x 64      2-way      8              2                      4
//    6    128 x 32      4-way      8              1                      8
// tile = 0, the launcher's rule (linear_fp8.hip's): 64-row tiles while ceil(N / 64) ceil(M / 64)
// <= 256 (at most one 64 x 64 workgroup per CU) or M <= 64, else 128-row tiles, which fetch W
// once per 128 rows. Then the widest tile that still gives >= 256 workgroups: 64 rows -> 1, else
// 2; 128 rows -> 4, else 5, else 6. An 8192-wide layer runs 64 rows on 256 workgroups of 64 x 32
// (2-way), 128 rows on 256 of 64 x 64, 256 rows on 256 of 128 x 64 and 512 rows on 256 of 128 x
// 128: at each of these points that is the fastest of the six tiles, or within the spread of it
// (bench/linear_stream_bench.py --tiles 1,2,3,4,5,6, 8192 x 8192 cold, us, spreads <= 4.5 %):
//   rows   tile 1   tile 2   tile 3   tile 4   tile 5   tile 6
//    64     56.0     42.2     50.9     90.5     62.7     56.6
//   128     55.1     71.6     91.2    105.9     74.3     72.1
//   256     93.1    126.4    170.9    101.2     74.4    131.6
//   512    173.1    223.0    294.2    103.6    130.8    236.9
// On the resident 1024 x 1024 layer tile 2 is the fastest up to 512 rows too (6.5 - 6.8 us against
// 7.6 - 7.9 for tile 3). The 4-way split with two waves per SIMD loses to the 2-way split with
// one at 64 rows on both layers (50.9 against 42.2 us, 7.6 against 6.5): it pays one workgroup
// barrier of 8 waves per 4 MFMAs of a wave and a 3-step reduction, and the second wave's cover
// of the LDS read -> MFMA waits does not buy that back. The one-wave-per-SIMD diagnosis of
// linear_fp8.hip is not confirmed by this kernel. Tile 3 stays as a forced tile for the
// benchmark and the tests; tile 6 is the rule's narrow end of the 128-row tiles (65 .. 128 rows
// of a layer between 8192 and 16320 wide), where it measured level with tile 5 (72.1 against
// 74.3 us at 128 rows above).
// Longest accumulation chain: one accumulator takes one MFMA (32 products) per k-step of its
// group, K products without the split, plus KS - 1 cross-group additions with it: K + 3 covers
// every tile.
//
// Registers (hipcc -O3 for gfx950, kernel-resource-usage remark; ScratchSize 0 and no spill in
// every instantiation; fp32 and bf16 output are the same):
//   tile   BM x BN    K split   waves/WG   VGPRs   AGPRs   LDS bytes   waves/SIMD (remark)
//    1     64 x 64      no          4        97      16      32768         4
//    2     64 x 32     2-way        4       128      16      32768         3
//    3     64 x 32     4-way        8       138       0      32768         3
//    4    128 x 128     no          8       130       0      65536         3
//    5    128 x 64     2-way        8       160       0      65536         3
//    6    128 x 32     4-way        8       226       0      65536         2
#include "common.hpp"
#include "linear_stream.hpp"

namespace dnn {

constexpr int LS_BK = 128;           // columns of x per LDS stage: 4 k-steps
constexpr int LS_KSTEP = 32;         // columns per k-step: 4 lane groups x 8 bf16, one MFMA
constexpr int LS_RING = 8;           // k-steps of weight loads in flight per wave
constexpr int LS_ROWB = LS_BK * 2;   // bytes of an LDS row
constexpr int LS_CUS = 256;          // CUs of an MI355X: the split tiles are taken below one WG per CU

// BM = rows of the x tile (every wave takes all of them: BM / 16 accumulators); NW = waves;
// KS = groups of waves that split a stage's k-steps (1, 2, 4).
template <int BM, int NW, int KS, bool OUT_F32>
__global__ __launch_bounds__(NW * 64) void linear_stream_kernel(
    const u16* __restrict__ x, long ldx, const u16* __restrict__ w, long ldw,
    const float* __restrict__ bias, void* __restrict__ y, long ldy, int M, int N, int K, int act,
    int vec) {
  constexpr int NT = NW * 64;                   // threads
  constexpr int WN = NW / KS;                   // neuron groups of 16 per workgroup
  constexpr int FM = BM / 16;                   // accumulators (16-row blocks) per wave
  constexpr int SK = LS_BK / LS_KSTEP;          // k-steps of a stage: 4
  constexpr int NS = SK / KS;                   // k-steps of a wave per stage: 4, 2 or 1
  constexpr int U = LS_RING;                    // k-steps of weight loads in flight per wave
  constexpr int XD = U / NS;                    // stages of x in flight in registers
  constexpr int XJ = BM * (LS_BK / 8) / NT;     // 16-byte chunks of x per thread and stage
  constexpr int STAGE = BM * LS_ROWB;
  static_assert(NW % KS == 0 && SK % KS == 0 && U % NS == 0, "whole groups, whole stages");
  static_assert(XD % 2 == 0, "the LDS buffer of a ring slot is fixed; stage pairs are whole");
  static_assert((NT / 16) % 16 == 0, "a thread's x rows share row & 15");
  static_assert((KS - 1) * WN * FM * 1024 <= 2 * STAGE, "K-split reduction fits the x buffers");
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int wn = wave % WN, ks = wave / WN;
  const int m0 = blockIdx.y * BM;
  const int n0 = (blockIdx.x * WN + wn) * 16;
  const bool wlive = n0 < N;  // false: this wave stores nothing
  const u16* wr = w + (long)min(n0 + i, N - 1) * ldw;
  // stages, rounded up to whole trips of the unrolled loop (the extra ones are zeros of x)
  const int S = (K + LS_BK * XD - 1) / (LS_BK * XD) * XD;
  // first column of k-step j (0 .. 3; group j / NS) of stage s: see the header for NS == 1
  auto stage_col = [&](int s, int j) {
    return NS >= 2 ? s * LS_BK + j * LS_KSTEP
                   : (s >> 1) * (2 * LS_BK) + j * (2 * LS_KSTEP) + (s & 1) * LS_KSTEP;
  };

  // Every load is unconditional from a clamped (valid) address: a branch around a load makes
  // the compiler wait for ALL loads at every use, and so does a select on the loaded value that
  // it is free to hoist. What is outside the operands is made harmless where x is written to
  // LDS: columns past K are zeros there, so the weights a lane re-reads for them (K % 32 == 0:
  // its 8 columns are inside K or wholly outside, where it takes the row's last 8) meet zeros;
  // rows past M and neurons past N (row M - 1 / N - 1 re-read) only reach outputs that are
  // never stored. (A re-read NaN or infinity times zero is NaN, in a neuron whose real last 8
  // weights hold it: its outputs are not finite by definition.)
  auto load_w = [&](int s, int e) {
    const int k = stage_col(s, ks * NS + e) + 8 * g;
    return *(const uint4*)(wr + min(k, K - 8));
  };
  // x chunks of a stage: thread -> rows (tid >> 4) + (NT / 16) j, chunk tid & 15 = 4 (k-step)
  // + (lane group whose fragment it is)
  const int xrow = tid >> 4, xch = tid & 15;
  auto x_col = [&](int s) { return stage_col(s, xch >> 2) + (xch & 3) * 8; };
  auto load_x = [&](int s, uint4 (&xr)[XJ]) {
    const int k = min(x_col(s), K - 8);
#pragma unroll
    for (int j = 0; j < XJ; ++j)
      xr[j] = *(const uint4*)(x + (long)min(m0 + xrow + (NT / 16) * j, M - 1) * ldx + k);
  };
  auto store_x = [&](int s, char* buf, const uint4 (&xr)[XJ]) {
    const bool in = x_col(s) < K;
#pragma unroll
    for (int j = 0; j < XJ; ++j) {
      const int r = xrow + (NT / 16) * j;  // r & 15 == xrow & 15
      *(uint4*)(buf + r * LS_ROWB + ((xch ^ (xrow & 15)) << 4)) =
          make_uint4(in ? xr[j].x : 0u, in ? xr[j].y : 0u, in ? xr[j].z : 0u, in ? xr[j].w : 0u);
    }
  };

  f32x4_t acc[FM];
#pragma unroll
  for (int f = 0; f < FM; ++f) acc[f] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  // each stage of x is issued just before the weights of its own k-steps, here and in the loop
  uint4 xq[XD][XJ];
  uint4 wq[U];
#pragma unroll
  for (int d = 0; d < XD; ++d) {
    load_x(d, xq[d]);
#pragma unroll
    for (int e = 0; e < NS; ++e) wq[d * NS + e] = load_w(d, e);
    __builtin_amdgcn_sched_barrier(0);  // keep the issue order of the loop
  }

  for (int s0 = 0; s0 < S; s0 += XD) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      __builtin_amdgcn_sched_barrier(0);  // nothing moves across k-steps: loads keep their order
      const int d = u / NS, e = u % NS;  // ring slot of the stage, k-step of the wave in it
      const int s = s0 + d;
      char* buf = lds + (d & 1) * STAGE;
      if (e == 0) {  // first k-step of the stage (compile time)
        // this buffer was last read in stage s - 2, which every wave left before it passed
        // the barrier of stage s - 1
        store_x(s, buf, xq[d]);
        __syncthreads();
        load_x(s + XD, xq[d]);
      }
      const bf16x8_t a = __builtin_bit_cast(bf16x8_t, wq[u]);
      const int ch = (ks * NS + e) * 4 + g;  // the lane's x chunk of the k-step
#pragma unroll
      for (int f = 0; f < FM; ++f) {
        const bf16x8_t b =
            *(const bf16x8_t*)(buf + (16 * f + i) * LS_ROWB + ((ch ^ i) << 4));
        acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[f], 0, 0, 0);
      }
      // refill the slot after its last use: the new load takes the registers it frees (a load
      // into other registers has to be copied into the ring at the loop's end, after a wait)
      wq[u] = load_w(s + XD, e);
    }
  }

  if constexpr (KS > 1) {  // fixed order: ((group 0) + (group 1)) + (group 2)) + (group 3)
    __syncthreads();       // the x buffers are free
    f32x4_t* red = (f32x4_t*)lds + (wn * FM) * 64 + lane;
    if (ks > 0) {
#pragma unroll
      for (int f = 0; f < FM; ++f) red[((ks - 1) * WN * FM + f) * 64] = acc[f];
    }
    __syncthreads();
    if (ks > 0) return;
#pragma unroll
    for (int q = 1; q < KS; ++q)
#pragma unroll
      for (int f = 0; f < FM; ++f) acc[f] += red[((q - 1) * WN * FM + f) * 64];
  }
  if (!wlive) return;

  const int n = n0 + 4 * g;  // this lane's 4 output features
  float bi[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bi[r] = (bias && n + r < N) ? bias[n + r] : 0.f;
  const bool whole = vec && n + 3 < N;
#pragma unroll
  for (int f = 0; f < FM; ++f) {
    const int m = m0 + 16 * f + i;
    if (m >= M) continue;
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = act_fwd(acc[f][r] + bi[r], act);
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

int linear_stream(const uint16_t* x, long ldx, const uint16_t* w, long ldw, const float* bias,
                  void* y, long ldy, int M, int N, int K, int act, int out_f32, int tile,
                  hipStream_t stream) {
  if (M < 1 || N < 1 || K < LS_KSTEP || K % LS_KSTEP) return -1;
  if (ldx < K || ldw < K || ldy < N || ldx % 8 || ldw % 8) return -2;
  if (!x || !w || !y) return -3;
  if (act != ACT_LINEAR && act != ACT_RELU && act != ACT_SIGMOID) return -4;
  if ((((uintptr_t)x) | ((uintptr_t)w)) & 15) return -5;
  const int esz = out_f32 ? 4 : 2;
  if (((uintptr_t)y) % esz) return -6;
  if (tile < 0 || tile > LINEAR_STREAM_TILES) return -8;
  // Tile choice (header). 64-row tiles while they give at most one 64 x 64 workgroup per CU;
  // past that the 128-row tiles, which fetch W once per 128 rows. Then the widest tile that
  // still gives a workgroup per CU, else the most split one of those rows that is chosen at all
  // (2-way at 64 rows: measured faster than the 4-way, header).
  auto wgs = [&](int bm, int bn) { return ((long)(N + bn - 1) / bn) * (((long)M + bm - 1) / bm); };
  if (!tile) {
    if (M <= 64 || wgs(64, 64) <= LS_CUS)
      tile = wgs(64, 64) >= LS_CUS ? 1 : 2;
    else
      tile = wgs(128, 128) >= LS_CUS ? 4 : wgs(128, 64) >= LS_CUS ? 5 : 6;
  }
  const int bm = tile <= 3 ? 64 : 128;
  const int bn = tile == 4 ? 128 : (tile == 1 || tile == 5) ? 64 : 32;
  const int nw = tile <= 2 ? 4 : 8;
  const long tiles_m = ((long)M + bm - 1) / bm;
  if (tiles_m > 65535) return -7;
  // 4 consecutive outputs of a row in one store: every row's n0 + 4 g must be 4-element aligned
  const int vec = ldy % 4 == 0 && ((uintptr_t)y) % (4 * esz) == 0;
  const dim3 grid((N + bn - 1) / bn, (unsigned)tiles_m), block(nw * 64);
#define DNN_LS(BM_, NW_, KS_)                                                                   \
  if (out_f32)                                                                                  \
    hipLaunchKernelGGL((linear_stream_kernel<BM_, NW_, KS_, true>), grid, block, 0, stream, x,  \
                       ldx, w, ldw, bias, y, ldy, M, N, K, act, vec);                           \
  else                                                                                          \
    hipLaunchKernelGGL((linear_stream_kernel<BM_, NW_, KS_, false>), grid, block, 0, stream, x, \
                       ldx, w, ldw, bias, y, ldy, M, N, K, act, vec);
  switch (tile) {
    case 1: DNN_LS(64, 4, 1) break;
    case 2: DNN_LS(64, 4, 2) break;
    case 3: DNN_LS(64, 8, 4) break;
    case 4: DNN_LS(128, 8, 1) break;
    case 5: DNN_LS(128, 8, 2) break;
    default: DNN_LS(128, 8, 4) break;
  }
#undef DNN_LS
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

}  // namespace dnn
