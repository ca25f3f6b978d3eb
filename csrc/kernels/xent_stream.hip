// Last layer + softmax cross-entropy over ANY class count with no logits matrix in memory
// (gfx950): dz, the loss, the correct count and the bias-gradient partials straight from x and W.
// The contract is that of the GEMM-fused cross-entropy (gemm.hpp, one 64/128-wide class tile)
// with the 64-row partials of softmax_xent; the logits z = x . W^T + b are computed TWICE on
// v_mfma_f32_16x16x32_bf16 instead of being written as fp32 and read back (8 bytes of traffic and
// 4 bytes of residency per logit).
//
// Structure (grid M / 64, 4 waves):
//   * the block's x[64][K] tile is loaded ONCE into LDS and stays there for both sweeps, K
//     padded with zeros to a multiple of 256 (8 k-steps, the weight ring below). Its row is
//     KMAX bf16 (KMAX = 256, 512 or 1024, the smallest that holds K: 32, 64 or 128 KiB, so a
//     narrow K still fits several workgroups on a CU); that is the cap XENT_STREAM_MAX_K = 1024.
//     Layout: linear_stream.hip's XOR chunk swizzle, the 16-byte chunk c of row r at chunk
//     c ^ (r & 15) -- conflict-free for the ds_read_b128 of 16 rows by the 16 lanes of a lane
//     group;
//   * a class tile is 128 columns; a wave owns 32 of them, all 64 rows: 2 x 4 accumulators.
//     WEIGHTS NEVER TOUCH LDS (linear_stream.hip): lane (i = lane & 15, g = lane >> 4) reads
//     w[n][k + 8 g .. + 7] of classes n = c0 + i and c0 + 16 + i with one 16-byte load each, and
//     those registers are the A fragments; every x fragment read from LDS feeds TWO MFMAs (4
//     ds_read_b128 per 8 MFMAs: half the LDS read rate of a 16-class wave);
//   * the weight loads run ahead in a register ring of 8 k-steps (16 loads per lane, 16 KiB of
//     W per wave in flight) that walks ONE flat stream -- tile 0 .. T - 1 of sweep 1, then
//     the same tiles of sweep 2 -- so it never drains at a tile's epilogue: the exponentials of
//     tile t run under the loads of tile t + 1. No branch and no select in the k loop; loads
//     past K or past class N - 1 re-read a valid address and meet zeros of x or a masked column;
//   * swapped operands, mfma(W fragment, x fragment): a lane holds 4 consecutive classes of ONE
//     row 16 f + i per accumulator, 8 logits per row and tile, and visits its columns in rising
//     order.
//
// Sweep 1 is an ONLINE softmax PER LANE: for each of its 4 rows a lane keeps (m, s, argmax) over
// the columns it has seen. A tile gives 8 logits: m' = max(m, tile max) -- '>' keeps the lowest
// column --, s = s * exp(m - m') + ((e0 + e1) + (e2 + e3)) + ((e4 + e5) + (e6 + e7)) with
// e = exp(z - m'); exp(0) = 1 is exact, so nothing is rounded while the maximum stands. Columns
// >= n_cls are selected away (never multiplied). No shuffle, no barrier and no atomic inside the
// sweep. After it the partial states are merged in a fixed order: lane groups g ^ 1, then g ^ 2
// (shuffles), then waves 0, 1, 2, 3 serially by one thread per row through LDS; a merge is
// m' = max, s = s1 exp(m1 - m') + s2 exp(m2 - m') (one of the factors is exactly 1), argmax by
// (greater maximum, then lower column). The label's logit is kept by the one lane that owns
// that column. Then per row loss = (m - z_label) + log s, and the block's loss_part / correct
// are the 6-level wave butterfly over its 64 rows (a chain of 7 with the row's own rounding).
//
// Sweep 2 recomputes every tile through the same loop body: the accumulator chains are the same
// MFMAs in the same order, so every logit has the bits it had in sweep 1. dz = (exp(z - m) / s -
// onehot) * scale is rounded once to bf16 and stored (8-byte stores where dz allows), zeros in
// columns >= n_cls and rows with a label < 0; the STORED values are summed over the lane's 4 rows
// serially, then over the 16 lanes i by the xor butterfly 1, 2, 4, 8 (chain 7), and lane i = 0
// writes colsum. Two launches are bit-identical.
//
// Longest chain of roundings in a row sum s, in the units of tests/_wide_softmax_oracle.py (an
// exponential beyond the formula's own counts 2, a product or an addition 1), T = ceil(n_cls /
// 128) tiles:
//     D = 3 (the 8 terms of a tile) + 4 (T - 1) (per later tile: rescale 2 + 1, addition 1)
//         + 4 * 5 (merges: 2 lane-group levels + 3 waves) = 4 T + 19,
// e.g. 23 up to 128 classes, 27 at 130, 31 at 257, 55 at 1025, 1043 at 32768 -- against n_cls - 1
// of a serial sum. The rescales' exponents m_old - m_new telescope to the term's own m - z, so the
// 1.25 (m - z) u of the oracle's exponential covers them.
// XS_NEG = -1e38 stands for "no column seen" (finite, so XS_NEG - XS_NEG = 0 and no NaN).
//
// Registers (hipcc -O3 for gfx950, kernel-resource-usage remark): 198 VGPRs + 32 AGPRs, no
// scratch; LDS 36608 / 69376 / 134912 bytes at KMAX 256 / 512 / 1024, i.e. 2, 2 and 1 waves per
// SIMD. Measured (bench/xent_stream_bench.py, profiles/xent_stream/xent_stream_bench.jsonl)
// against linear_fwd to fp32 logits + softmax_xent it LOSES at all four shapes, 1.21 x (65536 x
// 1024 x 512) to 1.57 x (16384 x 8192 x 1024) the pair's time: the grid is M / 64 workgroups of
// one wave per SIMD, and the second GEMM costs more than the logits' round trip. What it buys is
// the logits buffer (4 bytes per logit); the engine's switch stays off by default.
#include "common.hpp"
#include "xent_stream.hpp"

namespace dnn {

constexpr int XS_BN = 128;    // class columns per tile
constexpr int XS_RING = 8;    // k-steps of weight loads in flight per wave
constexpr float XS_NEG = -1.0e38f;

// One gradient entry before its bf16 rounding (softmax_wide.hip's: not contracted to an fma).
__device__ __forceinline__ float xs_grad(float z, float mx, float inv, bool hot, float scale) {
#pragma clang fp contract(off)
  const float p = __expf(z - mx) * inv;
  return (p - (hot ? 1.f : 0.f)) * scale;
}

// (m, s, a) <- merge with (om, os, oa): commutative bit for bit (no fma).
__device__ __forceinline__ void xs_merge(float& m, float& s, int& a, float om, float os, int oa) {
#pragma clang fp contract(off)
  if (om > m || (om == m && oa < a)) a = oa;
  const float mn = fmaxf(m, om);
  s = s * __expf(m - mn) + os * __expf(om - mn);
  m = mn;
}

template <int KMAX>
__global__ __launch_bounds__(256) void xent_stream_kernel(
    const u16* __restrict__ x, long ldx, const u16* __restrict__ w, long ldw,
    const float* __restrict__ bias, const int* __restrict__ labels, u16* __restrict__ dz,
    long ld_dz, int N, int K, int n_cls, float scale, float* __restrict__ loss_part,
    int* __restrict__ correct, float* __restrict__ colsum, long ld_colsum, int vec_dz,
    int vec_cs) {
  constexpr int ROWB = KMAX * 2;  // bytes of an LDS row of x
  __shared__ __attribute__((aligned(16))) char xs[XENT_STREAM_ROWS * ROWB];
  __shared__ float s_wm[4][XENT_STREAM_ROWS], s_ws[4][XENT_STREAM_ROWS];
  __shared__ int s_wa[4][XENT_STREAM_ROWS];
  __shared__ float s_zl[XENT_STREAM_ROWS], s_m[XENT_STREAM_ROWS], s_inv[XENT_STREAM_ROWS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  const long row0 = (long)blockIdx.x * XENT_STREAM_ROWS;
  const int KS = (K + 255) / 256 * XS_RING;  // k-steps of a tile, whole rings
  const int NT = (N + XS_BN - 1) / XS_BN;    // class tiles

  // ---- weights: the flat stream of (tile, k-step) and its ring -----------------------------
  auto load_w = [&](int t, int ks, int h) {
    const int n = min(t * XS_BN + wave * 32 + 16 * h + i, N - 1);
    return *(const uint4*)(w + (long)n * ldw + min(32 * ks + 8 * g, K - 8));
  };
  uint4 wq[XS_RING][2];
#pragma unroll
  for (int u = 0; u < XS_RING; ++u) {  // KS >= XS_RING: all of tile 0
    wq[u][0] = load_w(0, u, 0);
    wq[u][1] = load_w(0, u, 1);
  }
  int pt = 0, pk = XS_RING;  // the next (tile, k-step) to fetch
  if (pk == KS) {
    pk = 0;
    pt = NT > 1 ? 1 : 0;
  }

  // ---- x[64][K] -> LDS, zeros in columns K .. 32 KS ----------------------------------------
  if (tid < XENT_STREAM_ROWS) s_zl[tid] = -INFINITY;
  for (int cb = 0; cb < KS / 8; ++cb) {  // 32 chunks = 256 columns per trip
    const int c = cb * 32 + (tid & 31);
    const bool in = c * 8 < K;
    uint4 v[8];
#pragma unroll
    for (int rb = 0; rb < 8; ++rb) {
      const int r = rb * 8 + (tid >> 5);
      v[rb] = *(const uint4*)(x + (row0 + r) * ldx + min(c * 8, K - 8));
    }
#pragma unroll
    for (int rb = 0; rb < 8; ++rb) {
      const int r = rb * 8 + (tid >> 5);
      *(uint4*)(xs + r * ROWB + ((c ^ (r & 15)) << 4)) =
          in ? v[rb] : make_uint4(0u, 0u, 0u, 0u);
    }
  }
  int lab[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) lab[f] = labels[row0 + 16 * f + i];
  __syncthreads();

  float m[4], s[4], inv[4];
  int am[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    m[f] = XS_NEG;
    s[f] = 0.f;
    am[f] = 1 << 30;
    inv[f] = 0.f;
  }

  for (int pass = 0; pass < 2; ++pass) {
    for (int t = 0; t < NT; ++t) {
      f32x4_t acc[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int f = 0; f < 4; ++f) acc[h][f] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < KS; k0 += XS_RING) {
#pragma unroll
        for (int u = 0; u < XS_RING; ++u) {
          __builtin_amdgcn_sched_barrier(0);  // loads keep their order across k-steps
          const int ch = (k0 + u) * 4 + g;    // the lane's x chunk of the k-step
          const bf16x8_t a0 = __builtin_bit_cast(bf16x8_t, wq[u][0]);
          const bf16x8_t a1 = __builtin_bit_cast(bf16x8_t, wq[u][1]);
#pragma unroll
          for (int f = 0; f < 4; ++f) {
            const bf16x8_t b = *(const bf16x8_t*)(xs + (16 * f + i) * ROWB + ((ch ^ i) << 4));
            acc[0][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b, acc[0][f], 0, 0, 0);
            acc[1][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b, acc[1][f], 0, 0, 0);
          }
          wq[u][0] = load_w(pt, pk, 0);  // refill the slot after its last use
          wq[u][1] = load_w(pt, pk, 1);
          const bool wrap = ++pk == KS;  // wave-uniform: scalar selects
          pk = wrap ? 0 : pk;
          pt += wrap;
          pt = pt == NT ? 0 : pt;  // sweep 2 re-walks the tiles; past its end: tile 0, unused
        }
      }

      // ---- the tile's logits: z = acc + bias, the same bits in both sweeps -----------------
      const int cb = t * XS_BN + wave * 32;  // cb < N: the wave's 32 columns are all below N
      float bi[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) bi[h][r] = bias[min(cb + 16 * h + 4 * g + r, N - 1)];

      if (pass == 0) {
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          float z[8], tm = XS_NEG;
          int ta = 1 << 30;
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int col = cb + 16 * h + 4 * g + r;
              const float v = acc[h][f][r] + bi[h][r];
              z[4 * h + r] = v;
              if (col < n_cls && v > tm) {  // columns rise: '>' keeps the lowest
                tm = v;
                ta = col;
              }
              if (col < n_cls && col == lab[f]) s_zl[16 * f + i] = v;  // the one owner
            }
          if (tm > m[f]) am[f] = ta;  // an equal maximum keeps the earlier, lower column
          const float mn = fmaxf(m[f], tm);
          float e[8];
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float ex = __expf(z[4 * h + r] - mn);
              e[4 * h + r] = cb + 16 * h + 4 * g + r < n_cls ? ex : 0.f;  // a select
            }
          const float ts = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
          s[f] = s[f] * __expf(m[f] - mn) + ts;
          m[f] = mn;
        }
      } else if (cb < N) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int col0 = cb + 16 * h + 4 * g;
          f32x4_t cs = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int f = 0; f < 4; ++f) {
            bf16x4_t o;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float z = acc[h][f][r] + bi[h][r];
              const float gr = xs_grad(z, m[f], inv[f], col0 + r == lab[f], scale);
              const bool use = lab[f] >= 0 && col0 + r < n_cls;  // a select, never a product
              const u16 hb = f2bf(use ? gr : 0.f);
              o[r] = (short)hb;
              cs[r] += bf2f(hb);
            }
            u16* dr = dz + (row0 + 16 * f + i) * ld_dz + col0;
            if (vec_dz) {
              *(bf16x4_t*)dr = o;
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r) dr[r] = (u16)o[r];
            }
          }
          if (colsum) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
              for (int o = 1; o < 16; o <<= 1) cs[r] += __shfl_xor(cs[r], o, 64);
            if (i == 0) {
              float* cr = colsum + (long)blockIdx.x * ld_colsum + col0;
              if (vec_cs) {
                *(f32x4_t*)cr = cs;
              } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) cr[r] = cs[r];
              }
            }
          }
        }
      }
    }

    if (pass == 0) {  // merge the lanes' states; the block's loss and correct count
#pragma unroll
      for (int f = 0; f < 4; ++f) {
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) {
          const float om = __shfl_xor(m[f], o, 64), os = __shfl_xor(s[f], o, 64);
          const int oa = __shfl_xor(am[f], o, 64);
          xs_merge(m[f], s[f], am[f], om, os, oa);
        }
        if (g == 0) {
          s_wm[wave][16 * f + i] = m[f];
          s_ws[wave][16 * f + i] = s[f];
          s_wa[wave][16 * f + i] = am[f];
        }
      }
      __syncthreads();
      if (tid < XENT_STREAM_ROWS) {  // wave 0, a row per lane
        float rm = s_wm[0][tid], rs = s_ws[0][tid];
        int ra = s_wa[0][tid];
#pragma unroll
        for (int q = 1; q < 4; ++q) xs_merge(rm, rs, ra, s_wm[q][tid], s_ws[q][tid], s_wa[q][tid]);
        const int label = labels[row0 + tid];
        const bool valid = label >= 0;
        float loss = valid ? (rm - s_zl[tid]) + __logf(rs) : 0.f;
        int corr = valid && ra == label;
        s_m[tid] = valid ? rm : 0.f;
        s_inv[tid] = valid ? 1.f / rs : 0.f;
        loss = wave_sum(loss);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) corr += __shfl_xor(corr, o, 64);
        if (tid == 0) {
          if (loss_part) loss_part[blockIdx.x] = loss;
          if (correct) correct[blockIdx.x] = corr;
        }
      }
      __syncthreads();
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        m[f] = s_m[16 * f + i];
        inv[f] = s_inv[16 * f + i];
      }
    }
  }
}

int xent_stream(const uint16_t* x, long ldx, const uint16_t* w, long ldw, const float* bias,
                const int* labels, uint16_t* dz, long ld_dz, int M, int N, int K, int n_cls,
                float scale, float* loss_part, int* correct, float* colsum, long ld_colsum,
                hipStream_t stream) {
  if (M < XENT_STREAM_ROWS || M % XENT_STREAM_ROWS || N < 64 || N % 64 || K < 64 || K % 64 ||
      K > XENT_STREAM_MAX_K || n_cls < 1 || n_cls > N)
    return -1;
  if (ldx < K || ldw < K || ld_dz < N || ldx % 8 || ldw % 8 || (colsum && ld_colsum < N))
    return -2;
  if (!x || !w || !bias || !labels || !dz) return -3;
  if (((((uintptr_t)x) | ((uintptr_t)w)) & 15) || ((uintptr_t)dz & 1) || ((uintptr_t)colsum & 3))
    return -5;
  const int vec_dz = (uintptr_t)dz % 8 == 0 && ld_dz % 4 == 0;
  const int vec_cs = colsum && (uintptr_t)colsum % 16 == 0 && ld_colsum % 4 == 0;
  const dim3 grid(M / XENT_STREAM_ROWS), block(256);
#define DNN_XS(KMAX_)                                                                          \
  hipLaunchKernelGGL(xent_stream_kernel<KMAX_>, grid, block, 0, stream, x, ldx, w, ldw, bias,  \
                     labels, dz, ld_dz, N, K, n_cls, scale, loss_part, correct, colsum,        \
                     ld_colsum, vec_dz, vec_cs)
  if (K <= 256) DNN_XS(256);
  else if (K <= 512) DNN_XS(512);
  else DNN_XS(1024);
#undef DNN_XS
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

}  // namespace dnn
