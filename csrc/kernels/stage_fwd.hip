// Fused stage forward: all L layers of a narrow serving stage in ONE launch on bf16 weights
// (interface and math: stage_fwd.hpp). The per-layer path launches L GEMMs (+ softmax_rows) and
// sends every hidden activation through a global buffer; at these widths (<= 512) each of those
// launches is latency-bound. Here a hidden activation is born in registers, rounded to bf16 once
// and kept in LDS, and only x, the weights and the final output touch global memory.
//
// build-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
//
// Design.
//   * Work split: grid = ceil(M / BM) workgroups, one BM-row tile each, walking the layers in
//     order. Row tiles are independent: no grid-wide barrier, no flag, no cooperative launch.
//       tile  BM   waves  rows x columns of a wave in a layer of width N
//        1    16     4    16 x N / 4
//        2    64     4    64 x N / 4
//     Wave w owns the output columns [w N / 4, (w + 1) N / 4): NG = N / 64 groups of 16
//     neurons, times FM = BM / 16 blocks of 16 rows, all NG FM accumulators of a
//     layer held in registers (NG = 8, FM = 4: 128 per lane) until the layer's contraction is
//     over. Because of that the output tile overwrites the input tile IN PLACE after one barrier:
//     there is one activation buffer, not two.
//   * Products: __builtin_amdgcn_mfma_f32_16x16x32_bf16 with SWAPPED operands, mfma(W fragment,
//     activation fragment), as in mlp_tail.hip and linear_w4a8.hip: lane (i = lane & 15, g = lane
//     >> 4) then holds 4 consecutive output features n0 + 16 c + 4 g + r of data row 16 f + i,
//     which is one 8-byte LDS write (hidden layers) or one vector store (final layer).
//   * Weights are NOT staged through LDS (staging depth 0): no two waves share a weight row, so lane (i, g) loads W[n0 + 16 c + i][32 s + 8 g .. + 7] (16 bytes) straight
//     into the register that IS the A fragment. Loads run D k-steps of 32 columns ahead of their
//     use in a register ring, D = 8 / 4 / 2 for T <= 2 / <= 5 / more fragments per k-step (T = NG,
//     plus FM in layer 0; at most 24 fragments = 96 registers). A workgroup reads every weight
//     once, from L2.
//   * Layer 0 streams x from global memory the same way: lane (i, g) loads x[m][32 s + 8 g ..]
//     for its FM rows into the same ring (the four column waves re-read the tile's x from L1),
//     so layer 0 touches no LDS and K0 is bound only by % 64. Rows past M re-read row M - 1
//     and are never stored.
//   * Activation tile in LDS: bf16 [BM][LD], LD = STAGE_FWD_MAX_WIDTH + 8 elements. The row
//     stride of 1040 bytes is 16 mod 256, so the 16 rows that the lanes of one g read for a B
//     fragment (ds_read_b128 of columns 32 s + 8 g ..) start in 16 distinct 16-byte bank groups
//     of the 64 banks, and the 8-byte epilogue writes of lanes (i, g = 0, 1) fall in 32 distinct
//     8-byte slots. LDS bytes per workgroup = BM * (widest + 8) * 2 with widest = 512 compiled
//     in: 16640 / 66560 for tile 1 / 2 (static_assert against 160 KB below).
//   * Two barriers per layer: one after the epilogue wrote LDS (the next layer reads it), one
//     after the contraction (every wave has read the tile before anyone overwrites it).
//   * Softmax last layer (one 64-wide tile, n_cls <= 64): the mapping changes to wave w = row
//     block w, all 64 columns (NG = 4, FM = 1; tile 1: wave 0 only), so a data row's 64 logits
//     sit in the 4 lanes of one i and the row max and sum are two lane exchanges; probabilities
//     = __expf(z - max) / sum as softmax_rows computes them, columns < n_cls only.
// The summation order of an output is fixed by the shapes alone (one accumulator per output,
// ascending k, 32 products per MFMA): every tile gives the same bits, which are not in general
// the bits of the per-layer GEMM (its k order differs).
//
// Tile choice (tile = 0): 16 rows while that gives at most one workgroup per CU (M <= 4096),
// else 64 rows: a 16-row workgroup re-reads all the stage's weights from L2 for a quarter of
// the flops. Reasoned, then measured: DESIGN.md "Fused stage forward". Not shipped: a 128-row
// tile on 8 waves (two 64-row halves of this mapping). Its 128 accumulators plus the ring do
// not fit the 256 registers a wave has at 8 waves per workgroup: it compiled with 568 bytes of
// scratch per lane.
#include "common.hpp"
#include "stage_fwd.hpp"

namespace dnn {
namespace {

constexpr int SF_LD = STAGE_FWD_MAX_WIDTH + 8;  // LDS row stride in elements
constexpr int SF_CUS = 256;                     // CUs of an MI355X

template <int BM>
struct SfGeo {
  static constexpr int NW = 4;
  static constexpr int NT = 64 * NW;
  static constexpr int FM = BM / 16;
  static constexpr int LDS_BYTES = BM * SF_LD * 2;
  static_assert(BM == 16 || BM == 64, "tiles");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS of a gfx950 CU");
  static_assert((SF_LD * 2) % 256 == 16, "bank layout of the activation tile");
};

// Ring depth in k-steps from the fragments T a k-step loads per lane (NG weight fragments, plus
// FM of x in layer 0): at most 24 fragments = 96 registers in flight.
template <int T>
constexpr int sf_depth() { return T <= 2 ? 8 : T <= 5 ? 4 : 2; }

// acc[c][f] = sum_k W[n0 + 16 c + .][k] * h[16 (rb0 + f) + .][k] over K columns. Global
// addresses are a wave-uniform base plus a 32-bit byte offset of the lane (the launcher bounds
// the operands): wb = row n0 of the weight, wo = the lane's (row i, column 8 g), ldw16 = 16 row
// strides in bytes. The h fragments come from global memory (GLOBAL_B: xb = the tile's first
// row of x, xo[f] = the lane's row of block f, clamped, column 8 g) or from the LDS tile (bl:
// row 16 rb0 + i, column 8 g).
template <int NG, int FM, bool GLOBAL_B>
__device__ __forceinline__ void sf_mma(f32x4_t (&acc)[NG][FM], const char* __restrict__ wb,
                                       unsigned wo, long ldw16, const char* __restrict__ xb,
                                       const unsigned (&xo)[FM], const u16* bl, int K) {
  constexpr int D = sf_depth<NG + (GLOBAL_B ? FM : 0)>();
  const int S = K / 32;  // k-steps; K % 64 == 0, so S >= 2
  bf16x8_t wr[D][NG];
  bf16x8_t xr[GLOBAL_B ? D : 1][FM];
  // every load is unconditional from a clamped address (linear_fp8.hip): past the end the
  // ring re-reads the last k-step and never uses it
  auto load = [&](int s, bf16x8_t (&w)[NG], bf16x8_t (&x)[FM]) {
    const int k = min(s, S - 1) * 64;  // bytes
#pragma unroll
    for (int c = 0; c < NG; ++c) w[c] = *(const bf16x8_t*)(wb + c * ldw16 + k + wo);
    if constexpr (GLOBAL_B) {
#pragma unroll
      for (int f = 0; f < FM; ++f) x[f] = *(const bf16x8_t*)(xb + k + xo[f]);
    }
  };
  auto step = [&](int s, const bf16x8_t (&w)[NG], const bf16x8_t (&x)[FM]) {
    bf16x8_t b[FM];
#pragma unroll
    for (int f = 0; f < FM; ++f) {
      if constexpr (GLOBAL_B) b[f] = x[f];
      else b[f] = *(const bf16x8_t*)(bl + f * 16 * SF_LD + s * 32);
    }
#pragma unroll
    for (int c = 0; c < NG; ++c)
#pragma unroll
      for (int f = 0; f < FM; ++f)
        acc[c][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[c], b[f], acc[c][f], 0, 0, 0);
  };
#pragma unroll
  for (int c = 0; c < NG; ++c)
#pragma unroll
    for (int f = 0; f < FM; ++f) acc[c][f] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int d = 0; d < D; ++d) load(d, wr[d], xr[GLOBAL_B ? d : 0]);
  int s0 = 0;
  for (; s0 + D <= S; s0 += D) {
#pragma unroll
    for (int u = 0; u < D; ++u) {
      __builtin_amdgcn_sched_barrier(0);  // nothing moves across k-steps: loads keep their order
      step(s0 + u, wr[u], xr[GLOBAL_B ? u : 0]);
      load(s0 + u + D, wr[u], xr[GLOBAL_B ? u : 0]);  // refill the slot after its MFMAs
    }
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < D; ++u)  // the S % D steps left: already loaded (wave-uniform branch)
    if (s0 + u < S) step(s0 + u, wr[u], xr[GLOBAL_B ? u : 0]);
}

// One layer of a wave in the column mapping: contraction, then bias + activation and either the
// in-place bf16 write of the LDS tile (hidden layer) or the masked global store (final layer).
template <int BM, int NG, bool GLOBAL_B>
__device__ __forceinline__ void sf_layer(const StageFwdParams& p, const StageFwdLayer& ly,
                                         u16* hs, bool last, int vec) {
  constexpr int FM = SfGeo<BM>::FM;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * BM;
  constexpr int rb0 = 0;            // the wave's first 16-row block: every wave takes all rows
  const int n0 = wave * NG * 16;    // the wave's first output column
  unsigned xo[FM];
#pragma unroll
  for (int f = 0; f < FM; ++f)  // rows past M re-read row M - 1 (never stored)
    xo[f] = GLOBAL_B ? (unsigned)min(16 * (rb0 + f) + i, p.M - 1 - m0) * (unsigned)(2 * p.ldx) + 16 * g
                     : 0u;
  f32x4_t acc[NG][FM];
  sf_mma<NG, FM, GLOBAL_B>(acc, (const char*)(ly.W + (long)n0 * ly.ldw),
                           i * (unsigned)(2 * ly.ldw) + 16 * g, 32 * ly.ldw,
                           (const char*)(p.x + (long)m0 * p.ldx), xo,
                           hs + (16 * rb0 + i) * SF_LD + 8 * g, ly.K);
  if (!last) __syncthreads();  // every wave has read the tile: overwrite it in place
#pragma unroll
  for (int c = 0; c < NG; ++c) {
    const int n = n0 + 16 * c + 4 * g;  // this lane's 4 output features of the group
    float bi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bi[r] = ly.bias ? ly.bias[n + r] : 0.f;
#pragma unroll
    for (int f = 0; f < FM; ++f) {
      const int row = 16 * (rb0 + f) + i;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = act_fwd(acc[c][f][r] + bi[r], ly.act);
      if (!last) {
        bf16x4_t o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (short)f2bf(v[r]);
        *(bf16x4_t*)(hs + row * SF_LD + n) = o;
        continue;
      }
      const int m = m0 + row;
      if (m >= p.M) continue;
      if (p.out_f32) {
        float* o = (float*)p.y + (long)m * p.ldy + n;
        if (vec) {
          *(f32x4_t*)o = f32x4_t{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = v[r];
        }
      } else {
        u16* o = (u16*)p.y + (long)m * p.ldy + n;
        if (vec) {
          bf16x4_t q;
#pragma unroll
          for (int r = 0; r < 4; ++r) q[r] = (short)f2bf(v[r]);
          *(bf16x4_t*)o = q;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = f2bf(v[r]);
        }
      }
    }
  }
}

// Softmax last layer in the row mapping: wave w = 16-row block w, all 64 columns.
template <int BM>
__device__ __forceinline__ void sf_softmax(const StageFwdParams& p, const StageFwdLayer& ly,
                                           const u16* hs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave >= BM / 16) return;  // (tile 1: one row block; no barrier follows)
  const int i = lane & 15, g = lane >> 4;
  const unsigned none[1] = {0u};
  f32x4_t acc[4][1];
  sf_mma<4, 1, false>(acc, (const char*)ly.W, i * (unsigned)(2 * ly.ldw) + 16 * g, 32 * ly.ldw,
                      nullptr, none, hs + (16 * wave + i) * SF_LD + 8 * g, ly.K);
  // lane (i, g) holds the logits 16 c + 4 g + r of row i: the row lives in the 4 lanes of one i
  float z[4][4];
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int col = 16 * c + 4 * g + r;
      z[c][r] = col < p.n_cls ? acc[c][0][r] + (ly.bias ? ly.bias[col] : 0.f) : -INFINITY;
      mx = fmaxf(mx, z[c][r]);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float se = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      z[c][r] = __expf(z[c][r] - mx);  // exp(-inf) = 0 past n_cls
      se += z[c][r];
    }
  se += __shfl_xor(se, 16, 64);
  se += __shfl_xor(se, 32, 64);
  const float inv = 1.f / se;
  const int m = blockIdx.x * BM + 16 * wave + i;
  if (m >= p.M) return;
  float* o = (float*)p.y + (long)m * p.ldy;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int col = 16 * c + 4 * g + r;
      if (col < p.n_cls) o[col] = z[c][r] * inv;
    }
}

template <int BM>
__global__ __launch_bounds__(SfGeo<BM>::NT) void stage_fwd_kernel(const StageFwdParams p,
                                                                  int vec) {
  __shared__ __attribute__((aligned(16))) u16 hs[SfGeo<BM>::LDS_BYTES / 2];
#define DNN_SF_CASE(NG_, GB_) \
  case NG_: sf_layer<BM, NG_, GB_>(p, ly, hs, last, vec); break;
#define DNN_SF_LAYER(GB_)                                                   \
  switch (ly.N >> 6) { /* block-uniform */                                  \
    DNN_SF_CASE(1, GB_) DNN_SF_CASE(2, GB_) DNN_SF_CASE(3, GB_) DNN_SF_CASE(4, GB_) \
    DNN_SF_CASE(5, GB_) DNN_SF_CASE(6, GB_) DNN_SF_CASE(7, GB_) DNN_SF_CASE(8, GB_) \
  }
  {  // layer 0: x from global memory; never the last layer (L >= 2)
    const StageFwdLayer& ly = p.layer[0];
    const bool last = false;
    DNN_SF_LAYER(true)
  }
  for (int l = 1; l < p.L; ++l) {
    const StageFwdLayer& ly = p.layer[l];
    const bool last = l == p.L - 1;
    __syncthreads();  // the layer before wrote its activations into the tile
    if (last && ly.act == ACT_SOFTMAX) {
      sf_softmax<BM>(p, ly, hs);
      return;
    }
    DNN_SF_LAYER(false)
  }
#undef DNN_SF_LAYER
#undef DNN_SF_CASE
}

}  // namespace

const char* stage_fwd_error(int code) {
  switch (code) {
    case 0: return "ok";
    case -1: return "sizes: M >= 1, K0 % 64 == 0, 2 <= L <= 8, every width % 64 == 0 and <= 512, "
                    "K of a layer == N of the layer before, softmax N == 64 with 1 <= n_cls <= 64";
    case -2: return "a leading dimension is smaller than its row or not a multiple of 8 elements";
    case -3: return "null operand (x, a weight or y)";
    case -4: return "activation: linear / relu / sigmoid per layer, softmax on the last layer "
                    "only and into fp32";
    case -5: return "alignment: x and the weights 16 bytes, y its element size";
    case -6: return "tile must be 0..2";
    case -7: return "more row tiles than a grid holds";
    case -9: return "launch failed";
    default: return "unknown error";
  }
}

int stage_fwd(const StageFwdParams& p, hipStream_t stream) {
  if (p.L < 2 || p.L > STAGE_FWD_MAX_LAYERS) return -1;
  if (p.M < 1 || p.K0 < 64 || p.K0 % 64) return -1;
  if (!p.x || !p.y) return -3;
  // (lane offsets are 32-bit: 64 rows of x and 512 rows of a weight stay below 4 GB)
  if (p.ldx < p.K0 || p.ldx % 8 || p.ldx >= (1L << 22)) return -2;
  if (((uintptr_t)p.x) & 15) return -5;
  int K = p.K0;
  for (int l = 0; l < p.L; ++l) {
    const StageFwdLayer& ly = p.layer[l];
    if (ly.N < 64 || ly.N % 64 || ly.N > STAGE_FWD_MAX_WIDTH || ly.K != K) return -1;
    if (!ly.W) return -3;
    if (ly.ldw < K || ly.ldw % 8 || ly.ldw >= (1L << 22)) return -2;
    if (((uintptr_t)ly.W) & 15) return -5;
    if (ly.act == ACT_SOFTMAX) {
      if (l != p.L - 1 || !p.out_f32) return -4;
      if (ly.N != 64 || p.n_cls < 1 || p.n_cls > 64) return -1;
    } else if (ly.act != ACT_LINEAR && ly.act != ACT_RELU && ly.act != ACT_SIGMOID) {
      return -4;
    }
    K = ly.N;
  }
  if (p.ldy < K) return -2;  // K: the last layer's width
  const int esz = p.out_f32 ? 4 : 2;
  if (((uintptr_t)p.y) % esz) return -5;
  int tile = p.tile;
  if (tile < 0 || tile > STAGE_FWD_TILES) return -6;
  // Tile choice (header): 16 rows up to one workgroup per CU, else 64.
  if (!tile) tile = p.M <= 16 * SF_CUS ? 1 : 2;
  const int bm = tile == 1 ? 16 : 64;
  const long tiles_m = ((long)p.M + bm - 1) / bm;
  if (tiles_m > 0x7fffffffL) return -7;
  // 4 consecutive outputs of a row in one store: every row's n must be 4-element aligned
  const int vec = p.ldy % 4 == 0 && ((uintptr_t)p.y) % (4 * esz) == 0;
  const dim3 grid((unsigned)tiles_m);
  if (tile == 1)
    hipLaunchKernelGGL(stage_fwd_kernel<16>, grid, dim3(SfGeo<16>::NT), 0, stream, p, vec);
  else
    hipLaunchKernelGGL(stage_fwd_kernel<64>, grid, dim3(SfGeo<64>::NT), 0, stream, p, vec);
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

}  // namespace dnn
