// Dense-target losses of the last layer (gfx950): mean squared error and binary cross-entropy
// on logits against a bf16 target matrix, forward (loss partials) and backward (dz, bias-gradient
// partials) in one memory-bound pass. The training replacement, for regression / multi-label /
// autoencoder heads, of what softmax_xent (elementwise.hip) is for classifiers; the serving side
// applies the same linear / relu / sigmoid output functions.
//
// One block covers 64 rows x 256 columns: 4 waves of 16 rows, each lane owning 4 adjacent
// columns (16-byte fp32 loads, 8-byte bf16 loads and stores: guide Guideline 13). A wave loads
// all of its 16 rows before any arithmetic (16 independent loads in flight, as softmax_xent).
// Reductions run in a fixed order -- lane-serial, wave butterfly, then the 4 waves through LDS --
// so the partials are bitwise reproducible; there are no float atomics.
#include "common.hpp"
#include "dense_loss.hpp"

namespace dnn {

constexpr int DL_ROWS_PER_WAVE = 16;
constexpr int DL_ROWS = 4 * DL_ROWS_PER_WAVE;  // = XENT_ROWS_PER_BLOCK: same partial bookkeeping
constexpr int DL_COLS = 4 * kWave;             // columns per chunk

// One element: gradient g (before the bf16 rounding) and loss term (before the 1/n).
// The sigmoid is evaluated from e = exp(-|z|) as p = 1 / (1 + e), q = e p: y and 1 - y are then
// both accurate at either tail, and nothing overflows (|z| = 200: e = 0, p = 1, q = 0).
template <int LOSS, int ACT>
__device__ __forceinline__ void dense_elem(float z, float t, float coef, float& g, float& term) {
  if (ACT == ACT_SIGMOID) {
    const float e = __expf(-fabsf(z));
    const float p = __builtin_amdgcn_rcpf(1.f + e);
    const float q = e * p;
    const float y = z >= 0.f ? p : q;
    if (LOSS == DENSE_BCE) {
      term = (fmaxf(z, 0.f) - t * z) + __logf(1.f + e);
      g = coef * (y - t);
    } else {
      const float d = y - t;
      term = d * d;
      g = coef * d * (p * q);  // y (1 - y) = p q
    }
  } else {
    const float y = (ACT == ACT_RELU && !(z > 0.f)) ? 0.f : z;
    const float d = y - t;
    term = d * d;
    g = (ACT == ACT_RELU && !(z > 0.f)) ? 0.f : coef * d;
  }
}

// VEC: every row of z / t / dz can be accessed in aligned 16 / 8 / 8-byte pieces.
template <int LOSS, int ACT, bool VEC>
__global__ __launch_bounds__(256) void dense_loss_kernel(
    const float* __restrict__ z, long ld_z, const u16* __restrict__ t, long ld_t,
    const int* __restrict__ row_ok, u16* __restrict__ dz, long ld_dz, int rows, int n_out,
    int width, float coef, float inv_n, float* __restrict__ loss_part,
    float* __restrict__ colsum, long ld_colsum) {
  __shared__ float s_loss[4];
  __shared__ f32x4_t s_col[4][kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row0 = blockIdx.x * DL_ROWS + wave * DL_ROWS_PER_WAVE;
  const int col0 = blockIdx.y * DL_COLS + lane * 4;
  const bool in_w = col0 < width;                 // width % 64 == 0: all 4 columns or none
  const int nv = min(max(n_out - col0, 0), 4);    // this lane's columns below n_out
  f32x4_t zs[DL_ROWS_PER_WAVE];
  bf16x4_t ts[DL_ROWS_PER_WAVE];
  int oks[DL_ROWS_PER_WAVE];
  // loads first; rows past the end re-read the last row (always in bounds) and are masked below
  if (VEC && nv == 4) {
#pragma unroll
    for (int k = 0; k < DL_ROWS_PER_WAVE; ++k) {
      const long row = min(row0 + k, rows - 1);
      zs[k] = *(const f32x4_t*)(z + row * ld_z + col0);
      ts[k] = *(const bf16x4_t*)(t + row * ld_t + col0);
    }
  } else {
#pragma unroll
    for (int k = 0; k < DL_ROWS_PER_WAVE; ++k) {
      const long row = min(row0 + k, rows - 1);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        zs[k][e] = e < nv ? z[row * ld_z + col0 + e] : 0.f;
        ts[k][e] = e < nv ? (short)t[row * ld_t + col0 + e] : (short)0;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < DL_ROWS_PER_WAVE; ++k) {
    const int row = row0 + k;
    oks[k] = row < rows ? (row_ok ? row_ok[row] : 0) : -1;
  }
  float acc = 0.f;
  f32x4_t cs = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < DL_ROWS_PER_WAVE; ++k) {
    const int row = row0 + k;
    if (row >= rows) break;
    const bool valid = oks[k] >= 0;
    bf16x4_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float g, term;
      dense_elem<LOSS, ACT>(zs[k][e], bf2f((u16)ts[k][e]), coef, g, term);
      const bool use = valid && e < nv;  // a select, never a product: padding may hold NaN
      const u16 h = f2bf(use ? g : 0.f);
      o[e] = (short)h;
      cs[e] += bf2f(h);
      acc += use ? term : 0.f;
    }
    if (in_w) {
      u16* dr = dz + (long)row * ld_dz + col0;
      if (VEC) {
        *(bf16x4_t*)dr = o;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) dr[e] = (u16)o[e];
      }
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) s_loss[wave] = acc;
  s_col[wave][lane] = cs;
  __syncthreads();
  if (threadIdx.x == 0 && loss_part)
    loss_part[(long)blockIdx.x * gridDim.y + blockIdx.y] =
        ((s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3])) * inv_n;
  if (colsum) {
    const int col = blockIdx.y * DL_COLS + threadIdx.x;
    if (col < width) {
      const float* sc = (const float*)s_col;
      colsum[(long)blockIdx.x * ld_colsum + col] =
          (sc[threadIdx.x] + sc[DL_COLS + threadIdx.x]) +
          (sc[2 * DL_COLS + threadIdx.x] + sc[3 * DL_COLS + threadIdx.x]);
    }
  }
}

int dense_loss_row_blocks(int rows) { return (rows + DL_ROWS - 1) / DL_ROWS; }
int dense_loss_col_chunks(int width) { return (width + DL_COLS - 1) / DL_COLS; }

template <int LOSS, int ACT>
static void dense_loss_launch(bool vec, dim3 grid, hipStream_t stream, const float* z, long ld_z,
                              const u16* t, long ld_t, const int* row_ok, u16* dz, long ld_dz,
                              int rows, int n_out, int width, float coef, float inv_n,
                              float* loss_part, float* colsum, long ld_colsum) {
  if (vec)
    hipLaunchKernelGGL((dense_loss_kernel<LOSS, ACT, true>), grid, dim3(256), 0, stream, z, ld_z,
                       t, ld_t, row_ok, dz, ld_dz, rows, n_out, width, coef, inv_n, loss_part,
                       colsum, ld_colsum);
  else
    hipLaunchKernelGGL((dense_loss_kernel<LOSS, ACT, false>), grid, dim3(256), 0, stream, z, ld_z,
                       t, ld_t, row_ok, dz, ld_dz, rows, n_out, width, coef, inv_n, loss_part,
                       colsum, ld_colsum);
}

int dense_loss(const float* z, long ld_z, const uint16_t* t, long ld_t, const int* row_ok,
               uint16_t* dz, long ld_dz, int rows, int n_out, int width, int loss, int act,
               float scale, float* loss_part, float* colsum, long ld_colsum,
               hipStream_t stream) {
  if (!z || !t || !dz || rows <= 0 || n_out <= 0 || n_out > width || width % 64 ||
      ld_z < n_out || ld_t < n_out || ld_dz < width || (colsum && ld_colsum < width))
    return -1;
  if (loss == DENSE_BCE ? act != ACT_SIGMOID
                        : (loss != DENSE_MSE ||
                           (act != ACT_LINEAR && act != ACT_RELU && act != ACT_SIGMOID)))
    return -1;
  const int chunks = dense_loss_col_chunks(width);
  if (chunks > 65535) return -1;
  const dim3 grid(dense_loss_row_blocks(rows), chunks);
  const bool vec = (uintptr_t)z % 16 == 0 && ld_z % 4 == 0 && (uintptr_t)t % 8 == 0 &&
                   ld_t % 4 == 0 && (uintptr_t)dz % 8 == 0 && ld_dz % 4 == 0;
  const float coef = (float)((loss == DENSE_MSE ? 2.0 : 1.0) * (double)scale / n_out);
  const float inv_n = (float)(1.0 / n_out);
#define DL_ARGS                                                                                \
  vec, grid, stream, z, ld_z, t, ld_t, row_ok, dz, ld_dz, rows, n_out, width, coef, inv_n,     \
      loss_part, colsum, ld_colsum
  if (loss == DENSE_BCE) dense_loss_launch<DENSE_BCE, ACT_SIGMOID>(DL_ARGS);
  else if (act == ACT_SIGMOID) dense_loss_launch<DENSE_MSE, ACT_SIGMOID>(DL_ARGS);
  else if (act == ACT_RELU) dense_loss_launch<DENSE_MSE, ACT_RELU>(DL_ARGS);
  else dense_loss_launch<DENSE_MSE, ACT_LINEAR>(DL_ARGS);
#undef DL_ARGS
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

}  // namespace dnn
