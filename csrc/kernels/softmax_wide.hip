// Softmax kernels for rows wider than 256 columns (gfx950): the training loss
// (softmax_xent_wide) and the serving softmax (softmax_rows_wide). The kernels of
// elementwise.hip hold a whole row in registers (64 lanes x 4 columns); these sweep it instead,
// so the width is bounded only by int range. Contracts are those of softmax_xent /
// softmax_rows, which dispatch here for width (n_cls) > 256.
//
// A row is swept by ONE wave (the loss kernel interleaves SW_R rows per wave, each summed on its
// own): lane l owns columns 256 j + 4 l .. + 3 (16-byte fp32 loads, guide
// Guideline 13), SW_U such steps are loaded before any is consumed. Two passes, the maximum
// (and its lowest column) first, then sum exp(x - mx): each lane adds its terms serially in
// column order, then the 6-level wave butterfly. The longest addition chain of a row sum is
// therefore D = 4 floor(n_cls / 256) + min(n_cls mod 256, 4) - 1 + 6: the terms of lane 0, less
// the exact first addition, plus the butterfly (tests/_wide_softmax_oracle.py derives its bounds
// from it). Nothing is accumulated with atomics and every order is fixed: two launches are
// bitwise equal, and so are the vector and the scalar path (VEC), which differ only in the
// width of their loads and stores.
#include "common.hpp"
#include "softmax_wide.hpp"

namespace dnn {

constexpr int SW_ROWS_PER_WAVE = 16;
constexpr int SW_ROWS = 4 * SW_ROWS_PER_WAVE;  // = XENT_ROWS_PER_BLOCK: same partial bookkeeping
constexpr int SW_STEP = 4 * kWave;             // columns a wave covers per step
constexpr int SW_U = 4;                        // steps in flight per lane and row in a sweep
constexpr int SW_R = 2;                        // rows a wave of the loss kernel sweeps together
constexpr int SW_B = 8;                        // rows in flight per thread in the dz phase

// Four adjacent logits of which the first nv (<= 4; <= 0: none, nothing is read) are real;
// the others read as -inf: never the maximum, exp = 0. VEC: aligned 16-byte rows.
template <bool VEC>
__device__ __forceinline__ f32x4_t load_logits4(const float* p, int nv) {
  if (VEC && nv >= 4) return *(const f32x4_t*)p;
  f32x4_t v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = e < nv ? p[e] : -INFINITY;
  return v;
}

// R rows swept together (their loads are independent: R times the bytes in flight per lane).
// Maximum of xr[i][0..n_cls) and the lowest column holding it (np.argmax tie rule), in every
// lane.
template <bool VEC, int R>
__device__ __forceinline__ void row_max(const float* const (&xr)[R], int n_cls, int lane,
                                        float (&mx)[R], int (&amax)[R]) {
#pragma unroll
  for (int i = 0; i < R; ++i) {
    mx[i] = -INFINITY;
    amax[i] = 1 << 30;
  }
  for (int b = 0; b < n_cls; b += SW_STEP * SW_U) {
    f32x4_t v[R][SW_U];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int u = 0; u < SW_U; ++u) {
        const int c = b + u * SW_STEP + 4 * lane;
        v[i][u] = load_logits4<VEC>(xr[i] + c, n_cls - c);
      }
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int u = 0; u < SW_U; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (v[i][u][e] > mx[i]) {  // columns rise within a lane: '>' keeps the lowest
            mx[i] = v[i][u][e];
            amax[i] = b + u * SW_STEP + 4 * lane + e;
          }
  }
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(mx[i], o, 64);
      const int oa = __shfl_xor(amax[i], o, 64);
      if (om > mx[i] || (om == mx[i] && oa < amax[i])) {
        mx[i] = om;
        amax[i] = oa;
      }
    }
}

// se[i] = sum_c exp(xr[i][c] - mx[i]) in every lane: lane-serial in column order, then the wave
// butterfly.
template <bool VEC, int R>
__device__ __forceinline__ void row_sum(const float* const (&xr)[R], int n_cls, int lane,
                                        const float (&mx)[R], float (&se)[R]) {
#pragma unroll
  for (int i = 0; i < R; ++i) se[i] = 0.f;
  for (int b = 0; b < n_cls; b += SW_STEP * SW_U) {
    f32x4_t v[R][SW_U];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int u = 0; u < SW_U; ++u) {
        const int c = b + u * SW_STEP + 4 * lane;
        v[i][u] = load_logits4<VEC>(xr[i] + c, n_cls - c);
      }
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int u = 0; u < SW_U; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          se[i] += __expf(v[i][u][e] - mx[i]);  // exp(-inf) = 0: an exact no-op
  }
#pragma unroll
  for (int i = 0; i < R; ++i) se[i] = wave_sum(se[i]);
}

// One gradient entry before its bf16 rounding. Not contracted to an fma, so that every
// instantiation rounds alike.
__device__ __forceinline__ float xent_grad(float x, float mx, float inv, bool hot, float scale) {
#pragma clang fp contract(off)
  const float p = __expf(x - mx) * inv;
  return (p - (hot ? 1.f : 0.f)) * scale;
}

// ------------------------------------------------------------------------------------------
// softmax + cross-entropy, any width. One workgroup per 64-row block (the partial layout of
// softmax_xent_kernel). Phase A, a wave per row, 16 rows per wave taken SW_R at a time (one row
// per sweep leaves the wave waiting on a single round trip): mx, 1 / se and the label of
// every row go to LDS; loss and correct count as in the narrow kernel. Phase B, the whole
// workgroup: thread t owns columns 4 t .. 4 t + 3 of each 1024-column sweep and walks the
// block's rows in order -- dz computed, rounded, stored (8-byte bf16 stores) and the STORED
// value added into four registers: the column sums in a fixed row order, with no array
// proportional to the width. The block's logits (64 width 4 B) are read three times; the
// second and third read come from L2 / Infinity Cache while the blocks in flight fit there.
// ------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void softmax_xent_wide_kernel(
    const float* __restrict__ logits, long ld_logits, const int* __restrict__ labels,
    u16* __restrict__ dz, long ld_dz, int rows, int n_cls, int width, float scale,
    float* __restrict__ loss_part, int* __restrict__ correct, float* __restrict__ colsum,
    long ld_colsum) {
  __shared__ float s_mx[SW_ROWS], s_inv[SW_ROWS];
  __shared__ int s_lab[SW_ROWS];
  __shared__ float s_loss[4];
  __shared__ int s_corr[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long row0 = (long)blockIdx.x * SW_ROWS;
  const int nrows = (int)min((long)SW_ROWS, (long)rows - row0);

  float loss = 0.f;
  int corr = 0;
  for (int k = 0; k < SW_ROWS_PER_WAVE; k += SW_R) {
    int label[SW_R], first = -1;
#pragma unroll
    for (int i = SW_R - 1; i >= 0; --i) {
      const int r = wave * SW_ROWS_PER_WAVE + k + i;
      label[i] = r < nrows ? __builtin_amdgcn_readfirstlane(labels[row0 + r]) : -1;
      if (label[i] >= 0) first = i;
    }
    float mx[SW_R], se[SW_R];
    int amax[SW_R];
    if (first >= 0) {  // padding rows are never read (they may hold NaN): a valid row of the
      const float* xr[SW_R];  // group stands in for them and its result is dropped
#pragma unroll
      for (int i = 0; i < SW_R; ++i)
        xr[i] = logits +
                (row0 + wave * SW_ROWS_PER_WAVE + k + (label[i] >= 0 ? i : first)) * ld_logits;
      row_max<VEC, SW_R>(xr, n_cls, lane, mx, amax);
      row_sum<VEC, SW_R>(xr, n_cls, lane, mx, se);
    }
#pragma unroll
    for (int i = 0; i < SW_R; ++i) {
      const int r = wave * SW_ROWS_PER_WAVE + k + i;
      if (r >= nrows || lane != 0) continue;
      const bool valid = label[i] >= 0;
      if (valid) {
        const float xl =
            label[i] < n_cls ? logits[(row0 + r) * ld_logits + label[i]] : -INFINITY;
        loss += -(xl - mx[i] - __logf(se[i]));
        corr += amax[i] == label[i];
      }
      s_mx[r] = valid ? mx[i] : 0.f;
      s_inv[r] = valid ? 1.f / se[i] : 0.f;
      s_lab[r] = label[i];
    }
  }
  if (lane == 0) {
    s_loss[wave] = loss;
    s_corr[wave] = corr;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (loss_part) loss_part[blockIdx.x] = (s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3]);
    if (correct) correct[blockIdx.x] = s_corr[0] + s_corr[1] + s_corr[2] + s_corr[3];
  }

  for (int base = 0; base < width; base += 4 * 256) {
    const int col0 = base + 4 * (int)threadIdx.x;
    if (col0 >= width) break;
    const int nv = min(n_cls - col0, 4);  // this thread's columns below n_cls (<= 0: none)
    const int nw = min(width - col0, 4);  // ... and below width: the ones it stores
    f32x4_t cs = {0.f, 0.f, 0.f, 0.f};
    for (int r0 = 0; r0 < nrows; r0 += SW_B) {
      f32x4_t xs[SW_B];
#pragma unroll
      for (int k = 0; k < SW_B; ++k) {  // rows past the block's end re-read its last row
        const int r = min(r0 + k, nrows - 1);
        xs[k] = load_logits4<VEC>(logits + (row0 + r) * ld_logits + col0,
                                  s_lab[r] >= 0 ? nv : 0);
      }
#pragma unroll
      for (int k = 0; k < SW_B; ++k) {
        const int r = r0 + k;
        if (r >= nrows) break;
        const int label = s_lab[r];
        const float mx = s_mx[r], inv = s_inv[r];
        bf16x4_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float g = xent_grad(xs[k][e], mx, inv, col0 + e == label, scale);
          const bool use = label >= 0 && e < nv;  // a select, never a product
          const u16 h = f2bf(use ? g : 0.f);
          o[e] = (short)h;
          cs[e] += bf2f(h);
        }
        u16* dr = dz + (row0 + r) * ld_dz + col0;
        if (VEC && nw == 4) {
          *(bf16x4_t*)dr = o;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (e < nw) dr[e] = (u16)o[e];
        }
      }
    }
    if (colsum) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < nw) colsum[(long)blockIdx.x * ld_colsum + col0 + e] = cs[e];
    }
  }
}

int softmax_xent_wide(const float* logits, long ld_logits, const int* labels, uint16_t* dz,
                      long ld_dz, int rows, int n_cls, int width, float scale, float* loss_part,
                      int* correct, float* colsum, long ld_colsum, hipStream_t stream) {
  if (!logits || !labels || !dz || rows <= 0 || n_cls <= 0 || n_cls > width ||
      width > (1 << 30) || ld_logits < n_cls || ld_dz < width || (colsum && ld_colsum < width))
    return -1;
  const dim3 grid((rows + SW_ROWS - 1) / SW_ROWS), block(256);
  const bool vec = (uintptr_t)logits % 16 == 0 && ld_logits % 4 == 0 && (uintptr_t)dz % 8 == 0 &&
                   ld_dz % 4 == 0;
  if (vec)
    hipLaunchKernelGGL(softmax_xent_wide_kernel<true>, grid, block, 0, stream, logits, ld_logits,
                       labels, dz, ld_dz, rows, n_cls, width, scale, loss_part, correct, colsum,
                       ld_colsum);
  else
    hipLaunchKernelGGL(softmax_xent_wide_kernel<false>, grid, block, 0, stream, logits,
                       ld_logits, labels, dz, ld_dz, rows, n_cls, width, scale, loss_part,
                       correct, colsum, ld_colsum);
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

// ------------------------------------------------------------------------------------------
// Inference softmax over the first n_cls columns, any n_cls: a wave per row, three sweeps
// (max + argmax, sum, write), nothing kept in registers across them. out may be the logits
// themselves: a lane reads every element it writes before it writes it, and writes no other.
// ------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void softmax_rows_wide_kernel(const float* logits, long ld_in,
                                                                float* out, long ld_out, int rows,
                                                                int n_cls,
                                                                const int* __restrict__ labels,
                                                                int* __restrict__ pred,
                                                                int* correct) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const float* xr = logits + row * ld_in;
  const float* const xrs[1] = {xr};
  float mxs[1], ses[1];
  int amaxs[1];
  row_max<VEC, 1>(xrs, n_cls, lane, mxs, amaxs);
  const float mx = mxs[0];
  const int amax = amaxs[0];
  if (out) {
    row_sum<VEC, 1>(xrs, n_cls, lane, mxs, ses);
    const float inv = 1.f / ses[0];
    float* orow = out + row * ld_out;
    for (int b = 0; b < n_cls; b += SW_STEP * SW_U) {
      f32x4_t v[SW_U];
#pragma unroll
      for (int u = 0; u < SW_U; ++u) {
        const int c = b + u * SW_STEP + 4 * lane;
        v[u] = load_logits4<VEC>(xr + c, n_cls - c);
      }
#pragma unroll
      for (int u = 0; u < SW_U; ++u) {
        const int c = b + u * SW_STEP + 4 * lane;
        const int nv = min(n_cls - c, 4);
        f32x4_t p;
#pragma unroll
        for (int e = 0; e < 4; ++e) p[e] = __expf(v[u][e] - mx) * inv;
        if (VEC && nv == 4) {
          *(f32x4_t*)(orow + c) = p;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (e < nv) orow[c + e] = p[e];
        }
      }
    }
  }
  if (lane == 0) {
    if (pred) pred[row] = amax;
    if (correct && labels && labels[row] == amax) atomicAdd(correct, 1);
  }
}

int softmax_rows_wide(const float* logits, long ld_in, float* out, long ld_out, int rows,
                      int n_cls, const int* labels, int* pred, int* correct,
                      hipStream_t stream) {
  if (!logits || rows <= 0 || n_cls <= 0 || n_cls > (1 << 30) || ld_in < n_cls ||
      (out && ld_out < n_cls))
    return -1;
  const dim3 grid((rows + 3) / 4), block(256);
  const bool vec = (uintptr_t)logits % 16 == 0 && ld_in % 4 == 0 &&
                   (!out || ((uintptr_t)out % 16 == 0 && ld_out % 4 == 0));
  if (vec)
    hipLaunchKernelGGL(softmax_rows_wide_kernel<true>, grid, block, 0, stream, logits, ld_in, out,
                       ld_out, rows, n_cls, labels, pred, correct);
  else
    hipLaunchKernelGGL(softmax_rows_wide_kernel<false>, grid, block, 0, stream, logits, ld_in,
                       out, ld_out, rows, n_cls, labels, pred, correct);
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

}  // namespace dnn
