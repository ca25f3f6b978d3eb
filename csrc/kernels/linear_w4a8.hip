// Forward layer over MXFP4 weight rows against e4m3 activations (w4a8), for the serving buckets
// over 8 rows:
//   y[m][n] = act(fl32(sx[m] * S[m][n]) + b[n]),
//   S[m][n] = sum_k e4m3(xq[m][k]) * e2m1(q[n][k]) * 2^(e[n][k / 32] - 127),
// xq / sx the rows of quant_rows_fp8 (elementwise.hip), q / e the rows of quant_rows_mxfp4
// (mxfp4.hip); a block whose scale byte is 0 contributes nothing (mxfp4.hpp). The products run
// on v_mfma_scale_f32_16x16x128_f8f6f4 in its mixed form: cbsz = 4 makes the A operand 32 e2m1
// codes in 4 VGPRs, taken undecoded, blgp = 0 leaves B e4m3. The weight block scales ARE the
// instruction's A-side scale operand (one e8m0 byte per lane and k-step: the byte of one of the
// k-step's four MX blocks); the activation side passes the constant E8M0 1.0 (0x7F). The fp32
// row scale is applied once per output in the epilogue.
//
// Structure: linear_w8a8.hip's (read its header first), 4 waves, grid (ceil(N / BN), ceil(M /
// BM)), swapped operands, a k-step of 128 columns = one MFMA per (neuron group, 16-row block),
// the x tile shared through swizzled LDS, every load unconditional from a clamped address, the
// ring of 4 stages refilled after its MFMAs, 4 consecutive outputs of a row in one store. What
// differs:
//   * the instruction's k map, measured (identity x against random codes under distinct scale
//     bytes): the fp4 operand's slot j of lane (i = lane & 15, g = lane >> 4) is k = 32 g + j, 32
//     consecutive columns, and the scale byte that lane supplies applies to exactly those: a
//     lane's 32 columns of a k-step ARE one MX block. The e4m3 operand's slot j is k = 16 g + j
//     for j < 16 and k = 64 + 16 g + (j - 16) for j >= 16, two halves of 16. w8a8 never sees the
//     difference (both its operands use one slot order and its scales are constant); here the
//     x fragment must follow the e4m3 map: chunks g and 4 + g of the 128-byte LDS row;
//   * lane (i, g) reads the 32 codes q[n0 + i][k + 32 g .. + 31] with ONE 16-byte load (fp8
//     needed two) straight into the 4 registers that are the A fragment: nibble j is column k +
//     32 g + j;
//   * its scale is the byte e[n0 + i][k / 32 + g], one global_load_ubyte per (k-step, neuron
//     group) into the same ring, zero-extended: byte 0 of the scale VGPR, op_sel 0. `e` may
//     have any alignment and any row stride, so the byte load is the general path and the only
//     one here. Not built: re-assigning columns to lanes so that a lane's four k-steps of a trip
//     use four consecutive scale bytes (one 4-byte load, op_sel 0..3). It needs the x stage in
//     LDS to be the trip's 512 columns instead of one k-step's 128 and a dword-aligned e row,
//     which the engine's row stride of Kp / 32 (only even) does not give; the byte loads are 1 /
//     17 of the weight bytes and ride in the ring the codes already keep full;
//   * the zero-block rule: the MFMA would multiply an E = 0 block by 2^-127, so a lane clears
//     its four code registers when its scale byte is 0 -- at use time (4 v_cndmask per fragment,
//     shared by the fragment's FM MFMAs), never around the load: a select around a load makes
//     the compiler drain all loads;
//   * epilogue: __fmul_rn(sx, S) (one rounding of its own, nothing fused), + bias, act_fwd,
//     store.
// Edges: columns past K are zeros where x is written to LDS; the codes and the scale byte a lane
// re-reads for them (its row's last block, always inside the operands) meet those zeros, and
// every scale byte the format defines is finite. Rows past M and neurons past N re-read row M -
// 1 / N - 1 of xq, q and e and only reach outputs that are never stored: no byte of e outside
// [N][K / 32] is ever read.
// No atomics and no split of K anywhere: the summation order is fixed by (M, N, K, tile).
//
// Tiles (BM x BN; tile = 1, 2), chosen in the launcher by M and N with linear_w8a8's rule: 64
// x 64 (NG = 1) while ceil(N / 64) ceil(M / 64) <= 512 (at most two of its workgroups per CU),
// or M <= 64; else 128 x 128 (NG = 2). Measurements at the end of this header.
// Longest accumulation chain: one accumulator takes one MFMA (128 products) per 128 columns, so
// 128 ceil(K / 128) additions, the same for every tile.
//
// Registers (hipcc -O3 for gfx950, kernel-resource-usage remark; ScratchSize 0 and no spill in
// every instantiation; fp32 and bf16 output are the same):
//   tile   BM x BN     NG   waves/WG   VGPRs   AGPRs   LDS bytes   waves/SIMD (remark)
//    1     64 x 64      1      4         90      16      16384         4
//    2     128 x 128    2      4        162      64      32768         2
// The MFMA is emitted as v_mfma_scale_f32_16x16x128_f8f6f4 a[..3], v[4 regs], v[8 regs], ...
// cbsz:4, and the k loop keeps partial load counters (vmcnt(10) .. (14) in tile 1).
// Measured (bench/linear_w4a8_bench.py --w4a8-tiles 1,2, graph replay, median of 7 alternating
// rounds, all contenders in one job, the GEMM alone; profiles/linear_w4a8/):
//   * the tile rule, taken over from linear_w8a8, picks the faster tile at all 16 points. On
//     8192 x 8192 read cold, tile 1 / tile 2: 27.9 / 56.9 us at 64 rows, 27.2 / 61.0 at 128, 46.4
//     / 60.1 at 256 (the last bucket on tile 1), then 84.1 / 59.5 at 512, 159 / 92.9 at 1024 and
//     2616 / 1415 at 16384. On the resident 1024 x 1024 layer 5.84 / 11.6 us at 64 rows up to
//     9.97 / 14.8 at 2048 (tile 1), then 17.6 / 16.2 at 4096 and 58.7 / 46.4 at 16384 (tile 2);
//   * against linear_w8a8 on the same rows the GEMM ties or sits within 4 % on either side
//     (28.0 against 27.1 us at 64 rows cold, 92.4 against 92.3 at 1024, 1404 against 1347 at
//     16384), except 512 rows cold, 59.6 against 52.8 us: the fp4 x fp8 form showed no rate
//     advantage over fp8 x fp8 anywhere, and halving the weight bytes did not show either -- at
//     these sizes neither the weight stream nor the MFMA rate is what bounds the kernel.
// Not measured: the instruction's cost in isolation; the op_sel scale variant (not built).
#include "common.hpp"
#include "linear_w4a8.hpp"

namespace dnn {

constexpr int LW4_BK = 128;  // columns per stage = per k-step = per MFMA; bytes of an LDS row
constexpr int LW4_NT = 256;  // threads: 4 waves
constexpr int LW4_XD = 4;    // stages of x, of codes and of scale bytes in flight in registers
constexpr int LW4_CUS = 256;  // CUs of an MI355X
constexpr int LW4_ONE = 0x7F7F7F7F;  // E8M0 1.0 in every byte: the x side's block scale
constexpr int LW4_FP4 = 4;   // cbsz: the A operand holds e2m1 codes (4 VGPRs)

typedef int lw4_i32x4_t __attribute__((ext_vector_type(4)));
typedef int lw4_i32x8_t __attribute__((ext_vector_type(8)));

// 2 x 16 e4m3 codes -> the 32-code x fragment (8 VGPRs), slot j = code j
__device__ __forceinline__ lw4_i32x8_t lw4_frag(lw4_i32x4_t lo, lw4_i32x4_t hi) {
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
// 32 e2m1 codes -> the operand the builtin takes; with cbsz = 4 only its first 4 registers exist
__device__ __forceinline__ lw4_i32x8_t lw4_frag4(lw4_i32x4_t c) {
  return __builtin_shufflevector(c, c, 0, 1, 2, 3, -1, -1, -1, -1);
}

// BM = rows of the x tile (FM = BM / 16 row blocks per wave); NG = groups of 16 neurons per wave.
template <int BM, int NG, bool OUT_F32>
__global__ __launch_bounds__(LW4_NT) void linear_w4a8_kernel(
    const unsigned char* __restrict__ xq, long ldxq, const float* __restrict__ sx,
    const unsigned char* __restrict__ q, long ldq, const unsigned char* __restrict__ e, long lde,
    const float* __restrict__ bias, void* __restrict__ y, long ldy, int M, int N, int K, int act,
    int vec) {
  constexpr int FM = BM / 16;                    // 16-row blocks (accumulators per neuron group)
  constexpr int XJ = BM * (LW4_BK / 16) / LW4_NT;  // 16-byte chunks of x per thread and stage
  constexpr int XR = LW4_NT / 8;                 // rows between a thread's chunks: 32
  constexpr int STAGE = BM * LW4_BK;
  constexpr int XD = LW4_XD;
  static_assert(XD % 2 == 0, "the LDS buffer of a ring slot is fixed");
  static_assert(XJ >= 1 && (XR / 2) % 8 == 0, "a thread's x rows share (row >> 1) & 7");
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.y * BM;
  const int n0 = (blockIdx.x * 4 + wave) * NG * 16;  // the wave's first neuron
  const int KB = K / 32;                             // blocks (scale bytes) of a weight row
  const unsigned char* qr[NG];
  const unsigned char* er[NG];
#pragma unroll
  for (int c = 0; c < NG; ++c) {
    const long n = min(n0 + 16 * c + i, N - 1);
    qr[c] = q + n * ldq;
    er[c] = e + n * lde;
  }
  // stages, rounded up to whole trips of the unrolled loop (the extra ones are zeros x codes)
  const int S = (K + LW4_BK * XD - 1) / (LW4_BK * XD) * XD;

  // Every load is unconditional from a clamped (valid) address (linear_fp8.hip: a branch or a
  // select around a load makes the compiler wait for ALL loads at every use). A lane's block of
  // a k-step is inside K or wholly outside, where it takes the row's last block and its scale
  // byte and meets the zeros that store_x wrote for those columns.
  auto load_w = [&](int s, lw4_i32x4_t (&wr)[NG], int (&sr)[NG]) {
    const int b = min(s * (LW4_BK / 32) + g, KB - 1);  // the lane's block
#pragma unroll
    for (int c = 0; c < NG; ++c) {
      wr[c] = *(const lw4_i32x4_t*)(qr[c] + 16 * b);
      sr[c] = er[c][b];
    }
  };
  // x chunks of a stage: thread -> rows (tid >> 3) + 32 j, chunk tid & 7
  const int xrow = tid >> 3, xch = tid & 7;
  const int xsw = (xch ^ ((xrow >> 1) & 7)) << 4;  // the same for all of the thread's rows
  auto load_x = [&](int s, uint4 (&xr)[XJ]) {
    const int k = min(s * LW4_BK + xch * 16, K - 16);
#pragma unroll
    for (int j = 0; j < XJ; ++j)
      xr[j] = *(const uint4*)(xq + (long)min(m0 + xrow + XR * j, M - 1) * ldxq + k);
  };
  auto store_x = [&](int s, char* buf, const uint4 (&xr)[XJ]) {
    const bool in = s * LW4_BK + xch * 16 < K;
#pragma unroll
    for (int j = 0; j < XJ; ++j)
      *(uint4*)(buf + (xrow + XR * j) * LW4_BK + xsw) =
          make_uint4(in ? xr[j].x : 0u, in ? xr[j].y : 0u, in ? xr[j].z : 0u, in ? xr[j].w : 0u);
  };

  f32x4_t acc[NG][FM];
#pragma unroll
  for (int c = 0; c < NG; ++c)
#pragma unroll
    for (int f = 0; f < FM; ++f) acc[c][f] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  uint4 xr[XD][XJ];
  lw4_i32x4_t wr[XD][NG];
  int sr[XD][NG];
#pragma unroll
  for (int d = 0; d < XD; ++d) {
    load_x(d, xr[d]);
    load_w(d, wr[d], sr[d]);
    __builtin_amdgcn_sched_barrier(0);  // keep the issue order of the loop
  }

  // the lane's two x chunks of a k-step in the e4m3 operand's k map (columns 16 g .. and 64 +
  // 16 g ..), swizzled: (16 f + i) >> 1 & 7 == (i >> 1) & 7
  const int rsw0 = (g ^ ((i >> 1) & 7)) << 4, rsw1 = ((4 + g) ^ ((i >> 1) & 7)) << 4;
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
      // the zero-block rule, at use time: E == 0 is +0 whatever the nibbles hold
      lw4_i32x8_t a[NG];
#pragma unroll
      for (int c = 0; c < NG; ++c) {
        const bool live = sr[u][c] != 0;
        a[c] = lw4_frag4(lw4_i32x4_t{live ? wr[u][c][0] : 0, live ? wr[u][c][1] : 0,
                                     live ? wr[u][c][2] : 0, live ? wr[u][c][3] : 0});
      }
#pragma unroll
      for (int f = 0; f < FM; ++f) {
        const char* row = buf + (16 * f + i) * LW4_BK;
        const lw4_i32x8_t b = lw4_frag(*(const lw4_i32x4_t*)(row + rsw0),
                                       *(const lw4_i32x4_t*)(row + rsw1));
#pragma unroll
        for (int c = 0; c < NG; ++c)
          acc[c][f] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              a[c], b, acc[c][f], LW4_FP4, 0, 0, sr[u][c], 0, LW4_ONE);
      }
      // refill the slot after its MFMAs (linear_w8a8.hip: the codes ARE the A fragments)
      load_w(s + XD, wr[u], sr[u]);
    }
  }

  float sxm[FM];
#pragma unroll
  for (int f = 0; f < FM; ++f) sxm[f] = sx[min(m0 + 16 * f + i, M - 1)];
#pragma unroll
  for (int c = 0; c < NG; ++c) {
    const int n = n0 + 16 * c + 4 * g;  // this lane's 4 output features of the group
    if (n0 + 16 * c >= N) break;        // (wave-uniform) the group stores nothing
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
      for (int r = 0; r < 4; ++r) {
        // one rounding of its own; a zero row scale gives act(bias)
        float z = __fmul_rn(sxm[f], acc[c][f][r]);
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

int linear_w4a8(const unsigned char* xq, long ldxq, const float* sx, const unsigned char* q,
                long ldq, const unsigned char* e, long lde, const float* bias, void* y, long ldy,
                int M, int N, int K, int act, int out_f32, int tile, hipStream_t stream) {
  if (M < 1 || N < 1 || K < 32 || K % 32) return -1;
  if (ldxq < K || ldq < K / 2 || lde < K / 32 || ldy < N || ldxq % 16 || ldq % 16) return -2;
  if (!xq || !sx || !q || !e || !y) return -3;
  if (act != ACT_LINEAR && act != ACT_RELU && act != ACT_SIGMOID) return -4;
  if ((((uintptr_t)xq) | ((uintptr_t)q)) & 15) return -5;
  const int esz = out_f32 ? 4 : 2;
  if (((uintptr_t)y) % esz) return -6;
  if (tile < 0 || tile > LINEAR_W4A8_TILES) return -8;
  // Tile choice (header): 64 x 64 while it gives at most two workgroups per CU.
  const long wg64 = ((long)(N + 63) / 64) * (((long)M + 63) / 64);
  if (!tile) tile = (M <= 64 || wg64 <= 2 * LW4_CUS) ? 1 : 2;
  const int bm = tile == 1 ? 64 : 128, bn = bm;
  const long tiles_m = ((long)M + bm - 1) / bm;
  if (tiles_m > 65535) return -7;
  // 4 consecutive outputs of a row in one store: every row's n0 + 4 g must be 4-element aligned
  const int vec = ldy % 4 == 0 && ((uintptr_t)y) % (4 * esz) == 0;
  const dim3 grid((N + bn - 1) / bn, (unsigned)tiles_m), block(LW4_NT);
#define DNN_LW4(BM_, NG_)                                                                     \
  if (out_f32)                                                                                \
    hipLaunchKernelGGL((linear_w4a8_kernel<BM_, NG_, true>), grid, block, 0, stream, xq, ldxq, \
                       sx, q, ldq, e, lde, bias, y, ldy, M, N, K, act, vec);                  \
  else                                                                                        \
    hipLaunchKernelGGL((linear_w4a8_kernel<BM_, NG_, false>), grid, block, 0, stream, xq,     \
                       ldxq, sx, q, ldq, e, lde, bias, y, ldy, M, N, K, act, vec);
  if (tile == 1) { DNN_LW4(64, 1) } else { DNN_LW4(128, 2) }
#undef DNN_LW4
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

}  // namespace dnn
