// Device-side serving chain kernels (chain.hpp; host side serve/fastpath.py). Every wait is a
// single lane polling a flag with system-scope acquire loads and s_sleep between polls, with a
// wall-clock timeout, so every wave of every launch finishes. Flags and slot headers are
// written with vector stores (the address is lane-indexed), never through the scalar cache.
//
// Weight rows are bf16, or (w_scale != nullptr) OCP e4m3 codes with one fp32 scale per output
// neuron, summed in gemv_fp8.hip's order so the rows are bitwise that kernel's. Registers of the
// fp8 forms (hipcc -O3 for gfx950, kernel-resource-usage remark; none has scratch; the bf16
// forms are what they were: 56 / 92 / 158 / 255 and 253 VGPRs):
//   kernel                          rows capacity   NB   U   VGPRs   waves/SIMD
//   chain_gemv_send_kernel<.,.,1>         1          1   4     76        6
//                                         2          1   4    124        4
//                                         4          1   2    122        4
//                                         8          1   2    202        2
//   chain_stage_kernel<1>                 1          4   4    242        2
//   (one kernel holds all four            2          4   4   (the whole kernel)
//   cs_layer_fp8 forms)                   4          4   2
//                                         8          4   2
// (NB: neurons a wave holds at once; U: 1024-column chunks whose loads are in flight together.
// The stage kernel reads x from LDS 8 columns at a time: with a lane's 16 columns of 8 rows
// held at once it needed 256 VGPRs + 20 AGPRs and ran at 1 wave/SIMD.)
//
// Or (w_e8m0 != nullptr) MXFP4: packed e2m1 codes with one e8m0 scale byte per 32 columns, summed
// in gemv_mxfp4.hip's order so the rows are bitwise that kernel's. That order depends on the
// lane's unit (16 or 32 columns), so both exist; the unit is chosen as gemv_mxfp4 chooses it.
// Registers of the mxfp4 forms (same build, same remark; none has scratch; the bf16 and fp8
// forms above are unchanged):
//   kernel                          rows capacity   unit   NB   U   VGPRs   waves/SIMD
//   chain_gemv_send_kernel<.,.,0,B>       1          32     1   2     78        6
//                                         2          32     1   2    124        4
//                                         1          16     1   4     94        5
//                                         2          16     1   4    136        3
//                                         4          16     1   2    128        4
//                                         8          16     1   2    208        2
//   chain_stage_kernel<2>                 1          32     4   2    256        2
//   (one kernel holds all six             2          32     4   2   (the whole kernel)
//   cs_layer_mxfp4 forms)                 1          16     4   4
//                                         2          16     4   4
//                                         4          16     4   2
//                                         8          16     4   1
// (unit: columns of a lane per chunk of 64 units; 32 serves 1 and 2 rows when K >= 2048. Alone,
// the six stage forms take 136 / 169 / 168 / 192 / 174 / 200 VGPRs; with U = 2 at 8 rows (226
// alone) the whole kernel came to 256 VGPRs + 12 AGPRs, 1 wave/SIMD, hence U = 1 there.)
// No margin is left in two places: chain_stage_kernel<2> sits at exactly 256 VGPRs with no AGPRs,
// so another compiler or a further edit can tip it to 1 wave/SIMD or into scratch, and the bf16
// 8-row send (unchanged) is at 255 VGPRs + 2 AGPRs, 1 wave/SIMD. Check the remark after either.
#include <algorithm>

#include "chain.hpp"
#include "common.hpp"
#include "gemv.hpp"

namespace dnn {

namespace {

bool misaligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) & 3; }
bool misaligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) & 15; }

// mxfp4 weight rows (w_e8m0 set): whole blocks of 32 columns, a lane's codes one aligned 8- or
// 16-byte load, rows of codes and of scale bytes that hold K columns, and no fp8 row scales
bool bad_mxfp4(const float* w_scale, int K, long ldw, long lde) {
  return w_scale || K % 32 || ldw % 16 || ldw < K / 2 || lde < K / 32;
}

__device__ __forceinline__ bool reached(const uint32_t* flag, uint32_t target) {
  return (int)(__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) - target) >=
         0;
}

// lane 0 of the calling wave: poll until reached or timed out. `relaxed`: a long sleep
// between polls (~1000 clocks instead of ~64), for the many workgroups of a one-launch hop
// that all wait on one flag -- their uncached polls otherwise flood the memory system the
// flag's own write has to get through (profiles/r4_chain: 4 waiting stages, 144 vs 18 us)
template <bool relaxed = false>
__device__ __forceinline__ bool spin(const uint32_t* flag, uint32_t target,
                                     unsigned long long ticks) {
  const unsigned long long t0 = wall_clock64();
  while (!reached(flag, target)) {
    if constexpr (relaxed) __builtin_amdgcn_s_sleep(16);
    else __builtin_amdgcn_s_sleep(1);
    if (wall_clock64() - t0 > ticks) return false;
  }
  return true;
}

// rows x row_bytes from src (ld sld bytes) to dst (ld dld bytes), 16-byte vectors
__device__ __forceinline__ void copy_rows(const char* src, long sld, char* dst, long dld,
                                          int rows, int row_bytes) {
  const int cpr = row_bytes >> 4;
  const int n = rows * cpr;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int r = i / cpr, c = i - r * cpr;
    *(uint4*)(dst + r * dld + 16 * c) = *(const uint4*)(src + r * sld + 16 * c);
  }
}

}  // namespace

__global__ void chain_wait_kernel(const uint32_t* flag, uint32_t target, uint32_t* err,
                                  unsigned long long ticks) {
  const unsigned l = threadIdx.x;
  if (l != 0) return;
  const bool ok = spin(flag + l, target, ticks);  // err: this wait's outcome (0 = arrived)
  __hip_atomic_store(err + l, ok ? 0u : 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(256) void chain_recv_kernel(ChainRecv p) {
  __shared__ uint32_t s_ok;
  const unsigned t = threadIdx.x;
  if (t == 0) {
    const bool ok = spin(p.flag + t, p.seq, p.timeout_ticks);
    if (!ok) __hip_atomic_store(p.err + t, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    s_ok = ok ? 1u : 0u;
  }
  __syncthreads();
  if (!s_ok) return;  // uniform
  copy_rows((const char*)p.slot, p.slot_ld, (char*)p.dst, p.dst_ld, p.rows, p.row_bytes);
  if (t < 2)
    p.dst_hdr[t] = __hip_atomic_load(p.slot_hdr + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  // every read of the slot is done before the producer may overwrite it
  __syncthreads();
  if (t == 0 && p.prev_ack) {
    __threadfence_system();
    __hip_atomic_store(p.prev_ack + t, p.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ __launch_bounds__(256) void chain_send_kernel(ChainSend p) {
  __shared__ uint32_t s_st;
  const unsigned t = threadIdx.x;
  if (t == 0) {
    bool ok = true;
    if (p.ack) ok = spin(p.ack + t, p.ack_target, p.timeout_ticks);
    uint32_t st = p.status;
    if (!st) {
      const uint32_t in = p.in_hdr ? p.in_hdr[t] : 0u;
      if (in & 0xffu)  // an upstream failure travels on unchanged (it names its stage)
        st = in;
      else if (__hip_atomic_load(p.err + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM))
        st = CHAIN_DEADLINE | ((uint32_t)(p.stage - 1) << 8);  // the producer never delivered
      else if (!ok)
        st = CHAIN_DEADLINE | ((uint32_t)(p.stage + 1) << 8);  // the consumer never drained
    }
    __hip_atomic_store(p.err + t, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    s_st = st | (ok ? 0u : 0x80000000u);
  }
  __syncthreads();
  const uint32_t st = s_st & 0x7fffffffu;
  const bool slot_free = (s_st & 0x80000000u) == 0u;
  if (st == 0u && slot_free)
    copy_rows((const char*)p.src, p.src_ld, (char*)p.dst, p.dst_ld, p.rows, p.row_bytes);
  if (t < 2)
    __hip_atomic_store(p.dst_hdr + t, t == 0 ? st : (uint32_t)p.rows, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
  __threadfence_system();  // this thread's rows and header are visible before the flag
  __syncthreads();
  if (t == 0)
    __hip_atomic_store(p.next_flag + t, p.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  if (t == 1 && p.prev_ack)
    __hip_atomic_store(p.prev_ack + (t - 1), p.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The status a hop sends on (chain_send's rule): an upstream failure travels on unchanged,
// a missed input blames the producer, an ack timeout the consumer.
__device__ __forceinline__ uint32_t hop_status(uint32_t status, const uint32_t* in_hdr,
                                               const uint32_t* err, int stage, bool ack_ok,
                                               unsigned t, bool in_ok = true) {
  if (status) return status;
  if (!in_ok) return CHAIN_DEADLINE | ((uint32_t)(stage - 1) << 8);  // input never came
  const uint32_t in = in_hdr ? __hip_atomic_load(in_hdr + t, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_SYSTEM) : 0u;
  if (in & 0xffu) return in;
  if (__hip_atomic_load(err + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM))
    return CHAIN_DEADLINE | ((uint32_t)(stage - 1) << 8);
  if (!ack_ok) return CHAIN_DEADLINE | ((uint32_t)(stage + 1) << 8);
  return 0u;
}

constexpr int CG_WAVES = 4;  // output neurons (waves) per 256-thread workgroup, as gemv.hip

// ---- fp8 weight rows (w_scale != nullptr) ----------------------------------------------------
// gemv_fp8.hip's sum, bit for bit: lane l owns columns k0 + 1024 u + 16 l .. + 15 of every
// 1024-column chunk, chunks ascending, columns ascending, then wave_sum; dec * x is exact in
// fp32, so only this order fixes the result (not U, not how many neurons a wave holds).
constexpr int C8_CHUNK = 1024;  // columns per chunk: 64 lanes x 16 codes
typedef float f32x2_t __attribute__((ext_vector_type(2)));

// acc[m] += sum over 8 of the lane's columns (two words of codes) of dec(code) * x[m][column],
// columns ascending
template <int M>
__device__ __forceinline__ void fp8_fma8(unsigned w0, unsigned w1, const bf16x8_t (&xv)[M],
                                         float (&acc)[M]) {
  const unsigned word[2] = {w0, w1};
#pragma unroll
  for (int j = 0; j < 2; ++j) {  // word j holds columns 4 j .. 4 j + 3
    const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8(word[j], false);
    const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8(word[j], true);
    const float we[4] = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int m = 0; m < M; ++m) acc[m] += we[c] * bf2f((u16)xv[m][4 * j + c]);
    }
  }
}

// One neuron's fp8 row against `rows` <= M input rows in global memory (chain_gemv_send; the
// loop of gemv_fp8_kernel: all loads of U chunks are issued before any is used).
template <int M, int U>
__device__ __forceinline__ void fp8_row_sum(const unsigned char* qr, const u16* x, long ldx,
                                            int rows, int K, int lane, float (&acc)[M]) {
  for (int k0 = 0; k0 < K; k0 += C8_CHUNK * U) {
    uint4 qv[U];
    bf16x8_t xv[U][2][M];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + u * C8_CHUNK + lane * 16;
      if (k < K) {  // K % 16 == 0: a lane's 16 columns are inside K or wholly outside
        qv[u] = *(const uint4*)(qr + k);
#pragma unroll
        for (int m = 0; m < M; ++m) {
          xv[u][0][m] = m < rows ? *(const bf16x8_t*)(x + m * ldx + k) : bf16x8_t{};
          xv[u][1][m] = m < rows ? *(const bf16x8_t*)(x + m * ldx + k + 8) : bf16x8_t{};
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (k0 + u * C8_CHUNK + lane * 16 < K) {
        fp8_fma8<M>(qv[u].x, qv[u].y, xv[u][0], acc);
        fp8_fma8<M>(qv[u].z, qv[u].w, xv[u][1], acc);
      }
  }
}

// ---- mxfp4 weight rows (w_e8m0 != nullptr) --------------------------------------------------
// gemv_mxfp4.hip's sum, bit for bit. A lane's unit there is B columns of every chunk of 64 B:
// B = 32 (a whole block) for a request of 1 or 2 rows when K >= C4_WHOLE_MIN_K, B = 16 (half a
// block) otherwise, so lane l owns columns k0 + 64 B u + B l .. + B - 1, chunks ascending,
// columns ascending, then wave_sum. The decoded code times its block scale times a bf16 x is
// exact in fp32, so only this order fixes the result (not U, not how many neurons a wave holds)
// -- but the order DOES depend on B, which is why both units exist here too. The decode is that
// kernel's: the hardware conversion with the scale operand E << 23, a block with E == 0 has its
// code word cleared first. There is no scale multiply after the reduction.
constexpr int C4_WHOLE_MIN_K = 2048;  // gemv_mxfp4.hip's GEMV4_WHOLE_BLOCK_MIN_K
template <int W>
using qword_t = unsigned __attribute__((ext_vector_type(W)));  // W code words: 8 W columns

// acc[m] += sum over the 8 columns of one code word of dec(code) * 2^(E - 127) * x[m][column],
// columns ascending (byte c / 2 of the word, its low nibble first). `word` is already cleared
// when E == 0.
template <int M>
__device__ __forceinline__ void fp4_fma8(unsigned word, float scale, const bf16x8_t (&xv)[M],
                                         float (&acc)[M]) {
  const f32x2_t d[4] = {__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, scale, 0),
                        __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, scale, 1),
                        __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, scale, 2),
                        __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, scale, 3)};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float we = d[c >> 1][c & 1];
#pragma unroll
    for (int m = 0; m < M; ++m) acc[m] += we * bf2f((u16)xv[m][c]);
  }
}

// One neuron's mxfp4 row (codes qr, scale bytes er) against `rows` <= M input rows in global
// memory (chain_gemv_send; the loop of gemv_mxfp4_kernel: all loads of U chunks are issued
// before any is used).
template <int M, int U, int B>
__device__ __forceinline__ void fp4_row_sum(const unsigned char* qr, const unsigned char* er,
                                            const u16* x, long ldx, int rows, int K, int lane,
                                            float (&acc)[M]) {
  constexpr int CHUNK = 64 * B, W = B / 8;
  for (int k0 = 0; k0 < K; k0 += CHUNK * U) {
    qword_t<W> qv[U];
    unsigned ev[U];
    bf16x8_t xv[U][W][M];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + u * CHUNK + lane * B;
      if (k < K) {  // K % 32 == 0: a lane's B columns are inside K or wholly outside
        qv[u] = *(const qword_t<W>*)(qr + (k >> 1));
        ev[u] = er[k >> 5];
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
          for (int j = 0; j < W; ++j)
            xv[u][j][m] = m < rows ? *(const bf16x8_t*)(x + m * ldx + k + 8 * j) : bf16x8_t{};
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (k0 + u * CHUNK + lane * B < K) {
        const float scale = __uint_as_float(ev[u] << 23);  // 2^(E - 127)
#pragma unroll
        for (int j = 0; j < W; ++j)  // word j holds columns k + 8 j .. k + 8 j + 7
          fp4_fma8<M>(ev[u] ? qv[u][j] : 0u, scale, xv[u][j], acc);
      }
  }
}

// FP8: p.w holds e4m3 codes and p.w_scale their row scales; only the k loop and the scale
// multiply differ -- the waits, hop_status, counter, header, flag and ack are the bf16 form's.
// Registers: the file header; U as gemv_fp8.hip (8 rows at U = 4 cannot be held).
// B4 != 0: p.w holds packed e2m1 codes and p.w_e8m0 their block scales; B4 is the lane's unit
// (16 or 32 columns, chosen by the launcher as gemv_mxfp4 chooses it), U as gemv_mxfp4.hip.
template <int M, bool OUT_F32, bool FP8 = false, int B4 = 0>
__global__ __launch_bounds__(256) void chain_gemv_send_kernel(ChainGemvSend p) {
  __shared__ uint32_t s_go;
  const unsigned t = threadIdx.x;
  const int lane = t & 63;
  if (t == 0) {
    // the input (folded receive) first, then the consumer's slot; both bounded
    const bool in_ok = !p.in_flag ? true
                       : blockIdx.x == 0 ? spin(p.in_flag + t, p.seq, p.timeout_ticks)
                                         : spin<true>(p.in_flag + t, p.seq, p.timeout_ticks);
    // (the grid can be N / 4 workgroups: all but one poll the consumer's ack relaxed, as the
    // folded receive's input flag, so a wide layer does not flood the memory system)
    const bool ok = !p.ack ? true
                    : blockIdx.x == 0 ? spin(p.ack + t, p.ack_target, p.timeout_ticks)
                                      : spin<true>(p.ack + t, p.ack_target, p.timeout_ticks);
    if (!ok || !in_ok)  // remembered for the last workgroup: bit 0 ack, bit 1 input
      __hip_atomic_fetch_or(p.counter + 1 + t, (ok ? 0u : 1u) | (in_ok ? 0u : 2u),
                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_go = hop_status(p.status, p.in_hdr, p.err, p.stage, ok, t, in_ok) == 0u ? 1u : 0u;
  }
  __syncthreads();
  // a wave per output neuron; with fewer workgroups than N / 4 (the folded receive: every
  // workgroup spins, so the grid is capped) a wave takes every (grid * 4)-th neuron
  for (int n = blockIdx.x * CG_WAVES + (int)(t >> 6); s_go && n < p.N;
       n += gridDim.x * CG_WAVES) {  // (no early return: every thread reaches the barrier)
    float acc[M];
#pragma unroll
    for (int m = 0; m < M; ++m) acc[m] = 0.f;
    if constexpr (FP8) {
      fp8_row_sum<M, (M <= 2 ? 4 : 2)>((const unsigned char*)p.w + (long)n * p.ldw, p.x, p.ldx,
                                       p.rows, p.K, lane, acc);
    } else if constexpr (B4 != 0) {
      fp4_row_sum<M, (B4 == 32 || M > 2 ? 2 : 4), B4>(
          (const unsigned char*)p.w + (long)n * p.ldw, p.w_e8m0 + (long)n * p.lde, p.x, p.ldx,
          p.rows, p.K, lane, acc);
    } else {
      const uint16_t* wr = p.w + (long)n * p.ldw;
      constexpr int U = 4;
      for (int k0 = 0; k0 < p.K; k0 += 512 * U) {
        bf16x8_t wv[U], xv[U][M];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int k = k0 + u * 512 + lane * 8;
          if (k < p.K) {
            wv[u] = *(const bf16x8_t*)(wr + k);
#pragma unroll
            for (int m = 0; m < M; ++m)
              xv[u][m] = m < p.rows ? *(const bf16x8_t*)(p.x + m * p.ldx + k) : bf16x8_t{};
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int k = k0 + u * 512 + lane * 8;
          if (k < p.K) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float we = bf2f((u16)wv[u][e]);
#pragma unroll
              for (int m = 0; m < M; ++m) acc[m] += we * bf2f((u16)xv[u][m][e]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int m = 0; m < M; ++m) acc[m] = wave_sum(acc[m]);
    if (lane < p.rows) {
      float v = 0.f;
#pragma unroll
      for (int m = 0; m < M; ++m)
        if (m == lane) v = acc[m];
      if constexpr (FP8) {  // gemv_fp8_kernel's epilogue, statement for statement
        v = __fmul_rn(p.w_scale[n], v);
        v += p.bias ? p.bias[n] : 0.f;
        v = act_fwd(v, p.act);
      } else if constexpr (B4 != 0) {  // gemv_mxfp4_kernel's epilogue: no scale multiply
        v += p.bias ? p.bias[n] : 0.f;
        v = act_fwd(v, p.act);
      } else {
        v = act_fwd(v + (p.bias ? p.bias[n] : 0.f), p.act);
      }
      if constexpr (OUT_F32)
        ((float*)p.dst)[(long)lane * p.dst_ld + n] = v;
      else
        ((u16*)p.dst)[(long)lane * p.dst_ld + n] = f2bf(v);
    }
  }
  __threadfence_system();  // this thread's rows are visible before the workgroup counts in
  __syncthreads();
  if (t == 0) {
    const uint32_t prev = __hip_atomic_fetch_add(p.counter + t, 1u, __ATOMIC_ACQ_REL,
                                                 __HIP_MEMORY_SCOPE_AGENT);
    if (prev == gridDim.x - 1) {  // the last workgroup: every row has landed
      const uint32_t fail = __hip_atomic_load(p.counter + 1 + t, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t st = hop_status(p.status, p.in_hdr, p.err, p.stage, (fail & 1u) == 0u, t,
                                     (fail & 2u) == 0u);
      __hip_atomic_store(p.counter + t, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(p.counter + 1 + t, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(p.err + t, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(p.dst_hdr + t, st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(p.dst_hdr + 1 + t, (uint32_t)p.rows, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
      __threadfence_system();
      __hip_atomic_store(p.next_flag + t, p.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      if (p.prev_ack)
        __hip_atomic_store(p.prev_ack + t, p.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// ---- persistent stage (ChainStage, chain.hpp) ---------------------------------------------
// sync words: [0, nslot) per-slot arrival counters, [nslot, 2 nslot) per-slot ack failures
// (written by workgroup 0 before it releases the slot), then go, exit.

// One request's layer for `rows` <= M rows staged in LDS (xs, row stride K). A wave takes NB
// neurons at once (their weight loads in flight together, the x vectors read once for all);
// per neuron the loop and reduction order are chain_gemv_send's, so the outputs are bitwise
// the same. `logits` != nullptr (softmax, one workgroup): the pre-activation rows go there.
template <int M, int NB>
__device__ __forceinline__ void cs_layer(const ChainStage& p, const u16* xs, int rows, char* dst,
                                         float* logits) {
  const unsigned t = threadIdx.x;
  const int lane = t & 63;
  constexpr int U = 2;  // (the loop order per lane is U-independent: bitwise as U = 4)
  for (int n0 = (blockIdx.x * CG_WAVES + (int)(t >> 6)) * NB; n0 < p.N;
       n0 += gridDim.x * CG_WAVES * NB) {
    float acc[NB][M];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int m = 0; m < M; ++m) acc[j][m] = 0.f;
    for (int k0 = 0; k0 < p.K; k0 += 512 * U) {
      bf16x8_t wv[NB][U], xv[U][M];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = k0 + u * 512 + lane * 8;
        if (k < p.K) {
#pragma unroll
          for (int j = 0; j < NB; ++j)
            wv[j][u] = n0 + j < p.N ? *(const bf16x8_t*)(p.w + (long)(n0 + j) * p.ldw + k)
                                    : bf16x8_t{};
#pragma unroll
          for (int m = 0; m < M; ++m)
            xv[u][m] = m < rows ? *(const bf16x8_t*)(xs + m * p.K + k) : bf16x8_t{};
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = k0 + u * 512 + lane * 8;
        if (k < p.K) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
#pragma unroll
            for (int j = 0; j < NB; ++j) {
              const float we = bf2f((u16)wv[j][u][e]);
#pragma unroll
              for (int m = 0; m < M; ++m) acc[j][m] += we * bf2f((u16)xv[u][m][e]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
#pragma unroll
      for (int m = 0; m < M; ++m) acc[j][m] = wave_sum(acc[j][m]);
      const int n = n0 + j;
      if (n < p.N && lane < rows) {
        float v = 0.f;
#pragma unroll
        for (int m = 0; m < M; ++m)
          if (m == lane) v = acc[j][m];
        v += p.bias ? p.bias[n] : 0.f;
        if (logits) {
          logits[lane * p.N + n] = v;
        } else {
          v = act_fwd(v, p.act);
          if (p.out_f32)
            ((float*)dst)[(long)lane * p.dst_ld + n] = v;
          else
            ((u16*)dst)[(long)lane * p.dst_ld + n] = f2bf(v);
        }
      }
    }
  }
}

// cs_layer over fp8 weight rows (p.w_scale != nullptr): per neuron fp8_row_sum's order, so the
// outputs are bitwise gemv_fp8.hip's. A lane's 16 codes of each of the NB neurons are one
// 16-byte global load each, all NB x U of them issued before any is used; its 16 bf16 of a row
// are two 16-byte LDS reads, made chunk by chunk as they are used (LDS is near: holding the x of
// U chunks as well would only cost registers). The softmax `logits` get scale * S + bias.
// NB is CS_NB for every row capacity, so chain_stage_workgroups' grid rule holds for both
// forms; NB, U and the registers per row capacity: the file header.
template <int M, int NB, int U>
__device__ __forceinline__ void cs_layer_fp8(const ChainStage& p, const u16* xs, int rows,
                                             char* dst, float* logits) {
  const unsigned t = threadIdx.x;
  const int lane = t & 63;
  const unsigned char* q = (const unsigned char*)p.w;
  for (int n0 = (blockIdx.x * CG_WAVES + (int)(t >> 6)) * NB; n0 < p.N;
       n0 += gridDim.x * CG_WAVES * NB) {
    float acc[NB][M];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int m = 0; m < M; ++m) acc[j][m] = 0.f;
    for (int k0 = 0; k0 < p.K; k0 += C8_CHUNK * U) {
      uint4 qv[NB][U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = k0 + u * C8_CHUNK + lane * 16;
        if (k < p.K) {
#pragma unroll
          for (int j = 0; j < NB; ++j)  // (code 0 decodes to 0; a neuron past N is not written)
            qv[j][u] = n0 + j < p.N ? *(const uint4*)(q + (long)(n0 + j) * p.ldw + k) : uint4{};
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = k0 + u * C8_CHUNK + lane * 16;
        if (k < p.K) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {  // 8 columns at a time: x in registers for 8 only
            bf16x8_t xv[M];
#pragma unroll
            for (int m = 0; m < M; ++m)
              xv[m] = m < rows ? *(const bf16x8_t*)(xs + m * p.K + k + 8 * h) : bf16x8_t{};
#pragma unroll
            for (int j = 0; j < NB; ++j)
              fp8_fma8<M>(h ? qv[j][u].z : qv[j][u].x, h ? qv[j][u].w : qv[j][u].y, xv, acc[j]);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
#pragma unroll
      for (int m = 0; m < M; ++m) acc[j][m] = wave_sum(acc[j][m]);
      const int n = n0 + j;
      if (n < p.N && lane < rows) {
        float v = 0.f;
#pragma unroll
        for (int m = 0; m < M; ++m)
          if (m == lane) v = acc[j][m];
        v = __fmul_rn(p.w_scale[n], v);
        v += p.bias ? p.bias[n] : 0.f;
        if (logits) {
          logits[lane * p.N + n] = v;
        } else {
          v = act_fwd(v, p.act);
          if (p.out_f32)
            ((float*)dst)[(long)lane * p.dst_ld + n] = v;
          else
            ((u16*)dst)[(long)lane * p.dst_ld + n] = f2bf(v);
        }
      }
    }
  }
}

// cs_layer over mxfp4 weight rows (p.w_e8m0 != nullptr): per neuron fp4_row_sum's order for the
// unit B, so the outputs are bitwise gemv_mxfp4.hip's at the same rows and K. A lane's B codes of
// each of the NB neurons are one 8- or 16-byte global load and their block's scale one byte
// load, all NB x U of them issued before any is used; its bf16 of a row are 16-byte LDS reads,
// 8 columns (one code word) at a time as they are used, as cs_layer_fp8. A neuron past N gets
// E = 0, which adds nothing, and is not written. The softmax `logits` get S + bias.
// NB is CS_NB for every row capacity; NB, U, B and the registers: the file header.
template <int M, int NB, int U, int B>
__device__ __forceinline__ void cs_layer_mxfp4(const ChainStage& p, const u16* xs, int rows,
                                               char* dst, float* logits) {
  const unsigned t = threadIdx.x;
  const int lane = t & 63;
  constexpr int CHUNK = 64 * B, W = B / 8;
  const unsigned char* q = (const unsigned char*)p.w;
  for (int n0 = (blockIdx.x * CG_WAVES + (int)(t >> 6)) * NB; n0 < p.N;
       n0 += gridDim.x * CG_WAVES * NB) {
    float acc[NB][M];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int m = 0; m < M; ++m) acc[j][m] = 0.f;
    for (int k0 = 0; k0 < p.K; k0 += CHUNK * U) {
      qword_t<W> qv[NB][U];
      unsigned ev[NB][U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = k0 + u * CHUNK + lane * B;
        if (k < p.K) {  // K % 32 == 0: a lane's B columns are inside K or wholly outside
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            const bool in = n0 + j < p.N;
            qv[j][u] = in ? *(const qword_t<W>*)(q + (long)(n0 + j) * p.ldw + (k >> 1))
                          : qword_t<W>{};
            ev[j][u] = in ? (unsigned)p.w_e8m0[(long)(n0 + j) * p.lde + (k >> 5)] : 0u;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = k0 + u * CHUNK + lane * B;
        if (k < p.K) {
#pragma unroll
          for (int h = 0; h < W; ++h) {  // word h: columns k + 8 h .. k + 8 h + 7
            bf16x8_t xv[M];
#pragma unroll
            for (int m = 0; m < M; ++m)
              xv[m] = m < rows ? *(const bf16x8_t*)(xs + m * p.K + k + 8 * h) : bf16x8_t{};
#pragma unroll
            for (int j = 0; j < NB; ++j)
              fp4_fma8<M>(ev[j][u] ? qv[j][u][h] : 0u, __uint_as_float(ev[j][u] << 23), xv,
                          acc[j]);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
#pragma unroll
      for (int m = 0; m < M; ++m) acc[j][m] = wave_sum(acc[j][m]);
      const int n = n0 + j;
      if (n < p.N && lane < rows) {
        float v = 0.f;
#pragma unroll
        for (int m = 0; m < M; ++m)
          if (m == lane) v = acc[j][m];
        v += p.bias ? p.bias[n] : 0.f;
        if (logits) {
          logits[lane * p.N + n] = v;
        } else {
          v = act_fwd(v, p.act);
          if (p.out_f32)
            ((float*)dst)[(long)lane * p.dst_ld + n] = v;
          else
            ((u16*)dst)[(long)lane * p.dst_ld + n] = f2bf(v);
        }
      }
    }
  }
}

constexpr int CS_NB = 4;  // neurons per wave in flight (chain_stage_kernel, every weight form)

// WT: the layer's weight form -- 0 bf16 (cs_layer), 1 e4m3 codes (cs_layer_fp8), 2 mxfp4
// (cs_layer_mxfp4); everything else is shared.
template <int WT>
__global__ __launch_bounds__(256) void chain_stage_kernel(ChainStage p) {
  extern __shared__ __attribute__((aligned(16))) char cs_lds[];
  __shared__ uint32_t s_cmd[4];  // run, input status, rows, ack failure
  u16* xs = (u16*)cs_lds;
  float* logits = p.act == ACT_SOFTMAX ? (float*)(cs_lds + (long)p.max_rows * p.K * 2) : nullptr;
  const unsigned t = threadIdx.x;
  uint32_t* cnt = p.sync;
  uint32_t* fail = p.sync + p.nslot;
  uint32_t* go = p.sync + 2 * p.nslot;  // workgroup 0: the last request it let through
  uint32_t* ex = go + 1;                // == epoch: this launch ends before request *go + 1
                                        // (ex[1]: why -- 1 stop, 2 idle; ex[2]: the stop
                                        // word read / the idle ticks)
  uint32_t stop_seen = 0;  // workgroup 0: the stop word read after the last request's go
  for (uint32_t seq = p.start_seq + 1;; ++seq) {
    const int slot = (int)(seq % (uint32_t)p.nslot);
    if (t == 0) {
      uint32_t run = 1;
      if (blockIdx.x == 0 && stop_seen) {  // asked to stop while the last request ran
        run = 0;
        __hip_atomic_store(ex + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ex + 2, stop_seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ex, p.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      } else if (blockIdx.x == 0) {
        // the consumer drained the slot this request will reuse -- checked BEFORE the input
        // arrives (it nearly always has: the wait is off the request's path). Bounded: a stuck
        // consumer is reported downstream as DEADLINE naming it, no rows are written.
        // The stop word lives in host memory (a read crosses the host link): looked at every
        // ~20 us of waiting, not every poll of a (local) flag -- in this ack wait too, so a
        // stage whose consumer is stuck still returns promptly when asked.
        bool ack_ok = true;
        unsigned long long t_stop = wall_clock64();
        {
          const unsigned long long ta = t_stop;
          while ((int)(__hip_atomic_load(p.ack, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) -
                       (seq - (uint32_t)p.nslot)) < 0) {
            const unsigned long long now = wall_clock64();
            if (now - t_stop > 2000) {
              t_stop = now;
              const uint32_t sv = __hip_atomic_load(p.stop, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_SYSTEM);
              if (sv) {  // the exit reason is recorded as on the input-wait path
                run = 0;
                __hip_atomic_store(ex + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(ex + 2, sv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
              }
            }
            if (now - ta > p.timeout_ticks) {
              ack_ok = false;
              break;
            }
            __builtin_amdgcn_s_sleep(1);
          }
        }
        const unsigned long long t0 = wall_clock64();
        for (; run;) {
          if ((int)(__hip_atomic_load(p.in_flags + slot, __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_SYSTEM) - seq) >= 0)
            break;
          const unsigned long long now = wall_clock64();
          if (now - t_stop > 2000) {
            t_stop = now;
            const uint32_t sv = __hip_atomic_load(p.stop, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_SYSTEM);
            if (sv) {
              run = 0;
              __hip_atomic_store(ex + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              __hip_atomic_store(ex + 2, sv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              break;
            }
          }
          if (now - t0 > p.idle_ticks) {
            run = 0;
            __hip_atomic_store(ex + 1, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ex + 2, (uint32_t)(now - t0), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            break;
          }
          __builtin_amdgcn_s_sleep(1);
        }
        if (run) {
          __hip_atomic_store(fail + slot, ack_ok ? 0u : 1u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(go, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
          // one look at the stop word per request, off the request's path (the other
          // workgroups are already computing): back-to-back requests never wait the ~20 us
          // the polls above need before they read it, so a paused() chain would otherwise
          // run until its hop timeout
          stop_seen = __hip_atomic_load(p.stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        } else {
          __hip_atomic_store(ex, p.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
      } else {
        // the other workgroups follow workgroup 0's decision (it alone polls the input flag
        // and owns the idle / stop exit, so every workgroup leaves at the same request)
        for (;;) {
          if ((int)(__hip_atomic_load(go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - seq) >= 0)
            break;
          if (__hip_atomic_load(ex, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p.epoch) {
            run = 0;
            break;
          }
          __builtin_amdgcn_s_sleep(1);
        }
      }
      if (run) {
        // no acquire fence: it would invalidate the L2 that keeps this stage's weights resident
        // between requests. The header and rows are read with system-scope loads instead
        // (they bypass every cache level), issued after the flag / go was seen.
        s_cmd[1] = __hip_atomic_load(p.in_hdrs + 2 * slot, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_SYSTEM);
        s_cmd[2] = __hip_atomic_load(p.in_hdrs + 2 * slot + 1, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_SYSTEM);
        s_cmd[3] = __hip_atomic_load(fail + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      s_cmd[0] = run;
    }
    __syncthreads();
    if (!s_cmd[0]) break;  // uniform: the launch ends here
    const uint32_t in_st = s_cmd[1];
    const int rows = (int)s_cmd[2];
    const bool rows_ok = rows >= 1 && rows <= p.max_rows;
    const uint32_t ack_fail = s_cmd[3];
    const bool compute = (in_st & 0xffu) == 0u && ack_fail == 0u && rows_ok;
    char* dst = p.dst + slot * p.dst_slot_bytes;
    if (compute) {
      const u16* src = p.in_slots + (long)slot * p.max_rows * p.ldx;
      const int cpr = p.K >> 2;  // 8-byte words per row
      for (int i = t; i < rows * cpr; i += blockDim.x) {
        const int r = i / cpr, c = i - r * cpr;
        *(uint64_t*)(xs + r * p.K + 4 * c) = __hip_atomic_load(
            (const uint64_t*)(src + r * p.ldx + 4 * c), __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_SYSTEM);
      }
      __syncthreads();
      if constexpr (WT == 1) {
        switch (rows) {
          case 1: cs_layer_fp8<1, CS_NB, 4>(p, xs, rows, dst, logits); break;
          case 2: cs_layer_fp8<2, CS_NB, 4>(p, xs, rows, dst, logits); break;
          case 3:
          case 4: cs_layer_fp8<4, CS_NB, 2>(p, xs, rows, dst, logits); break;
          default: cs_layer_fp8<8, CS_NB, 2>(p, xs, rows, dst, logits); break;
        }
      } else if constexpr (WT == 2) {
        const bool whole = p.K >= C4_WHOLE_MIN_K;  // 1 and 2 rows: gemv_mxfp4's unit rule
        switch (rows) {
          case 1:
            if (whole) cs_layer_mxfp4<1, CS_NB, 2, 32>(p, xs, rows, dst, logits);
            else cs_layer_mxfp4<1, CS_NB, 4, 16>(p, xs, rows, dst, logits);
            break;
          case 2:
            if (whole) cs_layer_mxfp4<2, CS_NB, 2, 32>(p, xs, rows, dst, logits);
            else cs_layer_mxfp4<2, CS_NB, 4, 16>(p, xs, rows, dst, logits);
            break;
          case 3:
          case 4: cs_layer_mxfp4<4, CS_NB, 2, 16>(p, xs, rows, dst, logits); break;
          // (U = 2 at 8 rows made the whole kernel 256 VGPRs + 12 AGPRs: 1 wave/SIMD)
          default: cs_layer_mxfp4<8, CS_NB, 1, 16>(p, xs, rows, dst, logits); break;
        }
      } else {
        switch (rows) {
          case 1: cs_layer<1, CS_NB>(p, xs, rows, dst, logits); break;
          case 2: cs_layer<2, CS_NB>(p, xs, rows, dst, logits); break;
          case 3:
          case 4: cs_layer<4, CS_NB>(p, xs, rows, dst, logits); break;
          default: cs_layer<8, CS_NB>(p, xs, rows, dst, logits); break;
        }
      }
      if (logits) {  // row softmax (one workgroup): a wave per row
        __syncthreads();
        const int lane = t & 63;
        for (int m = (int)(t >> 6); m < rows; m += CG_WAVES) {
          float mx = -INFINITY;
          for (int n = lane; n < p.N; n += 64) mx = fmaxf(mx, logits[m * p.N + n]);
          mx = wave_max(mx);
          float s = 0.f;
          for (int n = lane; n < p.N; n += 64) s += __expf(logits[m * p.N + n] - mx);
          s = wave_sum(s);
          const float inv = 1.f / s;
          for (int n = lane; n < p.N; n += 64) {
            const float v = __expf(logits[m * p.N + n] - mx) * inv;
            if (p.out_f32)
              ((float*)dst)[(long)m * p.dst_ld + n] = v;
            else
              ((u16*)dst)[(long)m * p.dst_ld + n] = f2bf(v);
          }
        }
      }
    }
    // this thread's rows are visible before the workgroup counts in: a release-only fence
    // (a full __threadfence_system would also invalidate the L2 holding the weights)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    __syncthreads();
    if (t == 0) {
      // acq_rel at agent scope: every workgroup's release (fence above) synchronizes with
      // the last arriver's acquire, so the rows it publishes below are ordered by the memory
      // model, not only by each writer's own fence. An agent-scope acquire invalidates the
      // per-CU caches only, not the L2 that keeps this stage's weights resident
      const uint32_t prev = __hip_atomic_fetch_add(cnt + slot, 1u, __ATOMIC_ACQ_REL,
                                                   __HIP_MEMORY_SCOPE_AGENT);
      if (prev == gridDim.x - 1) {  // the last workgroup: every row of the request landed
        uint32_t st = 0u;
        if (in_st & 0xffu) st = in_st;  // an upstream failure travels on unchanged
        else if (ack_fail) st = CHAIN_DEADLINE | ((uint32_t)(p.stage + 1) << 8);
        else if (!rows_ok) st = CHAIN_INTERNAL | ((uint32_t)p.stage << 8);
        __hip_atomic_store(cnt + slot, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t* hdr = p.dst_hdr + slot * p.hdr_stride;
        __hip_atomic_store(hdr, st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(hdr + 1, (uint32_t)(rows_ok ? rows : 0), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        __hip_atomic_store(p.next_flags + slot, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(p.prev_ack, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(p.done, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

__global__ void chain_signal_kernel(uint32_t* flag, uint32_t value) {
  const unsigned l = threadIdx.x;
  if (l == 0) {
    __threadfence_system();
    __hip_atomic_store(flag + l, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ __launch_bounds__(256) void p2p_copy_signal_seq_kernel(
    const uint4* __restrict__ src, uint4* __restrict__ dst, long n16,
    const unsigned char* __restrict__ src_t, unsigned char* __restrict__ dst_t, int tail,
    uint32_t* flag, const uint32_t* seq, int delta, uint32_t* counter) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n16; i += (long)gridDim.x * 256)
    dst[i] = src[i];
  if (blockIdx.x == 0 && (int)threadIdx.x < tail) dst_t[threadIdx.x] = src_t[threadIdx.x];
  __threadfence_system();  // this thread's part is visible before the workgroup counts in
  __syncthreads();
  const unsigned t = threadIdx.x;
  if (t == 0) {
    const uint32_t prev = __hip_atomic_fetch_add(counter + t, 1u, __ATOMIC_ACQ_REL,
                                                 __HIP_MEMORY_SCOPE_AGENT);
    if (prev == gridDim.x - 1) {  // the last workgroup: every part has landed
      __hip_atomic_store(counter + t, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t v = __hip_atomic_load(seq + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __threadfence_system();
      __hip_atomic_store(flag + t, v + (uint32_t)delta, __ATOMIC_RELEASE,
                         __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

int p2p_copy_signal_seq(void* dst, const void* src, size_t bytes, uint32_t* flag,
                        const uint32_t* seq, int delta, uint32_t* counter, hipStream_t stream) {
  if ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) return -1;
  if (!flag || !seq || !counter || misaligned4(flag) || misaligned4(counter)) return -1;
  const long n16 = (long)(bytes / 16);
  const int tail = (int)(bytes % 16);
  const int grid = (int)std::min<long>(std::max<long>(1, (n16 + 255) / 256), 2048);
  hipLaunchKernelGGL(p2p_copy_signal_seq_kernel, dim3(grid), dim3(256), 0, stream,
                     reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), n16,
                     reinterpret_cast<const unsigned char*>(src) + n16 * 16,
                     reinterpret_cast<unsigned char*>(dst) + n16 * 16, tail, flag, seq, delta,
                     counter);
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

unsigned long long chain_ticks(double seconds) {
  static int rate_khz = [] {  // wall_clock64 ticks per ms (100 MHz on gfx9)
    int r = 0, dev = 0;
    if (hipGetDevice(&dev) == hipSuccess)
      (void)hipDeviceGetAttribute(&r, hipDeviceAttributeWallClockRate, dev);
    return r > 0 ? r : 100000;
  }();
  return (unsigned long long)(std::max(0.0, seconds) * 1e3 * (double)rate_khz);
}


int chain_wait(const uint32_t* flag, uint32_t target, uint32_t* err, double timeout_s,
               hipStream_t stream) {
  if (!flag || !err || misaligned4(flag) || misaligned4(err)) return -1;
  hipLaunchKernelGGL(chain_wait_kernel, dim3(1), dim3(64), 0, stream, flag, target, err,
                     chain_ticks(timeout_s));
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

int chain_recv(const ChainRecv& p, hipStream_t stream) {
  if (!p.flag || !p.err || !p.dst_hdr || !p.slot_hdr || misaligned4(p.flag)) return -1;
  if (p.rows < 0 || p.row_bytes % 16 || p.slot_ld % 16 || p.dst_ld % 16 ||
      misaligned16(p.slot) || misaligned16(p.dst))
    return -2;
  hipLaunchKernelGGL(chain_recv_kernel, dim3(1), dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

int chain_send(const ChainSend& p, hipStream_t stream) {
  if (!p.next_flag || !p.dst_hdr || !p.err || misaligned4(p.next_flag)) return -1;
  if (p.rows < 0 || p.row_bytes % 16 || p.src_ld % 16 || p.dst_ld % 16 ||
      misaligned16(p.src) || misaligned16(p.dst))
    return -2;
  hipLaunchKernelGGL(chain_send_kernel, dim3(1), dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

int chain_gemv_send(const ChainGemvSend& p, hipStream_t stream) {
  if (!p.next_flag || !p.dst_hdr || !p.err || !p.counter || !p.dst || !p.x || !p.w ||
      misaligned4(p.next_flag) || misaligned4(p.counter))
    return -1;
  const bool fp4 = p.w_e8m0 != nullptr;  // (its ldw counts bytes of two codes each)
  if (p.rows < 1 || p.rows > GEMV_MAX_ROWS || p.N < 1 || p.K < 8 || p.K % 8 || p.ldx < p.K ||
      (!fp4 && p.ldw < p.K) || p.ldx % 8 || p.ldw % 8 || p.dst_ld < p.N || misaligned16(p.x) ||
      misaligned16(p.w))
    return -2;
  // fp8 rows: a lane's 16 codes are one aligned 16-byte load (ldw counts bytes)
  if (p.w_scale && (p.K % 16 || p.ldw % 16)) return -2;
  if (fp4 && bad_mxfp4(p.w_scale, p.K, p.ldw, p.lde)) return -2;
  // the folded receive makes every workgroup wait on the input flag: at most CG_RECV_WG of
  // them, so a node's worth of waiting stages (a one-GPU rehearsal puts 8 on one GPU) stays
  // far below what the GPU holds at once
  constexpr int CG_RECV_WG = 64;
  const int wg = (p.N + CG_WAVES - 1) / CG_WAVES;
  const dim3 grid(p.in_flag ? std::min(wg, CG_RECV_WG) : wg), block(256);
#define DNN_CG4(MM, BB)                                                                       \
  if (p.out_f32)                                                                              \
    hipLaunchKernelGGL((chain_gemv_send_kernel<MM, true, false, BB>), grid, block, 0, stream, \
                       p);                                                                    \
  else                                                                                        \
    hipLaunchKernelGGL((chain_gemv_send_kernel<MM, false, false, BB>), grid, block, 0,        \
                       stream, p);
  if (fp4) {  // the unit of gemv_mxfp4: a whole block for 1 and 2 rows from C4_WHOLE_MIN_K on
    const bool whole = p.K >= C4_WHOLE_MIN_K;
    switch (p.rows) {
      case 1:
        if (whole) { DNN_CG4(1, 32) } else { DNN_CG4(1, 16) }
        break;
      case 2:
        if (whole) { DNN_CG4(2, 32) } else { DNN_CG4(2, 16) }
        break;
      case 3:
      case 4: DNN_CG4(4, 16) break;
      default: DNN_CG4(8, 16) break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -9;
  }
#undef DNN_CG4
#define DNN_CG(MM)                                                                            \
  if (p.w_scale && p.out_f32)                                                                 \
    hipLaunchKernelGGL((chain_gemv_send_kernel<MM, true, true>), grid, block, 0, stream, p);  \
  else if (p.w_scale)                                                                         \
    hipLaunchKernelGGL((chain_gemv_send_kernel<MM, false, true>), grid, block, 0, stream, p); \
  else if (p.out_f32)                                                                         \
    hipLaunchKernelGGL((chain_gemv_send_kernel<MM, true>), grid, block, 0, stream, p);        \
  else                                                                                        \
    hipLaunchKernelGGL((chain_gemv_send_kernel<MM, false>), grid, block, 0, stream, p);
  switch (p.rows) {
    case 1: DNN_CG(1) break;
    case 2: DNN_CG(2) break;
    case 3:
    case 4: DNN_CG(4) break;
    default: DNN_CG(8) break;
  }
#undef DNN_CG
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

int chain_stage_workgroups(int N, int act) {
  if (act == ACT_SOFTMAX) return 1;  // the row pass needs every logit in one workgroup
  // a neuron group (CS_NB neurons) per wave, at most 64 workgroups: a one-GPU rehearsal keeps
  // 7 persistent stages resident at once (448 workgroups, far below the GPU's ~2048)
  return std::max(1, std::min(64, (N + CG_WAVES * CS_NB - 1) / (CG_WAVES * CS_NB)));
}

int chain_stage_run(const ChainStage& p, int workgroups, int share, hipStream_t stream) {
  if (!p.in_flags || !p.in_hdrs || !p.in_slots || !p.prev_ack || !p.w || !p.dst || !p.dst_hdr ||
      !p.next_flags || !p.ack || !p.stop || !p.done || !p.sync || misaligned4(p.in_flags) ||
      misaligned4(p.sync) || misaligned4(p.next_flags) || misaligned4(p.dst_hdr))
    return -1;
  const bool fp4 = p.w_e8m0 != nullptr;
  if (p.N < 1 || p.K < 8 || p.K % 8 || p.ldx < p.K || p.ldx % 8 || (!fp4 && p.ldw < p.K) ||
      p.ldw % 8 || p.dst_ld < p.N || p.nslot < 2 || p.max_rows < 1 ||
      p.max_rows > GEMV_MAX_ROWS || misaligned16(p.in_slots) || misaligned16(p.w) || p.epoch == 0)
    return -2;
  if (p.w_scale && (p.K % 16 || p.ldw % 16)) return -2;  // fp8 rows, as chain_gemv_send
  if (fp4 && bad_mxfp4(p.w_scale, p.K, p.ldw, p.lde)) return -2;
  // (the occupancy below is taken from the kernel that is launched: each form has its own)
  const auto kernel = fp4 ? chain_stage_kernel<2>
                          : p.w_scale ? chain_stage_kernel<1> : chain_stage_kernel<0>;
  const long lds = (long)p.max_rows * p.K * 2 +
                   (p.act == ACT_SOFTMAX ? (long)p.max_rows * p.N * 4 : 0);
  if (lds > 64 * 1024) return -3;  // rows staged in LDS: K (and a softmax's N) bounded
  if (workgroups < 1 || (p.act == ACT_SOFTMAX && workgroups != 1)) return -4;
  // every workgroup of every persistent stage on this GPU must be resident at once (a request
  // completes only when all of a stage's workgroups count in, and resident ones never yield):
  // `share` stages split what the GPU holds, with a quarter kept for everything else
  int per_cu = 0, dev = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, (size_t)lds) !=
          hipSuccess ||
      hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return -9;
  const int cap = std::max(1, per_cu * cus * 3 / 4 / std::max(1, share));
  workgroups = std::min(workgroups, cap);
  hipLaunchKernelGGL(kernel, dim3(workgroups), dim3(256), (size_t)lds, stream, p);
  return hipGetLastError() == hipSuccess ? workgroups : -9;
}

int chain_signal(uint32_t* flag, uint32_t value, hipStream_t stream) {
  if (!flag || misaligned4(flag)) return -1;
  hipLaunchKernelGGL(chain_signal_kernel, dim3(1), dim3(64), 0, stream, flag, value);
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

}  // namespace dnn
