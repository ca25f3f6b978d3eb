// Fused stage forward for requests of 1..8 rows: all L layers of a bf16 serving stage in ONE
// launch (interface and math: stage_gemv.hpp). The per-layer path is one gemv_kernel launch per
// layer (+ softmax_rows); at these sizes every one of them is a launch and two memory round
// trips long, whatever it computes. This kernel keeps gemv's work split and gemv's sums -- one
// wave per output neuron, the lane -> k mapping and the per-lane accumulation order of
// gemv_kernel<M> -- so its output is bit for bit the per-layer chain's.
//
// Design.
//   * Phase A, the head layer on the whole chip. The first layer holds most of a stage's
//     bytes, so it runs as gemv_kernel does: grid = N1 / SG_WAVES workgroups, wave = neuron,
//     the weight row in 16-byte loads (chunks of 512 = 64 lanes x 8 in k order, U chunks loaded
//     before any is used; U = 4 as in gemv, 2 for the 8-row template to stay inside the
//     register budget -- batching only, the sum order is the same), rows innermost, wave_sum,
//     bias, act_fwd, f2bf. Lane m < rows stores row m's bf16 output into the global workspace
//     h1[8][N1].
//   * Hand-off, last arriver, nobody waits. Every thread: release fence at agent scope;
//     __syncthreads; thread 0: fetch_add (ACQ_REL, agent scope) on the 32-bit counter. A
//     workgroup that does not read gridDim.x - 1 exits. The one that does resets the counter
//     (the next launch needs no memset) and goes on alone. There is no spin, no flag poll and
//     no cooperative launch: a workgroup never depends on another being resident.
//   * Why the last arriver sees h1 across XCDs. An MI355X has one L2 per XCD and they are not
//     kept coherent by hardware for ordinary device memory; the memory model is implemented by
//     the fences. The agent-scope RELEASE of a storing thread writes its XCD's dirty L2 lines
//     back to memory before its workgroup's counter increment can be performed (the increment
//     itself executes at the memory side, device-coherent). The fetch_add chain on the counter
//     orders every workgroup's release before the last arriver's acquire. After the barrier
//     that publishes thread 0's result, EVERY thread of the last workgroup executes its own
//     agent-scope ACQUIRE fence before its first read of h1: that invalidates the CU's vector
//     L1 and the non-local lines of this XCD's L2, so the reads that follow are served from
//     memory, where the released stores are. h1 is read with plain vector loads after that
//     fence and never before it in this launch.
//   * Phase B, the tail in one workgroup. h1 -> LDS, then layers 1..L-1 with the activations
//     ping-ponging between two LDS buffers of 8 x 512 bf16 (layer l reads buffer (l - 1) & 1
//     and writes l & 1; one barrier per layer). Wave w takes neurons w, w + SG_WAVES, ... in
//     batches of NB = 8 (1 or 2 rows) or 4. A lane's 8 x-columns of the <= 8 rows are read from LDS once per layer
//     and stay in registers; weight rows come from global memory as one 16-byte load per lane
//     (K <= 512: gemv's single chunk, lanes with 8 lane >= K idle as there). The tail is
//     latency-bound, so weight loads run one batch AHEAD of the sums in two register
//     buffers that take turns, across layer boundaries too (weights do not depend on
//     activations): 2 NB = 16 or 8 weight rows in flight per wave, 128 or 64 per workgroup.
//   * Last layer: bf16 or fp32 to y; or, softmax over <= 64 classes, fp32 logits to LDS and
//     then one wave per row in softmax_rows_kernel<1>'s order (column = lane, wave_max,
//     __expf(x - mx), wave_sum, x * (1 / se)).
//   * Workgroup size 512 (8 waves): 256 registers per lane, which holds the 8-row template's
//     double buffer (32) + x (32) + 4 x 8 sums without scratch; 1024 threads would leave 128.
//     Figures: DESIGN.md "Fused stage GEMV".
#include "common.hpp"
#include "gemv.hpp"
#include "stage_gemv.hpp"

namespace dnn {
namespace {

constexpr int SG_WAVES = 8;            // waves (= neurons in flight) per workgroup
constexpr int SG_NT = 64 * SG_WAVES;   // threads
// tail: neurons of a wave per batch, from the register budget (two batches of weight rows in
// flight: 4 registers a row; M sums a neuron)
template <int M>
constexpr int sg_nb() { return M <= 2 ? 8 : 4; }
constexpr int SG_LD = STAGE_GEMV_MAX_WIDTH;  // LDS activation row stride (elements)
static_assert(64 % (SG_WAVES * sg_nb<1>()) == 0 && 64 % (SG_WAVES * sg_nb<8>()) == 0,
              "a batch never straddles the end of a layer");

// gemv_kernel's per-lane sum over one chunk: elements in order, rows innermost. Only the ORDER
// of the additions matters for the bits: a product of two bf16 values has at most 16
// significant bits and is exact in fp32, so it is the same number whether the compiler
// contracts it into an FMA or not (it does both, in gemv_kernel too).
template <int M>
struct SgAcc {
  float a[M];
};
template <int M>
struct SgX {
  bf16x8_t v[M];
};
template <int M>
__device__ __forceinline__ SgAcc<M> sg_fma(SgAcc<M> acc, bf16x8_t wv, SgX<M> xv) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float we = bf2f((u16)wv[e]);
#pragma unroll
    for (int m = 0; m < M; ++m) acc.a[m] += we * bf2f((u16)xv.v[m][e]);
  }
  return acc;
}

// gemv_kernel's epilogue: after the wave sums lane m holds row m's act(sum + bias).
template <int M>
__device__ __forceinline__ float sg_out(SgAcc<M>& acc, int lane, const float* bias, int n,
                                        int act) {
#pragma unroll
  for (int m = 0; m < M; ++m) acc.a[m] = wave_sum(acc.a[m]);
  float v = 0.f;
#pragma unroll
  for (int m = 0; m < M; ++m)
    if (m == lane) v = acc.a[m];
  v += bias ? bias[n] : 0.f;
  return act_fwd(v, act);
}

// Phase A: this wave's neuron of layer 0 into the workspace.
template <int M>
__device__ __forceinline__ void sg_head(const StageGemvParams& p) {
  constexpr int U = M <= 4 ? 4 : 2;
  const StageGemvLayer& ly = p.layer[0];
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * SG_WAVES + (threadIdx.x >> 6);  // < N: grid = N / SG_WAVES
  const int K = p.K0, rows = p.rows;
  const u16* wr = ly.W + (long)n * ly.ldw;
  SgAcc<M> acc;
#pragma unroll
  for (int m = 0; m < M; ++m) acc.a[m] = 0.f;
  for (int k0 = 0; k0 < K; k0 += 512 * U) {
    bf16x8_t wv[U];
    SgX<M> xv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + u * 512 + lane * 8;
      if (k < K) {
        wv[u] = *(const bf16x8_t*)(wr + k);
#pragma unroll
        for (int m = 0; m < M; ++m)
          xv[u].v[m] = m < rows ? *(const bf16x8_t*)(p.x + m * p.ldx + k) : bf16x8_t{};
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + u * 512 + lane * 8;
      if (k < K) acc = sg_fma<M>(acc, wv[u], xv[u]);
    }
  }
  const float v = sg_out<M>(acc, lane, ly.bias, n, ly.act);
  if (lane < rows) p.work[lane * ly.N + n] = f2bf(v);
}

// Phase B: layers 1..L-1 in this workgroup. hs: two activation buffers [8][SG_LD], buffer 0
// holding h1; lg: [8][64] fp32 logits of a softmax last layer.
template <int M>
__device__ __forceinline__ void sg_tail(const StageGemvParams& p, u16* hs, float* lg) {
  constexpr int NB = sg_nb<M>();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows = p.rows, kl = lane * 8;
  const bool softmax = p.layer[p.L - 1].act == ACT_SOFTMAX;
  // batch b of layer l: the wave's neurons wave + SG_WAVES (b NB + j), j < NB
  auto load = [&](int l, int b, bf16x8_t (&w)[NB]) {
    const StageGemvLayer& ly = p.layer[l];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int n = wave + SG_WAVES * (b * NB + j);
      w[j] = kl < ly.K ? *(const bf16x8_t*)(ly.W + (long)n * ly.ldw + kl) : bf16x8_t{};
    }
  };
  SgX<M> xv;
  int l = 1, b = 0;
  // One batch: start the loads of the NEXT batch into `nxt` (across the layer boundary too),
  // then sum this one from `cur`. Returns false after the last batch. Every wave walks the same
  // (l, b) sequence, so the barriers are uniform.
  auto step = [&](const bf16x8_t (&cur)[NB], bf16x8_t (&nxt)[NB]) -> bool {
    const StageGemvLayer& ly = p.layer[l];
    int nl = l, nb = b + 1;
    if (nb * (SG_WAVES * NB) >= ly.N) {
      nl = l + 1;
      nb = 0;
    }
    if (nl < p.L) load(nl, nb, nxt);
    const bool last = l == p.L - 1;
    u16* hout = hs + (l & 1) * 8 * SG_LD;
    if (b == 0) {
      __syncthreads();  // the layer before (or the h1 copy) wrote its buffer, and every wave
                        // is done reading the buffer this layer overwrites
      const u16* hin = hs + ((l - 1) & 1) * 8 * SG_LD;
#pragma unroll
      for (int m = 0; m < M; ++m)
        xv.v[m] = m < rows && kl < ly.K ? *(const bf16x8_t*)(hin + m * SG_LD + kl) : bf16x8_t{};
    }
    SgAcc<M> acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
#pragma unroll
      for (int m = 0; m < M; ++m) acc[j].a[m] = 0.f;
      if (kl < ly.K) acc[j] = sg_fma<M>(acc[j], cur[j], xv);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int n = wave + SG_WAVES * (b * NB + j);
      const float v = sg_out<M>(acc[j], lane, ly.bias, n,
                                last && softmax ? (int)ACT_LINEAR : ly.act);
      if (lane < rows) {
        if (!last) hout[lane * SG_LD + n] = f2bf(v);
        else if (softmax) lg[lane * 64 + n] = v;
        else if (p.out_f32) ((float*)p.y)[(long)lane * p.ldy + n] = v;
        else ((u16*)p.y)[(long)lane * p.ldy + n] = f2bf(v);
      }
    }
    l = nl;
    b = nb;
    return nl < p.L;
  };
  // two register buffers taking turns (no copy between them: a copy would wait for the loads)
  bf16x8_t wa[NB], wb[NB];
  load(l, b, wa);
  while (step(wa, wb) && step(wb, wa)) {
  }
  if (!softmax) return;  // (block-uniform)
  __syncthreads();
  for (int r = wave; r < rows; r += SG_WAVES) {  // softmax_rows_kernel<1>, row r
    float x = lane < p.n_cls ? lg[r * 64 + lane] : -INFINITY;
    const float mx = wave_max(fmaxf(-INFINITY, x));
    x = __expf(x - mx);
    const float se = wave_sum(x);
    const float inv = 1.f / se;
    if (lane < p.n_cls) ((float*)p.y)[(long)r * p.ldy + lane] = x * inv;
  }
}

template <int M>
__global__ __launch_bounds__(SG_NT) void stage_gemv_kernel(const StageGemvParams p) {
  __shared__ __attribute__((aligned(16))) u16 hs[2 * 8 * SG_LD];
  __shared__ float lg[8 * 64];
  __shared__ uint32_t s_last;
  sg_head<M>(p);
  // this thread's row of h1 is released before the workgroup counts in
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __syncthreads();
  const unsigned t = threadIdx.x;
  if (t == 0) {
    const uint32_t prev = __hip_atomic_fetch_add(p.counter + t, 1u, __ATOMIC_ACQ_REL,
                                                 __HIP_MEMORY_SCOPE_AGENT);
    const bool last = prev == gridDim.x - 1;  // every workgroup's h1 has been released
    if (last)  // the next launch on this workspace starts from 0 again
      __hip_atomic_store(p.counter + t, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = last ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;  // uniform; nobody waits for anybody
  // every reading thread acquires for itself (file header: what that does across XCDs)
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const int N1 = p.layer[0].N, vpr = N1 >> 3;  // 16-byte vectors per row
  for (int i = t; i < p.rows * vpr; i += SG_NT) {
    const int r = i / vpr, c = i - r * vpr;
    *(bf16x8_t*)(hs + r * SG_LD + 8 * c) = *(const bf16x8_t*)(p.work + r * N1 + 8 * c);
  }
  sg_tail<M>(p, hs, lg);  // (its first barrier publishes the copy)
}

}  // namespace

const char* stage_gemv_error(int code) {
  switch (code) {
    case 0: return "ok";
    case -1: return "sizes: 1 <= rows <= 8, K0 % 8 == 0, 2 <= L <= 8, every width after the "
                    "input % 64 == 0 and <= 512, K of a layer == N of the layer before, softmax "
                    "N == 64 with 1 <= n_cls <= 64";
    case -2: return "a leading dimension is smaller than its row or not a multiple of 8 elements";
    case -3: return "null operand (x, a weight, y, the workspace or the counter)";
    case -4: return "activation: linear / relu / sigmoid per layer, softmax on the last layer "
                    "only and into fp32";
    case -5: return "alignment: x, the weights and the workspace 16 bytes, the counter 4, y its "
                    "element size";
    case -9: return "launch failed";
    default: return "unknown error";
  }
}

int stage_gemv(const StageGemvParams& p, hipStream_t stream) {
  if (p.L < 2 || p.L > STAGE_GEMV_MAX_LAYERS) return -1;
  if (p.rows < 1 || p.rows > GEMV_MAX_ROWS) return -1;
  if (p.K0 < 8 || p.K0 % 8 || p.K0 > (1 << 30)) return -1;
  if (!p.x || !p.y || !p.work || !p.counter) return -3;
  if (p.ldx < p.K0 || p.ldx % 8) return -2;
  if ((((uintptr_t)p.x) | ((uintptr_t)p.work)) & 15) return -5;
  if (((uintptr_t)p.counter) & 3) return -5;
  int K = p.K0;
  for (int l = 0; l < p.L; ++l) {
    const StageGemvLayer& ly = p.layer[l];
    if (ly.N < 64 || ly.N % 64 || ly.N > STAGE_GEMV_MAX_WIDTH || ly.K != K) return -1;
    if (!ly.W) return -3;
    if (ly.ldw < K || ly.ldw % 8) return -2;
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
  if (((uintptr_t)p.y) % (p.out_f32 ? 4 : 2)) return -5;
  const dim3 grid(p.layer[0].N / SG_WAVES), block(SG_NT);
  switch (p.rows) {
    case 1: hipLaunchKernelGGL(stage_gemv_kernel<1>, grid, block, 0, stream, p); break;
    case 2: hipLaunchKernelGGL(stage_gemv_kernel<2>, grid, block, 0, stream, p); break;
    case 3:  // rows 3..4 on the 4-row kernel, 5..8 on the 8-row one (guarded by `rows`)
    case 4: hipLaunchKernelGGL(stage_gemv_kernel<4>, grid, block, 0, stream, p); break;
    default: hipLaunchKernelGGL(stage_gemv_kernel<8>, grid, block, 0, stream, p); break;
  }
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

}  // namespace dnn
