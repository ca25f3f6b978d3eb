// Fused stage forward (csrc/kernels/stage_fwd.hip): all L layers of a serving stage on bf16
// weights in ONE launch. A workgroup owns a tile of rows and walks the layers; the hidden
// activations live in LDS as bf16 and never reach global memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dnn {

constexpr int STAGE_FWD_MAX_LAYERS = 8;
constexpr int STAGE_FWD_MAX_WIDTH = 512;  // widest padded OUTPUT of a layer (K0 is not bound)
constexpr int STAGE_FWD_TILES = 2;        // tile 1 / 2 = 16 / 64 rows per workgroup

struct StageFwdLayer {
  const uint16_t* W;  // [N][K] bf16, K-major: the stage's resident padded weight, read in place
  long ldw;           // row stride in elements, % 8 == 0
  const float* bias;  // [N] fp32, or null
  int N;              // padded output width: % 64 == 0, <= STAGE_FWD_MAX_WIDTH
  int K;              // padded input width: K0 for layer 0, else N of the layer before
  int act;            // Act code; ACT_SOFTMAX on the last layer only
};

// h_0 = x; h_{l+1} = bf16(act_l(h_l . W_l^T + b_l)) for l < L - 1, each hidden activation
// rounded to bf16 once, exactly where the per-layer path rounds it;
// y = act_{L-1}(h_{L-1} . W_{L-1}^T + b_{L-1}) as bf16 or fp32 (out_f32), rows < M, every one
// of the last layer's N columns and nothing beyond them. With a softmax last layer (N == 64,
// 1 <= n_cls <= 64, out_f32): y[m][c] = the fp32 probability of class c over the first n_cls
// logits, for c < n_cls, and nothing beyond (the contract of softmax_rows).
struct StageFwdParams {
  const uint16_t* x;  // [M][K0] bf16, 16-byte aligned rows
  long ldx;           // % 8 == 0
  int M, K0;          // any M >= 1; K0 % 64 == 0
  int L;              // 2 .. STAGE_FWD_MAX_LAYERS
  StageFwdLayer layer[STAGE_FWD_MAX_LAYERS];
  void* y;
  long ldy;
  int out_f32;
  int n_cls;  // softmax last layer only
  int tile;   // 0 = chosen from M (stage_fwd.hip); 1..STAGE_FWD_TILES force one
};

// 0, or -1 (sizes: M, K0, L, a width, n_cls), -2 (leading dimensions), -3 (null operand), -4
// (activation: unknown, a hidden softmax, or a softmax that is not fp32), -5 (alignment of x,
// a weight or y), -6 (tile), -7 (more row tiles than a grid holds), -9 (launch failed). A
// geometry the kernel does not serve returns its code and launches nothing.
int stage_fwd(const StageFwdParams& p, hipStream_t stream);
const char* stage_fwd_error(int code);

}  // namespace dnn
