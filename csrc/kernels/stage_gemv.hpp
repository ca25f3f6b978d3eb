// Fused stage forward for serving requests of 1..8 rows (csrc/kernels/stage_gemv.hip): all L
// layers of a bf16 stage in ONE launch, bit for bit the chain of gemv_bf16 launches (+
// softmax_rows) it replaces. The first layer runs on the whole chip, one wave per neuron; the
// workgroup that arrives last walks the other layers alone with the activations in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dnn {

constexpr int STAGE_GEMV_MAX_LAYERS = 8;
constexpr int STAGE_GEMV_MAX_WIDTH = 512;  // widest padded OUTPUT of a layer (K0 is not bound)

struct StageGemvLayer {
  const uint16_t* W;  // [N][K] bf16, K-major: the stage's resident padded weight, read in place
  long ldw;           // row stride in elements, % 8 == 0
  const float* bias;  // [N] fp32, or null
  int N;              // padded output width: % 64 == 0, <= STAGE_GEMV_MAX_WIDTH
  int K;              // padded input width: K0 for layer 0, else N of the layer before
  int act;            // Act code; ACT_SOFTMAX on the last layer only
};

// h_0 = x; h_{l+1} = bf16(act_l(h_l . W_l^T + b_l)) for l < L - 1; y = act_{L-1}(h_{L-1} .
// W_{L-1}^T + b_{L-1}) as bf16 or fp32 (out_f32), rows < rows, every one of the last layer's N
// columns and nothing beyond them. Every sum runs in gemv_kernel's order, so y holds the bits
// of L gemv_bf16 launches. With a softmax last layer (N == 64, 1 <= n_cls <= 64, out_f32):
// y[m][c] = the probability of class c over the first n_cls logits in softmax_rows' order, for
// c < n_cls, and nothing beyond.
struct StageGemvParams {
  const uint16_t* x;  // [rows][K0] bf16, 16-byte aligned rows
  long ldx;           // % 8 == 0
  int rows, K0;       // 1..GEMV_MAX_ROWS rows; K0 % 8 == 0, any size
  int L;              // 2 .. STAGE_GEMV_MAX_LAYERS
  StageGemvLayer layer[STAGE_GEMV_MAX_LAYERS];
  void* y;
  long ldy;
  int out_f32;
  int n_cls;  // softmax last layer only
  // [8][layer[0].N] bf16, 16-byte aligned: the first layer's output on its way to the last
  // workgroup. Owned by one launch at a time (launches on one stream are).
  uint16_t* work;
  // one 32-bit word, 0 before the first launch; every launch leaves it 0 again
  uint32_t* counter;
};

// 0, or -1 (sizes: rows, K0, L, a width, n_cls), -2 (leading dimensions), -3 (null operand,
// workspace or counter), -4 (activation: unknown, a hidden softmax, or a softmax that is not
// fp32), -5 (alignment of x, a weight, the workspace, the counter or y), -9 (launch failed). A
// geometry the kernel does not serve returns its code and launches nothing.
int stage_gemv(const StageGemvParams& p, hipStream_t stream);
const char* stage_gemv_error(int code);

}  // namespace dnn
