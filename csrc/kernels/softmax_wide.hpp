// Host-visible launchers of csrc/kernels/softmax_wide.hip: the softmax kernels for rows wider
// than the 256 columns the register-resident kernels of elementwise.hip hold. Same contracts and
// return codes as dnn::softmax_xent / dnn::softmax_rows, which dispatch here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dnn {

int softmax_xent_wide(const float* logits, long ld_logits, const int* labels, uint16_t* dz,
                      long ld_dz, int rows, int n_cls, int width, float scale, float* loss_part,
                      int* correct, float* colsum, long ld_colsum, hipStream_t stream);
int softmax_rows_wide(const float* logits, long ld_in, float* out, long ld_out, int rows,
                      int n_cls, const int* labels, int* pred, int* correct, hipStream_t stream);

}  // namespace dnn
