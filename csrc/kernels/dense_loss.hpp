// Host-visible launcher of csrc/kernels/dense_loss.hip: the dense-target losses (mean squared
// error, binary cross-entropy on logits) of a linear / relu / sigmoid output layer. Returns 0 on
// success and a negative code (nothing launched) when a host-side precondition fails.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dnn {

enum DenseLoss : int { DENSE_MSE = 1, DENSE_BCE = 2 };  // ops/kernels.py keeps the same table

// z: fp32 pre-activations [rows][ld_z], t: bf16 targets [rows][ld_t]; only their first n_out
// columns are read. row_ok (nullable = every row valid): a row with row_ok[r] < 0 is padding,
// it gets dz = 0 and no loss. dz: bf16 [rows][ld_dz], columns n_out..width written as 0, where
// width is the padded width (a multiple of 64, no upper limit). With y = act(z), n = n_out:
//   DENSE_MSE (act linear | relu | sigmoid): loss_r = (1/n) sum_c (y - t)^2,
//                                            dz = (2 scale / n) (y - t) act'(z)
//   DENSE_BCE (act sigmoid, from the logits): loss_r = (1/n) sum_c [max(z, 0) - t z +
//                                            log1p(exp(-|z|))], dz = (scale / n) (y - t)
// The grid is dense_loss_row_blocks(rows) x dense_loss_col_chunks(width) blocks of 64 rows x 256
// columns; block (rb, ch) writes loss_part[rb * chunks + ch] (optional) and its columns of
// colsum[rb][.] (optional: column sums of the stored bf16 dz = bias-gradient partials).
int dense_loss(const float* z, long ld_z, const uint16_t* t, long ld_t, const int* row_ok,
               uint16_t* dz, long ld_dz, int rows, int n_out, int width, int loss, int act,
               float scale, float* loss_part, float* colsum, long ld_colsum, hipStream_t stream);
int dense_loss_row_blocks(int rows);
int dense_loss_col_chunks(int width);

}  // namespace dnn
