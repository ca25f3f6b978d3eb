from . import gemm_plan
from .gemm_plan import (GEMV_MAX_ROWS, GemmPlan, dgrad_tiles, frag_mask_tiles, pick_splits,
                        pick_tiles, plan, wgrad_config, xent_tiles)
from .kernels import (FP8_DIRECT_MAX_ROWS, FP8_MAX, FP8_TINY_AMAX, MXFP4_BLOCK, KMAJ, MNMAJ, STREAMK_WG, adam_update, blas_gemm,
                      relu_mask_bits, FragMask,
                      colsum_partial, dact_colsum, dense_loss, dense_loss_col_chunks,
                      dense_loss_row_blocks, check_dense_loss, dequant_rows_fp8, quant_rows_fp8,
                      dequant_rows_mxfp4, quant_rows_mxfp4, gemv_mxfp4,
                      gemm, gemv, gemv_fp8, linear_dgrad, linear_fwd, linear_fwd_fp8, linear_fwd_w8a8, linear_fwd_xent, linear_w8a8,
                      linear_fwd_w4a8, linear_w4a8, W4A8_TILES,
                      linear_wgrad, linear_wgrad_group, linear_wgrad_streamk, mlp_tail, pack_bf16,
                      reduce_multi, reduce_slabs, sgd_update, softmax_rows, softmax_xent,
                      step_advance, streamk_partial_elems, streamk_tiles, tail_blocks,
                      tail_supported, transpose_bf16, transpose_multi, unpack_bf16, bias_act_cast,
                      xent_blocks)

__all__ = ["FP8_DIRECT_MAX_ROWS", "FP8_MAX", "FP8_TINY_AMAX", "MXFP4_BLOCK", "GEMV_MAX_ROWS", "KMAJ", "MNMAJ", "STREAMK_WG", "adam_update", "blas_gemm",
           "relu_mask_bits", "FragMask", "frag_mask_tiles", "GemmPlan", "gemm_plan", "plan",
           "colsum_partial", "dact_colsum", "dense_loss", "dense_loss_col_chunks",
           "dense_loss_row_blocks", "check_dense_loss", "dequant_rows_fp8", "quant_rows_fp8",
           "dequant_rows_mxfp4", "quant_rows_mxfp4", "gemv_mxfp4",
           "dgrad_tiles", "gemm", "gemv", "gemv_fp8", "linear_dgrad", "linear_fwd", "linear_fwd_fp8", "linear_fwd_w8a8", "linear_fwd_xent", "linear_w8a8",
           "linear_fwd_w4a8", "linear_w4a8", "W4A8_TILES",
           "linear_wgrad", "linear_wgrad_group", "linear_wgrad_streamk", "mlp_tail", "pack_bf16", "pick_splits", "pick_tiles",
           "reduce_multi", "reduce_slabs", "sgd_update", "softmax_rows", "softmax_xent",
           "step_advance", "streamk_partial_elems", "streamk_tiles", "tail_blocks", "tail_supported",
           "transpose_bf16", "transpose_multi", "unpack_bf16", "bias_act_cast", "wgrad_config", "xent_blocks", "xent_tiles"]
