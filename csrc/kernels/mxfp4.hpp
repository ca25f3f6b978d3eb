// OCP microscaling FP4 (MXFP4) weight rows: the quantiser and dequantiser (csrc/kernels/mxfp4.hip).
//
// The format (tests/_mxfp4_oracle.py is its exact reference): a row of K bf16 values, K % 32 ==
// 0, becomes K / 2 bytes of e2m1 codes and K / 32 bytes of e8m0 block scales.
//   element  4-bit code s|ee|m: magnitude {0, 0.5, 1, 1.5, 2, 3, 4, 6}[code & 7], sign = bit 3
//   packing  byte j of a row holds column 2j in its low nibble, column 2j + 1 in its high one
//   scale    one byte E per 32 consecutive columns, in a tensor of its own: 2^(E - 127)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dnn {

constexpr int MXFP4_BLOCK = 32;           // columns that share one scale byte
constexpr int MXFP4_TINY_EXP_FIELD = 17;  // bf16 exponent field of 2^-110: blocks whose amax is
                                          // below it are zero blocks (E = 0, every nibble 0x0)

// x bf16 [rows][ldx] -> q uint8 [rows][ldq >= cols / 2], e uint8 [rows][lde >= cols / 32]. Per
// block: amax = max |x|; amax < 2^-110: E = 0, nibbles 0x0; otherwise E = floor(log2 amax) - 2
// + 127 (the bf16 exponent field of amax minus 2, in [15, 252]), t = x * 2^(127 - E) (exact,
// |t| < 8), |t| > 6 saturates to 6, otherwise t rounds to the nearest magnitude, a tie to the
// even code; the sign bit is kept (also on a zero). cols % 32 == 0, ldx % 8 == 0, ldq % 16 ==
// 0, x and q 16-byte aligned. Rows holding NaN or infinity are not specified.
int quant_rows_mxfp4(const uint16_t* x, long ldx, int rows, int cols, unsigned char* q, long ldq,
                     unsigned char* e, long lde, hipStream_t stream);

// The inverse: x = bf16(dec(code) * 2^(E - 127)), exact for every E the quantiser writes; a
// block with E == 0 gives +0 whatever its nibbles hold. Same preconditions.
int dequant_rows_mxfp4(const unsigned char* q, long ldq, const unsigned char* e, long lde,
                       int rows, int cols, uint16_t* x, long ldx, hipStream_t stream);

}  // namespace dnn
