// What gram_kernels.hip and pc_kernels.hip share (included by them only): the
// f64 MFMA accumulator type and the loads of one element of the sentence rows
// x = num / count, which the Gram kernels and X^T Omega must read alike.  No
// __global__ function lives here, and nothing only one source uses.
#pragma once
#include "mmb_common.h"

namespace mmb {

using f64x4 = __attribute__((ext_vector_type(4))) double;

__device__ __forceinline__ float load_x(const float* __restrict__ num, const float* __restrict__ cnt,
                                        int64_t row, int col, int D) {
  if (col >= D) return 0.f;
  const float v = num[row * D + col];
  return cnt ? v / cnt[row] : v;  // x = num / count_nonzero(w), f32 (sif_functions.py:55)
}
// float64 rows (the numpy drop-in's general f64 X, sif_functions.py:58-81): no count
__device__ __forceinline__ double load_x(const double* __restrict__ num, const float* __restrict__,
                                         int64_t row, int col, int D) {
  return col < D ? num[row * D + col] : 0.0;
}

}  // namespace mmb
