// The text cache's row kernel as a template on the word table's element type
// TE (mmb_mm2_text_cache, mmb_mm2_text_cache_tt).  Three sources instantiate
// it: mm2_kernels.hip for an f32 table, split_tab_f16_kernels.hip and
// split_tab_bf16_kernels.hip for a 16-bit one.  A kernel is in exactly one
// code object: an instantiation's TE names its source.  Included by those
// three only.
#pragma once
#include "mmb_stream.h"

namespace mmb {

// element p of a table of type TE as f32: a 16-bit value widened exactly
// (scalar 2-byte loads: the build is off the hot path)
template <class TE>
__device__ __forceinline__ float text_elem(const TE* p) {
  if constexpr (std::is_same_v<TE, float>) {
    return *p;
  } else {
    return frame_f32<TE>(*reinterpret_cast<const uint16_t*>(p));
  }
}

// Row v of the cache (the layout: mm2_kernels.hip, "text cache"): E half = the
// table row as f32, P half = the f64 fma chain over it rounded once.  For a
// 16-bit TE both halves are, byte for byte, those of the table upcast to f32.
template <class TE>
__global__ __launch_bounds__(320) void mm2_text_table_kernel(const TE* __restrict__ E, int D,
                                                             const float* __restrict__ wm, int ldw,
                                                             float* __restrict__ rows) {
  __shared__ double se[kTextLdp], se2[kTextLdp];
  const int64_t v = blockIdx.x;
  for (int f = threadIdx.x; f < D; f += blockDim.x) {
    const double e = text_elem<TE>(E + v * D + f);
    se[f] = e;
    se2[f] = e * e;
  }
  __syncthreads();
  float* row = rows + v * kTextLdq;
  for (int f = threadIdx.x; f < D; f += blockDim.x) row[f] = text_elem<TE>(E + v * D + f);
  for (int j = threadIdx.x; j + D < kTextLdq; j += blockDim.x) {
    double acc = 0.0;
    if (j <= D) {
      for (int f = 0; f < D; ++f) {
        acc = fma(se[f], static_cast<double>(wm[static_cast<int64_t>(f) * ldw + j]), acc);
        acc = fma(se2[f], static_cast<double>(wm[static_cast<int64_t>(D + f) * ldw + j]), acc);
      }
    }
    row[D + j] = static_cast<float>(acc);
  }
}

template <class TE>
static int text_table_rows(const void* table, int64_t v, int d, const float* wm, int ldw, float* rows,
                           hipStream_t stream) {
  mm2_text_table_kernel<TE><<<static_cast<unsigned>(v), 320, 0, stream>>>(static_cast<const TE*>(table), d, wm,
                                                                          ldw, rows);
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

#pragma GCC visibility push(hidden)
// the rows from a 16-bit table, each instantiated in its own source
// (split_tab_f16_kernels.hip, split_tab_bf16_kernels.hip)
int text_table_rows_f16(const void* table, int64_t v, int d, const float* wm, int ldw, float* rows,
                        hipStream_t stream);
int text_table_rows_bf16(const void* table, int64_t v, int d, const float* wm, int ldw, float* rows,
                         hipStream_t stream);
#pragma GCC visibility pop

}  // namespace mmb
