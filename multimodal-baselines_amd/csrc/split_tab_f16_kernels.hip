// utt_split_part_kernel, utt_split_finish_kernel and mm2_text_table_kernel on
// a fp16 word table (mmb_mm2_stream_split_tt, mmb_mm2_text_cache_tt,
// MMB_TABLE_F16): the split stream's kernels for each of the three frame
// types and the text cache's row kernel, in a translation unit of their own.
#include "mmb_split_kernels.h"
#include "mmb_text_cache.h"

namespace mmb {

int split_route_f16(const StreamArgs& s, const SplitPlan& q, const StreamVec& vec, int frame_type, float* part,
                    hipStream_t stream) {
  return split_route<f16_t>(s, q, vec, frame_type, part, stream);
}

int text_table_rows_f16(const void* table, int64_t v, int d, const float* wm, int ldw, float* rows,
                        hipStream_t stream) {
  return text_table_rows<f16_t>(table, v, d, wm, ldw, rows, stream);
}

}  // namespace mmb
