// utt_fused_kernel on a bf16 word table and bf16 audio / visual frames
// (mmb_mm2_stream_project_tt, MMB_TABLE_BF16 with MMB_FRAMES_BF16): the eight
// pipelined instantiations and the fallback, in a translation unit of their own.
#include "mmb_fused.h"

namespace mmb {

int launch_fused_tbf16_bf16(const FusedArgs& f, int grid, hipStream_t stream) {
  return launch_fused_frames<bf16_t, bf16_t>(f, grid, stream);
}

}  // namespace mmb
