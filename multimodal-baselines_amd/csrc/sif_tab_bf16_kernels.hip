// utt_wave_kernel and utt_stream_kernel on a bf16 word table
// (mmb_sif_wavg_tt, mmb_mm2_stream_tt, MMB_TABLE_BF16): the SIF gather's
// kernels and the MMB2 stream's for each of the three frame types, in a
// translation unit of their own.
#include "mmb_stream_kernels.h"

namespace mmb {

int sif_route_bf16(const StreamArgs& a, bool v4, bool wave, hipStream_t stream) {
  return sif_route<bf16_t>(a, v4, wave, stream);
}

int stream_route_bf16(StreamArgs& s, int frame_type, uint32_t* colmax, hipStream_t stream) {
  return stream_route_frames<bf16_t>(s, frame_type, colmax, stream);
}

}  // namespace mmb
