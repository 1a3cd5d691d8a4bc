// The MMB2 stream and its projection in one kernel (mmb_fused.h): the f32
// instantiations of utt_fused_kernel and the entry points
// mmb_mm2_stream_project, mmb_mm2_stream_project_ft and
// mmb_mm2_stream_project_tt.  The 16-bit instantiations are in
// fused_f16_kernels.hip and fused_bf16_kernels.hip (frames) and in the six
// fused_t<table>_<frames>_kernels.hip (a 16-bit word table).
#include "mmb_fused.h"

namespace mmb {

static int launch_fused(const FusedArgs& f, int grid, hipStream_t stream) {
#ifndef MMB_HOOK_FUSED_LAUNCH  // (tools/diag: the MMB_FUSED_* sweeps and ablations)
#define MMB_HOOK_FUSED_LAUNCH false
#endif
  if (!(MMB_HOOK_FUSED_LAUNCH)) return launch_fused_frames<float>(f, grid, stream);
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

// the launch for a word table of storage type table_type and frames of
// storage type frame_type: each pair's kernels live in a source of their own
static int launch_fused_pair(int table_type, int frame_type, const FusedArgs& f, int grid, hipStream_t stream) {
  using Launch = int (*)(const FusedArgs&, int, hipStream_t);
  static constexpr Launch kLaunch[3][3] = {
      {launch_fused, launch_fused_f16, launch_fused_bf16},
      {launch_fused_tf16_f32, launch_fused_tf16_f16, launch_fused_tf16_bf16},
      {launch_fused_tbf16_f32, launch_fused_tbf16_f16, launch_fused_tbf16_bf16}};
  return kLaunch[table_type][frame_type](f, grid, stream);
}

// mmb_mm2_stream_project for a word table of storage type table_type
// (MMB_TABLE_*) and frames of storage type frame_type (MMB_FRAMES_*), both
// validated by the caller: the checks, the launch geometry and the column
// bounds are the same for the nine pairs.
static int fused_project(int table_type, int frame_type, const int32_t* ids, const void* table, int64_t v,
                         const float* wtab32, const float* text_dense, const float* w_dense,
                         const void* audio, const void* visual, int64_t n, int t, int d, int a_, int vd,
                         const void* wpieces, const float* c0, float* num_out, float* aux_out,
                         float* mmb2_out, int32_t* flag, uint32_t* colmax, void* colmax_ws,
                         hipStream_t stream) {
  FusedArgs f{};
  // the weighted sum's rows are the text frames themselves; the sums stay on
  // chip (no s_out), fp16 hi | lo
  if (const int rc = stream_args(&f.s, ids, static_cast<const float*>(table), v, wtab32, text_dense, text_dense, w_dense, audio, visual, n, t,
                                 d, a_, vd, num_out, nullptr, 1, aux_out, flag, colmax, colmax_ws))
    return rc;
  MMB_REQUIRE(mmb_mm2_stream_project_supported(t, d, a_, vd) && mmb2_out && wpieces && c0);
  // vector rows are required here, not an option: no scalar fused kernel
  // (stream_vec's width % 4 asks nothing new: the predicate above has it);
  // a unit of 4 values is one load: 16 bytes of f32, 8 of a 16-bit type
  const StreamVec vec = stream_vec(f.s, frame_bytes(frame_type), table_bytes(table_type));
  MMB_REQUIRE(vec.t && vec.a && vec.v && aligned16(num_out) && aligned16(wpieces));
  if (n == 0) return empty_call(colmax, d, stream);
  f.kq[0] = piece_k(d);
  f.kq[1] = piece_k(a_);
  f.kq[2] = piece_k(vd);
  f.img = static_cast<const _Float16*>(wpieces);
  f.col_inv = reinterpret_cast<const float*>(f.img + 2 * static_cast<size_t>(kFLdw) * (f.kq[0] + f.kq[1] + f.kq[2]));
  f.c0 = c0;
  f.out = mmb2_out;
  f.nb = ceil_div(n, kGR);
  const int grid = fused_grid(f.nb, stream);
  f.balanced = 1;  // balanced tail: 22.35 -> 22.26 ms (r02s)
  // the dynamic batch schedule's counter, past the column-bound partials
  // (zeroed here by a kernel: no memset node in a captured step)
  f.sched = colmax ? reinterpret_cast<unsigned*>(static_cast<char*>(colmax_ws) +
                                                 static_cast<size_t>(kCmaxRows) * d * sizeof(float))
                   : nullptr;
#ifdef MMB_HOOK_FUSED_ARGS  // (tools/diag: MMB_FUSED_BALANCED / MMB_FUSED_DYN)
  MMB_HOOK_FUSED_ARGS(f);
#endif
  // the dynamic order from 16 rounds of batches on (fewer: the static round
  // robin, whose finishing times spread little there); its units: 48-row
  // batches, then the last ~G batches' rows as 12-row units.  Same-process
  // A/B (tools/fused_dyn_ab.py, r05af/ag, fused kernel ms static ->
  // dynamic): 1M 22.63 -> 22.38, 500k 11.41 -> 11.28, 250k 5.98 -> 5.96;
  // 125k (10 rounds) 2.98 -> 3.06, so it stays static
  const int64_t G = grid;
  if (f.nb < 16 * G) f.sched = nullptr;
  if (f.sched) {
    f.big = std::max<int64_t>(0, n - kGR * G) / kGR;
    f.nu = f.big + ceil_div(n - f.big * kGR, kGR / 4);
    if (const int rc = zero_words_async(f.sched, 1, stream)) return rc;
  }
  const int rc = launch_fused_pair(table_type, frame_type, f, grid, stream);
  // the bounds: a partial row per streamer wave
  return reduce_colmax(rc, f.s, grid * 4, colmax, stream);
}

}  // namespace mmb

using namespace mmb;

extern "C" int mmb_mm2_stream_project_supported(int t, int d, int a_, int vd) {
  // every piece [Sx | Sxx] of one modality fits a ring slot (2 w <= 640),
  // two float4 columns per lane (w <= 512), the 320-column weight image
  return t > 0 && t <= kWave && d >= 256 && d < 320 && d % 4 == 0 && a_ > 0 && vd > 0 &&
         a_ % 4 == 0 && vd % 4 == 0 && 2 * a_ <= kGPlane && 2 * vd <= kGPlane;
}

extern "C" int mmb_mm2_stream_project(const int32_t* ids, const float* table, int64_t v,
                                      const float* wtab32, const float* text_dense,
                                      const float* w_dense, const float* audio, const float* visual,
                                      int64_t n, int t, int d, int a_, int vd, const void* wpieces,
                                      const float* c0, float* num_out, float* aux_out,
                                      float* mmb2_out, int32_t* flag, uint32_t* colmax,
                                      void* colmax_ws, hipStream_t stream) {
  return fused_project(MMB_TABLE_F32, MMB_FRAMES_F32, ids, table, v, wtab32, text_dense, w_dense, audio, visual, n, t, d, a_, vd,
                       wpieces, c0, num_out, aux_out, mmb2_out, flag, colmax, colmax_ws, stream);
}

extern "C" int mmb_mm2_stream_project_ft(const int32_t* ids, const float* table, int64_t v,
                                         const float* wtab32, const float* w_dense, const void* audio,
                                         const void* visual, int frame_type, int64_t n, int t, int d,
                                         int a_, int vd, const void* wpieces, const float* c0,
                                         float* num_out, float* aux_out, float* mmb2_out, int32_t* flag,
                                         uint32_t* colmax, void* colmax_ws, hipStream_t stream) {
  MMB_REQUIRE(frame_bytes(frame_type) != 0);
  MMB_REQUIRE(ids);  // gathered text only
  return fused_project(MMB_TABLE_F32, frame_type, ids, table, v, wtab32, nullptr, w_dense, audio, visual, n, t, d, a_,
                       vd, wpieces, c0, num_out, aux_out, mmb2_out, flag, colmax, colmax_ws, stream);
}

extern "C" int mmb_mm2_stream_project_tt(const int32_t* ids, const void* table, int table_type, int64_t v,
                                         const float* wtab32, const float* w_dense, const void* audio,
                                         const void* visual, int frame_type, int64_t n, int t, int d,
                                         int a_, int vd, const void* wpieces, const float* c0,
                                         float* num_out, float* aux_out, float* mmb2_out, int32_t* flag,
                                         uint32_t* colmax, void* colmax_ws, hipStream_t stream) {
  MMB_REQUIRE(table_bytes(table_type) != 0 && frame_bytes(frame_type) != 0);
  MMB_REQUIRE(ids);  // gathered text only
  return fused_project(table_type, frame_type, ids, table, v, wtab32, nullptr, w_dense, audio, visual, n, t, d, a_,
                       vd, wpieces, c0, num_out, aux_out, mmb2_out, flag, colmax, colmax_ws, stream);
}

// the tools build's variant launches, knobs and probes (tools/diag/); the
// product library includes an empty header here
#ifndef MMB_TOOLS_TAIL_FUSED
#define MMB_TOOLS_TAIL_FUSED "mmb_no_tools.h"
#endif
#include MMB_TOOLS_TAIL_FUSED
