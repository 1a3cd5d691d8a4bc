// The tools build's part of
// multimodal-baselines_amd/csrc/pc_remove_kernels.hip
// (tools/diag/libmmb_diag.so): the launch behind MMB_HOOK_PC_REMOVE_LAUNCH
// (tools/diag/diag_hooks.h), included at the end of that file through
// MMB_TOOLS_TAIL_PC_REMOVE.  Knobs: MMB_PC_REMOVE_R, MMB_PC_REMOVE_NT.
namespace mmb {

// pc_remove's one-row-per-wave launch with MMB_PC_REMOVE_NT (non-temporal
// rows) or MMB_PC_REMOVE_R = 2 / 8 rows per wave
bool diag_pc_remove_launch(int rr, int grid, hipStream_t stream, const float* num, const float* cnt,
                           int64_t n, int d, const double* pc, float* out32) {
  if (diag_knob("MMB_PC_REMOVE_NT", 0) != 0 && rr == 4) {
    pc_remove1_kernel<4, true><<<grid, 256, 0, stream>>>(num, cnt, n, d, pc, out32);
  } else if (rr == 2) {
    pc_remove1_kernel<2><<<grid, 256, 0, stream>>>(num, cnt, n, d, pc, out32);
  } else if (rr == 8) {
    pc_remove1_kernel<8><<<grid, 256, 0, stream>>>(num, cnt, n, d, pc, out32);
  } else {
    return false;
  }
  return true;
}

}  // namespace mmb
