// The tools build's part of
// multimodal-baselines_amd/csrc/narrow_fused_kernels.hip
// (tools/diag/libmmb_diag.so): the definitions behind its MMB_HOOK_* points
// (declared in tools/diag/diag_hooks.h, force-included by `make diag`).
// Included at the end of that file through MMB_TOOLS_TAIL_NARROW_FUSED; the
// product library includes an empty header there.
// Test and timing infrastructure, not product code.
namespace mmb {

// the narrow fused kernel's two-team variant (MMB_NF_TEAMS): its LDS
// attribute and launch
template <int I>
void diag_nf_teams_attr() {
  allow_dynamic_lds<&utt_narrow_fused_kernel<kNFUnr, kNFHU, kNFGA, kNFGV, true>>(kNFLds);
}
template <class F>
bool diag_nf_teams_launch(int teams, const F& f, int64_t grid, hipStream_t stream) {
  if (!teams) return false;
  utt_narrow_fused_kernel<kNFUnr, kNFHU, kNFGA, kNFGV, true><<<static_cast<unsigned>(grid), kNFThreads, kNFLds, stream>>>(f);
  return true;
}

}  // namespace mmb
