// The tools build's part of multimodal-baselines_amd/csrc/sif_kernels.hip
// (tools/diag/libmmb_diag.so): the definitions behind its MMB_HOOK_* points
// (declared in tools/diag/diag_hooks.h, force-included by `make diag`).
// Included at the end of that file through MMB_TOOLS_TAIL_SIF; the product
// library includes an empty header there.  (The fused kernels' parts:
// fused_tail.inc, narrow_fused_tail.inc.)
// Test and timing infrastructure, not product code.
namespace mmb {

// launch_narrow with MMB_STREAM_NARROW set (the product runs variant 10)
template <class A>
bool diag_narrow_launch(int var, const A& a, int grid, hipStream_t stream) {
  switch (var) {
    case 2: utt_narrow_kernel<2, 4, 7, 4, 2><<<grid, 256, 0, stream>>>(a); break;
    case 3: utt_narrow_kernel<2, 5, 7, 4, 2><<<grid, 256, 0, stream>>>(a); break;
    case 4: utt_narrow_kernel<2, 10, 7, 4, 2><<<grid, 256, 0, stream>>>(a); break;
    case 5: utt_narrow_kernel<2, 5, 7, 4, 4><<<grid, 256, 0, stream>>>(a); break;
    case 6: utt_narrow_kernel<2, 5, 7, 4, 2, 1><<<grid, 256, 0, stream>>>(a); break;
    case 7: utt_narrow_kernel<2, 5, 7, 4, 2, 2><<<grid, 256, 0, stream>>>(a); break;
    case 8: utt_narrow_kernel<2, 5, 7, 4, 2, 4><<<grid, 256, 0, stream>>>(a); break;
    case 9: utt_narrow_kernel<2, 5, 7, 4, 2, 3><<<grid, 256, 0, stream>>>(a); break;
    case 11: utt_narrow_kernel<2, 5, 7, 4, 2, 0, 0, 1><<<grid, 256, 0, stream>>>(a); break;
    case 12: utt_narrow_kernel<2, 5, 7, 4, 2, 0, 1, 1><<<grid, 256, 0, stream>>>(a); break;
    case 13: utt_narrow_kernel<2, 8, 7, 4, 2, 0, 1, 1><<<grid, 256, 0, stream>>>(a); break;
    default: utt_narrow_kernel<2, 5, 7, 4, 2, 0, 1, 0><<<grid, 256, 0, stream>>>(a); break;
  }
  return true;
}

// launch_wave with MMB_STREAM_POLICY set (the product runs policy 5)
template <bool MM2, int CT, int CA, int CV, class A>
bool diag_wave_launch(const A& a, int grid, hipStream_t stream) {
  switch (MM2 ? diag_knob("MMB_STREAM_POLICY", 5) & 15 : 0) {
    case 13: launch_wave_v<MM2, CT, CA, CV, 4, true, false, 2>(a, grid, stream); break;
    case 1: launch_wave_v<MM2, CT, CA, CV, 2, true, false>(a, grid, stream); break;
    case 2: launch_wave_v<MM2, CT, CA, CV, 2, false, true>(a, grid, stream); break;
    case 3: launch_wave_v<MM2, CT, CA, CV, 2, true, true>(a, grid, stream); break;
    case 4: launch_wave_v<MM2, CT, CA, CV, 4, false, false>(a, grid, stream); break;
    case 5: launch_wave_v<MM2, CT, CA, CV, 4, true, false>(a, grid, stream); break;
    case 6: launch_wave_v<MM2, CT, CA, CV, 4, false, true>(a, grid, stream); break;
    case 7: launch_wave_v<MM2, CT, CA, CV, 4, true, true>(a, grid, stream); break;
    default: launch_wave_v<MM2, CT, CA, CV, 2, false, false>(a, grid, stream); break;
  }
  return true;
}

// launch_wave on 16-bit frames with MMB_FRAMES16_UNR: frames per load group
// (the product runs 4; the sums do not depend on it)
template <int CT, int CA, int CV, class FE, class A>
bool diag_wave16_launch(const A& a, int grid, hipStream_t stream) {
  switch (diag_knob("MMB_FRAMES16_UNR", 4)) {
    case 6: utt_wave_kernel<true, CT, CA, CV, 6, true, false, false, 1, FE><<<grid, 256, 0, stream>>>(a); break;
    case 8: utt_wave_kernel<true, CT, CA, CV, 8, true, false, false, 1, FE><<<grid, 256, 0, stream>>>(a); break;
    default: return false;
  }
  return true;
}

// launch_split on 16-bit frames with MMB_SPLIT16_UNR: frames unrolled per
// thread group of the frame workgroups (the product runs kSplitFU16; the sums
// do not depend on it).  Only the all-vector instantiation has the variant:
// POM's widths, the ones tools/split_ab.py times.
template <int VT, int VA, int VV, class FE, class A, class Q>
bool diag_split16_launch(const A& a, const Q& q, float* part, int64_t grid, hipStream_t stream) {
  if constexpr (VT == 4 && VA == 4 && VV == 4) {
    const unsigned g = static_cast<unsigned>(grid);
    switch (diag_knob("MMB_SPLIT16_UNR", kSplitFU16)) {
      case 8: utt_split_part_kernel<4, 4, 4, 8, kSplitTU, FE><<<g, kNT, 0, stream>>>(a, q, part); return true;
      case 16: utt_split_part_kernel<4, 4, 4, 16, kSplitTU, FE><<<g, kNT, 0, stream>>>(a, q, part); return true;
    }
  }
  return false;
}

// launch_stream's few-long-rows branch with MMB_STREAM_SMALL: 0 as large N,
// 1 the product's 320 x 16 / 8 (returns false), 2 1024 threads x 4 / 4
template <bool MM2, int VT, int VA, int VV, class A>
bool diag_stream_small(const A& a, int grid, hipStream_t stream) {
  const int v = diag_knob("MMB_STREAM_SMALL", 1);
  if (v == 0) {
    utt_stream_kernel<MM2, VT, VA, VV><<<grid, kNT, 0, stream>>>(a);
  } else if (v == 2) {
    utt_stream_kernel<MM2, VT, VA, VV, 4, 4, 1024><<<grid, 1024, 0, stream>>>(a);
  } else {
    return false;
  }
  return true;
}

}  // namespace mmb
