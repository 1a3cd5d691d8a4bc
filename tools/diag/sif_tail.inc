// The tools build's part of multimodal-baselines_amd/csrc/sif_kernels.hip
// (tools/diag/libmmb_diag.so): the definitions behind its MMB_HOOK_* points
// (declared in tools/diag/diag_hooks.h, force-included by `make diag`) and
// the mmb_diag_* entry points.  Included at the end of that file through
// MMB_TOOLS_TAIL_SIF; the product library includes an empty header there.
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

// launch_fused with the MMB_FUSED_* knobs (read per launch: in-process sweeps):
// MMB_FUSED_UNR streamer frames per load group, MMB_FUSED_DIAG timing-only
// ablations, MMB_FUSED_PIPE streamer pipelining, MMB_FUSED_SLOTS ring slots
template <class F>
bool diag_fused_launch(const F& f, int grid, hipStream_t stream) {
  auto fused_diag = [] { return diag_knob("MMB_FUSED_DIAG", 0); };
  auto fused_pipe = [] { return diag_knob("MMB_FUSED_PIPE", 2); };
  auto fused_slots = [] { return diag_knob("MMB_FUSED_SLOTS", kGSlots); };
  const int dg = fused_diag();
  // the product's streamer (PIPE 2, two groups of kFUnr frames in flight)
  // and its ablations; everything else defaults to 8-frame groups
  const bool prod = fused_pipe() == 2 && (dg == 0 || dg == 1 || dg == 4 || dg == 128 || dg == 256);
  const int un = diag_knob("MMB_FUSED_UNR", prod ? kFUnr : 8);
  const bool pipe = fused_pipe() != 0 && fused_pipe_ok(f, un);
  if (pipe && prod && un == kFUnr) {
    if (dg == 1) {
      launch_fused_v<1, kFUnr, 2>(f, grid, stream);
    } else if (dg == 4) {
      launch_fused_v<4, kFUnr, 2>(f, grid, stream);
    } else if (dg == 128) {
      launch_fused_v<128, kFUnr, 2>(f, grid, stream);
    } else if (dg == 256) {
      launch_fused_v<256, kFUnr, 2>(f, grid, stream);
    } else {
      launch_fused_tm<kFUnr, 2>(f, grid, stream);
    }
  } else if (pipe && prod && dg == 0 && (un == 8 || un == 10 || un == 12)) {
    // the pipeline-depth candidates: two groups of MMB_FUSED_UNR frames in
    // flight (16, 20 or 24 frames); every piece with its tail load, which
    // is right at any width
    if (un == 8) {
      launch_fused_v<0, 8, 2>(f, grid, stream);
    } else if (un == 10) {
      launch_fused_v<0, 10, 2>(f, grid, stream);
    } else {
      launch_fused_v<0, 12, 2>(f, grid, stream);
    }
  } else if (pipe && un == 8) {
    switch (dg) {
      case 1: launch_fused_v<1, 8, true>(f, grid, stream); break;
      case 2: launch_fused_v<2, 8, true>(f, grid, stream); break;
      case 4: launch_fused_v<4, 8, true>(f, grid, stream); break;
      case 16: launch_fused_v<16, 8, true>(f, grid, stream); break;
      case 32: launch_fused_v<32, 8, true>(f, grid, stream); break;
      case 64: launch_fused_v<64, 8, true>(f, grid, stream); break;
      default:
        if (fused_slots() == 60) {
          launch_fused_v<0, 8, true, 60>(f, grid, stream);
        } else {
          launch_fused_v<0, 8, true>(f, grid, stream);
        }
        break;
    }
  } else if (pipe && dg == 0 && un == 6) {
    launch_fused_v<0, 6, true>(f, grid, stream);

  } else if (dg == 0 && un == 12) {
    launch_fused_v<0, 12>(f, grid, stream);
  } else if (dg == 0 && un == 16) {
    launch_fused_v<0, 16>(f, grid, stream);
  } else if (dg == 1 && un == 16) {
    launch_fused_v<1, 16>(f, grid, stream);
  } else switch (dg) {
    case 1: launch_fused_v<1>(f, grid, stream); break;
    case 2: launch_fused_v<2>(f, grid, stream); break;
    case 4: launch_fused_v<4>(f, grid, stream); break;
    case 8: launch_fused_v<8>(f, grid, stream); break;
    default: launch_fused_v<0>(f, grid, stream); break;
  }
  return true;
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

// tools build: the bounded waits' iteration budget (1 << 23 in the product)
extern "C" int mmb_diag_fused_wait_iters(int iters) {
  MMB_REQUIRE(iters >= 1);
  const hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_fused_wait_iters), &iters, sizeof(int));
  return e == hipSuccess ? MMB_OK : static_cast<int>(e);
}

// tools build: copy the fused kernel's per-workgroup wall-clock marks
// [1024][9] (start, streamer waves 0-3 end, projector waves 4-7 end) and the
// wall-clock rate (kHz) to the host
extern "C" int mmb_diag_fused_probe(unsigned long long* host_out, int* rate_khz) {
  MMB_REQUIRE(host_out && rate_khz);
  hipError_t e = hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_fused_probe), sizeof(g_fused_probe));
  if (e != hipSuccess) return static_cast<int>(e);
  int dev = 0;
  (void)hipGetDevice(&dev);
  e = hipDeviceGetAttribute(rate_khz, hipDeviceAttributeWallClockRate, dev);
  return e == hipSuccess ? MMB_OK : static_cast<int>(e);
}
