// The tools build's part of multimodal-baselines_amd/csrc/fused_kernels.hip
// (tools/diag/libmmb_diag.so): the definitions behind its MMB_HOOK_* points
// (declared in tools/diag/diag_hooks.h, force-included by `make diag`) and
// the mmb_diag_fused_* entry points -- here, in utt_fused_kernel's own
// translation unit: g_fused_wait_iters and g_fused_probe are static
// __device__, a copy per unit, and the kernel reads this unit's.  Included at
// the end of that file through MMB_TOOLS_TAIL_FUSED; the product library
// includes an empty header there.
// Test and timing infrastructure, not product code.
namespace mmb {

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
