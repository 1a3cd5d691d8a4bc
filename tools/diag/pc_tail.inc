// The tools build's part of multimodal-baselines_amd/csrc/pc_kernels.hip
// (tools/diag/libmmb_diag.so): the definitions behind its MMB_HOOK_* points
// (declared in tools/diag/diag_hooks.h, force-included by `make diag`), the
// variant kernel they launch and the mmb_diag_pc_* entry points.  Included at
// the end of that file through MMB_TOOLS_TAIL_PC; the product library
// includes an empty header there.  Test and timing infrastructure:
//   pc_solve_mc_v1_kernel  the r03-r04 multi-workgroup solve (MMB_PC_SOLVE_V1)
// and the knob MMB_PC_ABL.  mmb_diag_pc_wait_iters / mmb_diag_pc_skip_arrival
// are here because g_pm_wait_iters / g_pm_skip_wg (diag_hooks.h) are static
// __device__: one copy per translation unit, and pc_solve_mc_kernel reads
// this unit's.
namespace mmb {

// the r04 kernel's wave split
constexpr int kPmPw = 15;  // waves holding G (wave 15 runs the Cholesky meanwhile)
constexpr int kPmKs = 6;   // k-steps of G per wave: ceil(kP16MaxD / 4 / kPmPw)

// The r03-r04 round (tools build, MMB_PC_SOLVE_V1=1 for A/B runs): the
// Cholesky of W_r on wave 15 beside the partials of G_t B_r, then the
// exchange of Y_t = G_t B_r M_r^T and P_t = Y_t^T Y_t -- the factor (~5.5 us
// of a ~11 us round) and the exchange (~4.5 us) in sequence.
__global__ __launch_bounds__(kP16NT) void pc_solve_mc_v1_kernel(const double* __restrict__ G, int D,
                                                                  const double* __restrict__ z0, int k,
                                                                  int npc, int n_iter, int transposed,
                                                                  double* __restrict__ pc_out,
                                                                  double* xbuf, unsigned* ctl,
                                                                  int32_t* flag) {
  extern __shared__ __attribute__((aligned(16))) double p16_lds[];
  const int Dp = (D + 15) / 16 * 16;
  const int T = Dp / 16;
  double* sZ = p16_lds;               // the orthonormal block (explicit rounds)
  double* sY = sZ + Dp * kP16W;       // the raw block B_r (z0, then G Z_{r-1})
  double* part = sY + Dp * kP16W;     // max(16 x 256, Dp x 16)
  P16_SMALL_DECL
  __shared__ double sHt[256], sYt[256], sPt[256], sM[256], sM2[256], sd[kMaxK];
  __shared__ int s_abort;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int t = blockIdx.x;
  unsigned* ctr = ctl;
  unsigned* abort_w = ctl + 1;

  // this workgroup's 16 rows of G as MFMA A fragments on waves 0-14 (G
  // symmetric: row p of the tile = column p, 16 consecutive doubles per k-row:
  // coalesced); wave 15 is free for the k x k work that overlaps the product
  double ga[kPmKs];
  {
    const int p = t * 16 + (lane & 15);
#pragma unroll
    for (int j = 0; j < kPmKs; ++j) {
      const int q = 4 * (wave + kPmPw * j) + (lane >> 4);
      ga[j] = (wave < kPmPw && p < D && q < D) ? G[static_cast<int64_t>(q) * D + p] : 0.0;
    }
  }
  // waves 0-14: their partial products of this tile of G with a [Dp][16] block
  auto tile_partials = [&](const double* B) {
    if (wave < kPmPw) {
      f64x4 acc = {0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < kPmKs; ++j) {
        const int q = 4 * (wave + kPmPw * j) + (lane >> 4);
        if (4 * (wave + kPmPw * j) < Dp)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ga[j], B[q * kP16W + (lane & 15)], acc, 0, 0, 0);
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) part[wave * 256 + ((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = acc[reg];
    }
  };
  // ... summed over the waves in a fixed order (after a barrier)
  auto tile_sum = [&](double* out) {
    if (tid < 256) {
      double s = 0.0;
#pragma unroll
      for (int w = 0; w < kPmPw; ++w) s += part[w * 256 + tid];
      out[tid] = s;
    }
    __syncthreads();
  };
  auto tile_product = [&](const double* B, double* out) {
    tile_partials(B);
    __syncthreads();
    tile_sum(out);
  };
  // MGS^2 of the k columns of a [Dp][16] block on wave 0 (extreme
  // ill-conditioning: a Cholesky pivot <= 0), in place
  auto mgs = [&](double* B) {
    if (wave == 0) {
      for (int e = lane; e < D * k; e += kWave) part[e] = B[(e / k) * kP16W + e % k];
      wave_lds_sync();
      orth_wave(part, D, k, lane);
      for (int e = lane; e < D * k; e += kWave) B[(e / k) * kP16W + e % k] = part[e];
    }
    __syncthreads();
  };

  for (int e = tid; e < Dp * kP16W; e += kP16NT) {
    const int p = e / kP16W, j = e % kP16W;
    sY[e] = (p < D && j < k) ? z0[p * k + j] : 0.0;
    sZ[e] = 0.0;
  }
  if (tid == 0) s_abort = 0;
  __syncthreads();
  PC_MARK(0);
  p16_gram(sY, sY, Dp, k, part, sW);  // W_0 = B_0^T B_0 (every workgroup: identical)
  PC_MARK(1);

  // Round r: the raw block B_r (sY) and its Gram W_r (sW) -> Z_r = orth(B_r)
  // -> this tile of G Z_r -> exchange -> B_{r+1}, W_{r+1}.  Rounds r <
  // n_iter orthonormalise implicitly: Z_r = B_r M^T, so G_t Z_r = (G_t B_r)
  // M^T and no row of Z_r is formed.  Round n_iter (the block entering the
  // Rayleigh-Ritz tail) forms Z explicitly with CholeskyQR2.
  for (int r = 0; r <= n_iter; ++r) {
    const bool last = r == n_iter;
    // the equilibrated Cholesky of W on wave 15 while waves 0-14 form this
    // tile's partial products with the raw block B (G_t B: all the implicit
    // path needs before M)
    if (wave == kPmPw) {
      p16_eq_chol(sW, sL, sLi, sM, sd, k, lane, &s_fail);
    } else {
      tile_partials(sY);
    }
    __syncthreads();
    PC_MARK(44 + 2 * r);
    // explicit rows: a failed pivot (MGS^2), or the block entering the
    // transposed branch's tail (an orthonormal Q: CholeskyQR2).  The direct
    // branch's tail is a generalised eigenproblem on span(Z), invariant to
    // the basis, so its last block stays implicit; workgroup 0 forms its
    // rows for the tail.
    const bool explicit_z = (last && transposed) || s_fail;
    if (last && !explicit_z && t == 0) p16_rmul(sY, sM, sZ, Dp);  // Z = B M^T
    if (explicit_z) {
      if (s_fail) {  // the equilibrated rows, orthonormalised by MGS^2
        for (int e = tid; e < D * kP16W; e += kP16NT) sZ[e] = sY[e] * (e % kP16W < k ? sd[e % kP16W] : 0.0);
        __syncthreads();
        mgs(sZ);
      } else {
        p16_rmul(sY, sM, sZ, Dp);  // Z1 = B M1^T
        __syncthreads();
        p16_gram(sZ, sZ, Dp, k, part, sW);  // second CholeskyQR pass on the rows
        if (wave == 0) {
          if (lane == 0) s_fail = 0;
          wave_lds_sync();
          p16_chol(sW, sL, sLi, k, lane, &s_fail);
          for (int e = lane; e < 256; e += kWave) {
            const int j = e / kP16W, m = e % kP16W;
            sM2[e] = (j < k && m <= j) ? sLi[j * k + m] : 0.0;
          }
        }
        __syncthreads();
        if (s_fail) {
          mgs(sZ);
        } else {
          p16_rmul(sZ, sM2, sY, Dp);  // Z = Z1 L2^-T (sY free: B is no longer needed)
          __syncthreads();
          for (int e = tid; e < Dp * kP16W; e += kP16NT) sZ[e] = sY[e];
          __syncthreads();
        }
      }
      tile_product(sZ, sYt);  // Y_t = G_t Z
    } else {
      tile_sum(sHt);    // H_t = G_t B_r (its partials formed beside the Cholesky)
      if (wave == 0) {  // Y_t = H_t M^T
        f64x4 acc = {0, 0, 0, 0};
#pragma unroll
        for (int st = 0; st < 4; ++st) {
          const int m = 4 * st + (lane >> 4);
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sHt[(lane & 15) * 16 + m], sM[(lane & 15) * 16 + m],
                                                     acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) sYt[((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = acc[reg];
      }
    }
    PC_MARK(45 + 2 * r);
    // wave 0: P_t = Y_t^T Y_t, then publishes Y_t | P_t with write-through
    // 8-byte stores, drains them and adds one arrival
    double* xb = xbuf + static_cast<int64_t>(r & 1) * T * 512;
    if (wave == 0) {
      wave_lds_sync();
      f64x4 pa = {0, 0, 0, 0};
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const double y = sYt[(4 * st + (lane >> 4)) * 16 + (lane & 15)];
        pa = __builtin_amdgcn_mfma_f64_16x16x4f64(y, y, pa, 0, 0, 0);
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) sPt[((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = pa[reg];
      wave_lds_sync();
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = lane + kWave * u;
        const double v = e < 256 ? sYt[e] : sPt[e - 256];
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(xb + t * 512 + e),
                           __builtin_bit_cast(unsigned long long, v), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) {
        // release: the tile stores above are visible at agent scope before
        // the arrival that announces them
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        if (!pm_arrive(ctr, T, r, abort_w, flag)) {
          s_abort = 1;
        } else if (!(last && t != 0)) {
          if (!pm_wait(ctr, static_cast<unsigned>(T * (r + 1)), abort_w, flag)) {
            s_abort = 1;
          } else if (last) {
            // every workgroup has made its last arrival: the counter is free
            // again, so the next launch (eager or a graph replay) finds it at
            // 0 with no memset node in front of it
            __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          // acquire: the gather below reads the other workgroups' tiles only
          // after their arrivals were observed (the __syncthreads that follows
          // releases the other waves of this workgroup)
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
      }
    }
    if (last && t != 0) return;  // the tail runs on workgroup 0 only
    PC_MARK(2 + 3 * r);
    __syncthreads();
    if (s_abort) {
      // no caller may go on with a stale PC: an aborted solve leaves NaN in
      // pc_out (every aborting workgroup writes the same NaNs; workgroup 0
      // cannot complete the tail once any workgroup has left)
      for (int e = tid; e < npc * D; e += kP16NT) pc_out[e] = __builtin_nan("");
      return;
    }
    PC_MARK(3 + 3 * r);
    // gather every tile into sY and the partial Grams: all of a thread's
    // loads (sc1, 8 B: the table's first row) issued before any is used
    // (a load-then-store loop waited ~1.5 us per load), then W = sum_t P_t
    // as four strided partial sums combined in a fixed order
    {
      const int e = tid & 255, g = tid >> 8;  // element, tile group (tiles g, g + 4, ..)
      double yv[kPmMaxT / 4], pv[kPmMaxT / 4];
#pragma unroll
      for (int u = 0; u < kPmMaxT / 4; ++u) {
        const int tt = g + 4 * u;
        unsigned long long* src = reinterpret_cast<unsigned long long*>(xb + tt * 512 + e);
        yv[u] = tt < T ? __builtin_bit_cast(double, __hip_atomic_load(src, __ATOMIC_RELAXED,
                                                                      __HIP_MEMORY_SCOPE_AGENT))
                       : 0.0;
        pv[u] = tt < T ? __builtin_bit_cast(double, __hip_atomic_load(src + 256, __ATOMIC_RELAXED,
                                                                      __HIP_MEMORY_SCOPE_AGENT))
                       : 0.0;
      }
      double ps = 0.0;
#pragma unroll
      for (int u = 0; u < kPmMaxT / 4; ++u) {
        const int tt = g + 4 * u;
        if (tt < T) {
          sY[(tt * 16 + (e >> 4)) * kP16W + (e & 15)] = yv[u];
          ps += pv[u];
        }
      }
      part[g * 256 + e] = ps;
    }
    __syncthreads();
    if (tid < 256) {
      const double s = (part[tid] + part[256 + tid]) + (part[512 + tid] + part[768 + tid]);
      const int i = tid >> 4, j = tid & 15;
      if (i < k && j < k) sW[i * k + j] = s;  // W_{r+1}; after the last round H = Y^T Y
    }
    __syncthreads();
    PC_MARK(4 + 3 * r);
  }
  // workgroup 0: sZ = the final block, sY = G Z, sW = (G Z)^T (G Z)
  for (int e = tid; e < k * k; e += kP16NT) sT[e] = sW[e];
  __syncthreads();
  PC_MARK(40);
  p16_tail(sZ, sY, D, Dp, k, npc, transposed, part, sm, pc_out, sT);
  PC_PROBE_FLUSH();
}

// launch_solve_mc with MMB_PC_SOLVE_V1 (the r03-r04 kernel) or MMB_PC_ABL
// (timing-only ablations of the product kernel) set
bool diag_solve_launch(int& rc, const double* g, double* g2, int nsq_wg, int d, const double* z0, int k,
                       int npc, int n_iter, int transposed, double* pc_out, double* xbuf, unsigned* ctl,
                       int32_t* flag, int T, hipStream_t stream) {
  rc = MMB_OK;
  const size_t lds_max = p16_lds_bytes(kP16MaxD);  // allowed once, for the widest d
  if (diag_knob("MMB_PC_SOLVE_V1", 0) != 0) {
    allow_dynamic_lds<&pc_solve_mc_v1_kernel>(lds_max);
    pc_solve_mc_v1_kernel<<<T, kP16NT, p16_lds_bytes(d), stream>>>(g, d, z0, k, npc, n_iter, transposed,
                                                                   pc_out, xbuf, ctl, flag);
    MMB_LAUNCH_CHECK();
    return MMB_OK;
  }
  if (const int abl = diag_knob("MMB_PC_ABL", 0); abl != 0) {
    auto kern = pc_solve_mc_kernel<3>;
    if (abl == 1) {
      allow_dynamic_lds<&pc_solve_mc_kernel<1>>(lds_max);
      kern = pc_solve_mc_kernel<1>;
    } else if (abl == 2) {
      allow_dynamic_lds<&pc_solve_mc_kernel<2>>(lds_max);
      kern = pc_solve_mc_kernel<2>;
    } else {
      allow_dynamic_lds<&pc_solve_mc_kernel<3>>(lds_max);
    }
    kern<<<T + nsq_wg, kPnNT, p16_lds_bytes(d), stream>>>(g, g2, nsq_wg, d, z0, k, npc, n_iter, transposed,
                                                         pc_out, xbuf, ctl, flag);
    MMB_LAUNCH_CHECK();
    return MMB_OK;
  }
  return false;
}

}  // namespace mmb

// tools build: the multi-workgroup solve's bounded-wait budget (1 << 20 in
// the product)
extern "C" int mmb_diag_pc_wait_iters(int iters) {
  MMB_REQUIRE(iters >= 1);
  const hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_pm_wait_iters), &iters, sizeof(int));
  return e == hipSuccess ? MMB_OK : static_cast<int>(e);
}

// tools build: workgroup wg of the multi-workgroup solve skips its arrivals
// (-1: none, the product behaviour); every wait of the launch then times out
extern "C" int mmb_diag_pc_skip_arrival(int wg) {
  MMB_REQUIRE(wg >= -1);
  const hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_pm_skip_wg), &wg, sizeof(int));
  return e == hipSuccess ? MMB_OK : static_cast<int>(e);
}
