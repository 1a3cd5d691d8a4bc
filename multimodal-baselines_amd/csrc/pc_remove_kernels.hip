// Principal-component removal (a4) for MI355X: the pass
// x - sum_c (x . pc_c) pc_c over the sentence rows, in f64 like the reference
// (sif_functions.py:77-80), with the components from pc_kernels.hip's solve.
// pc_remove_kernel is the general one (any width, npc components, f32 or f64
// rows and output); pc_remove1_kernel the step's (one component, f32 rows of
// 256 < d <= 512, several rows per wave in flight), bit-identical to it.
#include <algorithm>

#include "mmb_common.h"

namespace mmb {

template <int VEC, int PER, typename TX = float>
__global__ __launch_bounds__(256) void pc_remove_kernel(const TX* __restrict__ num,
                                                        const float* __restrict__ cnt, int64_t N,
                                                        int D, const double* __restrict__ pc,
                                                        int npc, float* __restrict__ out32,
                                                        double* __restrict__ out64) {
  extern __shared__ double s_pc[];
  for (int e = threadIdx.x; e < npc * D; e += blockDim.x) s_pc[e] = pc[e];
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int U = D / VEC;
  const int64_t wstride = static_cast<int64_t>(gridDim.x) * (blockDim.x / kWave);
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * (blockDim.x / kWave) + wave; row < N;
       row += wstride) {
    const float sc = cnt ? cnt[row] : 1.f;
    double x[PER][VEC];
#pragma unroll
    for (int m = 0; m < PER; ++m) {
      const int u = lane + kWave * m;
      TX v[VEC];
      if (u < U) {
        if constexpr (VEC == 4) {
          const float4 q = *reinterpret_cast<const float4*>(num + row * D + u * 4);
          v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
          v[0] = num[row * D + u];
        }
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = TX(0);
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) x[m][e] = static_cast<double>(cnt ? v[e] / sc : v[e]);
    }
    double y[PER][VEC];
#pragma unroll
    for (int m = 0; m < PER; ++m)
#pragma unroll
      for (int e = 0; e < VEC; ++e) y[m][e] = 0.0;
    for (int c = 0; c < npc; ++c) {
      const double* pcc = s_pc + c * D;
      double d = 0.0;
#pragma unroll
      for (int m = 0; m < PER; ++m) {
        const int u = lane + kWave * m;
        if (u < U) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) d = fma(x[m][e], pcc[u * VEC + e], d);
        }
      }
      d = wave_sum(d);
#pragma unroll
      for (int m = 0; m < PER; ++m) {
        const int u = lane + kWave * m;
        if (u < U) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) y[m][e] = fma(d, pcc[u * VEC + e], y[m][e]);
        }
      }
    }
#pragma unroll
    for (int m = 0; m < PER; ++m) {
      const int u = lane + kWave * m;
      if (u < U) {
        if (out32) {
          if constexpr (VEC == 4) {
            float4 q;
            q.x = static_cast<float>(x[m][0] - y[m][0]);
            q.y = static_cast<float>(x[m][1] - y[m][1]);
            q.z = static_cast<float>(x[m][2] - y[m][2]);
            q.w = static_cast<float>(x[m][3] - y[m][3]);
            *reinterpret_cast<float4*>(out32 + row * D + u * 4) = q;
          } else {
            out32[row * D + u] = static_cast<float>(x[m][0] - y[m][0]);
          }
        } else {
#pragma unroll
          for (int e = 0; e < VEC; ++e) out64[row * D + u * VEC + e] = x[m][e] - y[m][e];
        }
      }
    }
  }
}

// One PC, f32 rows of 256 < D <= 512 (float4 columns l and l + 64 per lane):
// R rows per wave in flight -- all 2R row loads issued before the first dot,
// the R wave sums interleaved -- where pc_remove_kernel has one row and its
// dependent load -> dot -> sum -> store chain per wave; the PC's lane values
// stay in registers.  Arithmetic (f64 fma order, shuffle-tree wave sum, f32
// rounding) is pc_remove_kernel<4, 2>'s: bit-identical.
// NT (tools build, MMB_PC_REMOVE_NT=1): x read and the rows written
// non-temporally -- an A/B of whether the removal's 2 x N x D x 4 bytes evict
// the word rows the next step's fused kernel would find in L2 / MALL
template <int R, bool NT = false>
__global__ __launch_bounds__(256) void pc_remove1_kernel(const float* __restrict__ num,
                                                         const float* __restrict__ cnt, int64_t N,
                                                         int D, const double* __restrict__ pc,
                                                         float* __restrict__ out32) {
  const int lane = threadIdx.x & (kWave - 1);
  const int U = D / 4;
  const bool h1 = lane + kWave < U;
  double p[2][4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    p[0][e] = lane < U ? pc[4 * lane + e] : 0.0;
    p[1][e] = h1 ? pc[4 * (lane + kWave) + e] : 0.0;
  }
  const int64_t nw = static_cast<int64_t>(gridDim.x) * (blockDim.x / kWave);
  for (int64_t base = (static_cast<int64_t>(blockIdx.x) * (blockDim.x / kWave) + threadIdx.x / kWave) * R;
       base < N; base += nw * R) {
    float4 v[R][2];
    float sc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = min(base + r, N - 1);
      const float* src = num + row * D;
      auto ld = [](const float* q) {
        if constexpr (NT) {
          using f4 = float __attribute__((ext_vector_type(4)));
          const f4 t = __builtin_nontemporal_load(reinterpret_cast<const f4*>(q));
          return make_float4(t.x, t.y, t.z, t.w);
        } else {
          return *reinterpret_cast<const float4*>(q);
        }
      };
      v[r][0] = lane < U ? ld(src + 4 * lane) : make_float4(0.f, 0.f, 0.f, 0.f);
      v[r][1] = h1 ? ld(src + 4 * (lane + kWave)) : make_float4(0.f, 0.f, 0.f, 0.f);
      sc[r] = cnt ? cnt[row] : 1.f;
    }
    double x[R][2][4], d[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const float e4[4] = {v[r][m].x, v[r][m].y, v[r][m].z, v[r][m].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) x[r][m][e] = static_cast<double>(cnt ? e4[e] / sc[r] : e4[e]);
      }
      double acc = 0.0;
      if (lane < U) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fma(x[r][0][e], p[0][e], acc);
      }
      if (h1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fma(x[r][1][e], p[1][e], acc);
      }
      d[r] = acc;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int r = 0; r < R; ++r) d[r] += __shfl_xor(d[r], o, kWave);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (base + r >= N) break;
      float* dst = out32 + (base + r) * D;
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        if (m == 0 ? lane < U : h1) {
          float4 q;
          q.x = static_cast<float>(x[r][m][0] - fma(d[r], p[m][0], 0.0));
          q.y = static_cast<float>(x[r][m][1] - fma(d[r], p[m][1], 0.0));
          q.z = static_cast<float>(x[r][m][2] - fma(d[r], p[m][2], 0.0));
          q.w = static_cast<float>(x[r][m][3] - fma(d[r], p[m][3], 0.0));
          if constexpr (NT) {
            using f4 = float __attribute__((ext_vector_type(4)));
            __builtin_nontemporal_store(f4{q.x, q.y, q.z, q.w}, reinterpret_cast<f4*>(dst + 4 * (lane + kWave * m)));
          } else {
            *reinterpret_cast<float4*>(dst + 4 * (lane + kWave * m)) = q;
          }
        }
      }
    }
  }
}

// pc_remove1_kernel rows per wave (2, 4, 8); 0 = pc_remove_kernel.  Measured
// (tools/remove_ab.py, 1M x 300, r02q): R = 0 / 2 / 4 / 8 = 0.529 / 0.455 /
// 0.435 / 0.444 ms, all bit-identical
#ifndef MMB_HOOK_PC_REMOVE_R  // (tools/diag: MMB_PC_REMOVE_R)
#define MMB_HOOK_PC_REMOVE_R 4
#endif
static int remove_rows() { return MMB_HOOK_PC_REMOVE_R; }

template <int VEC, int PER, typename TX = float>
static int launch_remove(const TX* num, const float* cnt, int64_t n, int d, const double* pc,
                         int npc, float* out32, double* out64, hipStream_t stream) {
  const int64_t waves = ceil_div(n, 1);
  const int grid = static_cast<int>(std::min<int64_t>(ceil_div(waves, 4), 256 * 8));
  pc_remove_kernel<VEC, PER, TX><<<grid, 256, sizeof(double) * npc * d, stream>>>(num, cnt, n, d, pc, npc, out32, out64);
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

}  // namespace mmb

using namespace mmb;

extern "C" int mmb_pc_remove(const float* num, const float* cnt, int64_t n, int d,
                             const double* pc, int npc, float* out32, double* out64,
                             hipStream_t stream) {
  MMB_REQUIRE(num && pc && n >= 0 && d > 0 && npc >= 1 && ((out32 != nullptr) != (out64 != nullptr)));
  MMB_REQUIRE(static_cast<size_t>(npc) * d * sizeof(double) <= 64 * 1024);
  if (n == 0) return MMB_OK;
  const bool v4 = (d % 4 == 0) && aligned16(num) && (out32 == nullptr || aligned16(out32));
  const int U = v4 ? d / 4 : d;
  const int per = static_cast<int>(ceil_div(U, kWave));
  const int rr = remove_rows();
  if (v4 && per == 2 && npc == 1 && out32 && rr > 0) {
    const int64_t waves = ceil_div(n, rr);
    const int grid = static_cast<int>(std::min<int64_t>(ceil_div(waves, 4), 256 * 8));
#ifndef MMB_HOOK_PC_REMOVE_LAUNCH  // (tools/diag: MMB_PC_REMOVE_NT / MMB_PC_REMOVE_R)
#define MMB_HOOK_PC_REMOVE_LAUNCH false
#endif
    if (!(MMB_HOOK_PC_REMOVE_LAUNCH))    {
      pc_remove1_kernel<4><<<grid, 256, 0, stream>>>(num, cnt, n, d, pc, out32);
    }
    MMB_LAUNCH_CHECK();
    return MMB_OK;
  }
  if (v4) {
    if (per <= 1) return launch_remove<4, 1>(num, cnt, n, d, pc, npc, out32, out64, stream);
    if (per <= 2) return launch_remove<4, 2>(num, cnt, n, d, pc, npc, out32, out64, stream);
    if (per <= 4) return launch_remove<4, 4>(num, cnt, n, d, pc, npc, out32, out64, stream);
    if (per <= 8) return launch_remove<4, 8>(num, cnt, n, d, pc, npc, out32, out64, stream);
  } else {
    if (per <= 2) return launch_remove<1, 2>(num, cnt, n, d, pc, npc, out32, out64, stream);
    if (per <= 4) return launch_remove<1, 4>(num, cnt, n, d, pc, npc, out32, out64, stream);
    if (per <= 8) return launch_remove<1, 8>(num, cnt, n, d, pc, npc, out32, out64, stream);
  }
  return MMB_EINVAL;
}

// float64 X (the numpy drop-in's general rows, not f32-representable): the
// f64 removal reading and writing f64 rows
extern "C" int mmb_pc_remove_f64(const double* x, int64_t n, int d, const double* pc, int npc,
                                 double* out64, hipStream_t stream) {
  MMB_REQUIRE(x && pc && out64 && n >= 0 && d > 0 && npc >= 1);
  MMB_REQUIRE(static_cast<size_t>(npc) * d * sizeof(double) <= 64 * 1024);
  if (n == 0) return MMB_OK;
  const int per = static_cast<int>(ceil_div(d, kWave));
  if (per <= 2) return launch_remove<1, 2, double>(x, nullptr, n, d, pc, npc, nullptr, out64, stream);
  if (per <= 4) return launch_remove<1, 4, double>(x, nullptr, n, d, pc, npc, nullptr, out64, stream);
  if (per <= 8) return launch_remove<1, 8, double>(x, nullptr, n, d, pc, npc, nullptr, out64, stream);
  return MMB_EINVAL;
}

// the tools build's variant kernels, launches, knobs and entry points
// (tools/diag/); the product library includes an empty header here
#ifndef MMB_TOOLS_TAIL_PC_REMOVE
#define MMB_TOOLS_TAIL_PC_REMOVE "mmb_no_tools.h"
#endif
#include MMB_TOOLS_TAIL_PC_REMOVE
