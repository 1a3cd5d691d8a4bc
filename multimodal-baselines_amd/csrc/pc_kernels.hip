// The principal-component solve (a3) for MI355X: the randomized SVD replayed
// on the Gram matrix.
//
// The reference computes the PC with scikit-learn's randomized SVD
// (TruncatedSVD(npc, n_iter=7, random_state=0), sif_functions.py:58-67), which
// makes ~15 passes over X.  Here X is read once for its Gram G = X^T X
// (gram_kernels.hip) and the randomized SVD runs on G, [d, d] with d <= 512:
//   * direct branch (n >= d): Z0 = Omega [d,k] (RandomState(0).normal);
//     span(G^n_iter Z0) is the span the reference's LU-normalised iterations
//     build (LU/QR only right-multiply the block); the final SVD of Q^T X with
//     Q = orth(X Z) reduces to the k x k generalised symmetric eigenproblem
//     (Z^T G^2 Z) y = s^2 (Z^T G Z) y, v = G Z y;
//   * transposed branch (n < d, extmath.py:562-566): Z0 = X^T Omega_n, the same
//     iterations, then v = Z u with u the top eigenvector of Z^T G Z;
//   * svd_flip(u_based_decision=False): largest-|.| entry of each component > 0.
// This file holds X^T Omega (xt_omega_*), the one-workgroup solvers
// (pc_solve_kernel; pc_solve16_kernel and its p16_* helpers for d <= 320), the
// multi-workgroup solve (pc_solve_mc_kernel, its pm_* exchange and the squared
// rounds' G^2: square_tile_*, pc_prep_kernel), the step's status word
// (step_status_kernel) and their entry points.  tools/pc_probe/ includes it
// as the solver's source (MMB_PC_PROBE).  The removal is pc_remove_kernels.hip.
#include <algorithm>

#include "mmb_pc.h"

namespace mmb {

template <typename TX>
__global__ void xt_omega_kernel(const TX* __restrict__ num, const float* __restrict__ cnt,
                                int64_t N, int D, const double* __restrict__ om, int k,
                                double* __restrict__ z0) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= D * k) return;
  const int p = e / k, j = e % k;
  double acc = 0.0;
  for (int64_t n = 0; n < N; ++n) acc += static_cast<double>(load_x(num, cnt, n, p, D)) * om[n * k + j];
  z0[e] = acc;
}

// X^T Omega for the transposed branch's small splits (N < d rows, k <= 16):
// one wave per feature p, lane l summing rows l, l + 64, ... for all k
// columns (every load of a lane independent), then a fixed-order DPP wave sum
// per column.  The thread-per-output kernel above walked all N rows as one
// dependent chain of loads: 59 us for a 229-row split (r04 dataset_splits).
// X^T Omega for the transposed branch's small splits (N < d rows, k <= 16)
// on the f64 matrix pipe: workgroup `blk` owns the 16-feature tile blk of z0
// (all k <= 16 columns: one 16x16 output tile), its 4 waves split the N / 4
// MFMA k-steps (v_mfma_f64_16x16x4f64, A = X^T rows, B = Omega rows; every
// k-step's operands loaded before the first MFMA) and their sums are added in
// wave order.  (r05's wave per feature read 64 rows per load instruction and
// chained its iterations: 5 / 11 us at 100 / 203 rows, r06 kernel trace; a
// lane-per-feature loop over the rows with Omega in LDS measured 31 us.)
constexpr int kXtK = 16;
constexpr int kXtMaxN = 320;  // rows (the branch has N < d <= 320)
template <typename TX, bool CNT>
__device__ __forceinline__ void xt_omega_wave_body(const TX* __restrict__ num, const float* __restrict__ cnt,
                                                   int64_t N, int D, const double* __restrict__ om, int k,
                                                   double* __restrict__ z0, int blk) {
  __shared__ double s_part[4][256];
  constexpr int kS = (kXtMaxN / 4 + 3) / 4;  // k-steps per wave (20)
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int n_ = static_cast<int>(N);
  const int p = blk * 16 + (lane & 15), j = lane & 15;
  double xa[kS], ob[kS];
#pragma unroll
  for (int u = 0; u < kS; ++u) {
    const int n = 4 * (wave + 4 * u) + (lane >> 4);
    const bool ok = n < n_;
    xa[u] = (ok && p < D) ? static_cast<double>(CNT ? load_x(num, cnt, n, p, D)
                                                    : num[static_cast<int64_t>(n) * D + p])
                          : 0.0;
    ob[u] = (ok && j < k) ? om[static_cast<int64_t>(n) * k + j] : 0.0;
  }
  f64x4 acc = {0, 0, 0, 0};
#pragma unroll
  for (int u = 0; u < kS; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[u], ob[u], acc, 0, 0, 0);
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) s_part[wave][((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = acc[reg];
  __syncthreads();
  const int e = threadIdx.x;
  if (e < 256) {
    const double v = s_part[0][e] + s_part[1][e] + s_part[2][e] + s_part[3][e];
    const int pr = blk * 16 + (e >> 4), jc = e & 15;
    if (pr < D && jc < k) z0[pr * k + jc] = v;
  }
}
template <typename TX, bool CNT = false>
__global__ __launch_bounds__(256) void xt_omega_wave_kernel(const TX* __restrict__ num,
                                                            const float* __restrict__ cnt,
                                                            int64_t N, int D,
                                                            const double* __restrict__ om, int k,
                                                            double* __restrict__ z0) {
  xt_omega_wave_body<TX, CNT>(num, cnt, N, D, om, k, z0, blockIdx.x);
}

// ------------------------------------------------------------------ pc_solve
#ifdef MMB_PC_PROBE  // phase timestamps for tools/pc_probe.hip (never in libmmb)
__device__ unsigned long long g_pc_probe[64];
// The marks go to LDS and are copied out at the end of the kernel
// (PC_PROBE_FLUSH): a global store per mark put its completion wait into the
// next barrier's phase (r05: ~4 us of a round's update phase was the mark).
__device__ __forceinline__ unsigned long long* pc_probe_lds() {
  __shared__ unsigned long long s[64];
  return s;
}
#define PC_MARK(i)                                                               \
  do {                                                                           \
    __syncthreads();                                                             \
    if (threadIdx.x == 0 && blockIdx.x == 0) pc_probe_lds()[i] = wall_clock64(); \
  } while (0)
// one wave's own mark (no barrier): lane 0 of the calling wave, workgroup 0
#define PC_WMARK(i)                                                                     \
  do {                                                                                  \
    if ((threadIdx.x & 63) == 0 && blockIdx.x == 0) pc_probe_lds()[i] = wall_clock64(); \
  } while (0)
#define PC_PROBE_FLUSH()                                                                    \
  do {                                                                                      \
    __syncthreads();                                                                        \
    if (blockIdx.x == 0 && threadIdx.x < 64) g_pc_probe[threadIdx.x] = pc_probe_lds()[threadIdx.x]; \
  } while (0)
#else
#define PC_MARK(i) \
  do {             \
  } while (0)
#define PC_WMARK(i) \
  do {              \
  } while (0)
#define PC_PROBE_FLUSH() \
  do {                   \
  } while (0)
#endif
constexpr int kMaxD = 512;
constexpr int kMaxK = 16;
constexpr int kSolveNT = 1024;

// Modified Gram-Schmidt, twice ("twice is enough"), on the columns of Z [D][k]
// by one wave.  Lane l owns rows p = l (mod 64), so LDS needs no cross-lane
// ordering; dot products travel through shuffles.
__device__ void orth_wave(double* Z, int D, int k, int lane) {
  for (int j = 0; j < k; ++j) {
    for (int pass = 0; pass < 2; ++pass) {
      for (int i = 0; i < j; ++i) {
        double d = 0.0;
        for (int p = lane; p < D; p += kWave) d += Z[p * k + i] * Z[p * k + j];
        d = wave_sum(d);
        for (int p = lane; p < D; p += kWave) Z[p * k + j] -= d * Z[p * k + i];
      }
    }
    double nn = 0.0;
    for (int p = lane; p < D; p += kWave) nn += Z[p * k + j] * Z[p * k + j];
    nn = wave_sum(nn);
    const double inv = 1.0 / sqrt(nn);
    for (int p = lane; p < D; p += kWave) Z[p * k + j] *= inv;
  }
}

// GZ = G Z.  Thread (g, p) owns row p and column group g (MC columns), so
// every thread of the workgroup works (D=300: 3 groups of 4 of the 11
// columns).  G symmetric: read column p (coalesced across p; the groups
// re-read it from L1).  Z is read from LDS as a broadcast.
template <int MC>
__device__ void gz_product_mc(const double* __restrict__ G, const double* Z, double* GZ, int D,
                              int k, int groups) {
  const int t = threadIdx.x;
  const int g = t / D, p = t - g * D;
  if (g >= groups) return;
  const int j0 = g * MC;
  double acc[MC];
#pragma unroll
  for (int j = 0; j < MC; ++j) acc[j] = 0.0;
  const double* gcol = G + p;
  const double* zr = Z + j0;
#pragma unroll 16
  for (int q = 0; q < D; ++q) {
    const double gq = gcol[static_cast<int64_t>(q) * D];
#pragma unroll
    for (int j = 0; j < MC; ++j)
      if (j0 + j < k) acc[j] = fma(gq, zr[q * k + j], acc[j]);
  }
#pragma unroll
  for (int j = 0; j < MC; ++j)
    if (j0 + j < k) GZ[p * k + j0 + j] = acc[j];
}

__device__ void gz_product(const double* __restrict__ G, const double* Z, double* GZ, int D, int k) {
  const int maxg = kSolveNT / D;  // >= 2 for D <= 512
  if (maxg >= 3 && k <= 12) {
    gz_product_mc<4>(G, Z, GZ, D, k, (k + 3) / 4);
  } else {
    gz_product_mc<8>(G, Z, GZ, D, k, (k + 7) / 8);
  }
}

// M[i][j] = sum_p X[p][i] Y[p][j] for the k x k block, all waves.
__device__ void small_gram(const double* X, const double* Y, double* M, int D, int k) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  for (int e = wave; e < k * k; e += kSolveNT / kWave) {
    const int i = e / k, j = e % k;
    double d = 0.0;
    for (int p = lane; p < D; p += kWave) d += X[p * k + i] * Y[p * k + j];
    d = wave_sum(d);
    if (lane == 0) M[e] = d;
  }
}

// Cyclic Jacobi on symmetric A [k][k] (LDS) by one wave; V <- eigenvectors (columns).
__device__ void jacobi_wave(double* A, double* V, int k, int lane) {
  for (int r = lane; r < k * k; r += kWave) V[r] = (r / k == r % k) ? 1.0 : 0.0;
  wave_lds_sync();
  for (int sweep = 0; sweep < 40; ++sweep) {
    double off = 0.0, dia = 0.0;
    for (int r = lane; r < k * k; r += kWave) {
      const int i = r / k, j = r % k;
      const double a = A[r];
      if (i < j) off += a * a;
      else if (i == j) dia += a * a;
    }
    off = wave_sum(off);
    dia = wave_sum(dia);
    // converged when the off-diagonal mass is ~1e-14 of the diagonal's: the
    // rotations' own rounding (~1e-16 |lambda_max|) keeps regenerating
    // off-diagonal entries, so a bar at the rounding level itself is never met
    if (off <= 1e-28 * dia) break;
    bool rotated = false;
    for (int p = 0; p < k - 1; ++p) {
      for (int q = p + 1; q < k; ++q) {
        const double apq = A[p * k + q];
        const double app = A[p * k + p], aqq = A[q * k + q];
        // at rounding level next to both diagonal entries: rotating changes nothing
        if (fabs(apq) <= 2e-16 * (fabs(app) + fabs(aqq))) continue;
        rotated = true;
        const double theta = (aqq - app) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        double arp = 0.0, arq = 0.0, vrp = 0.0, vrq = 0.0;
        if (lane < k) {
          arp = A[lane * k + p];
          arq = A[lane * k + q];
          vrp = V[lane * k + p];
          vrq = V[lane * k + q];
        }
        wave_lds_sync();
        if (lane < k) {
          if (lane != p && lane != q) {
            const double np_ = c * arp - s * arq, nq = s * arp + c * arq;
            A[lane * k + p] = np_;
            A[p * k + lane] = np_;
            A[lane * k + q] = nq;
            A[q * k + lane] = nq;
          }
          V[lane * k + p] = c * vrp - s * vrq;
          V[lane * k + q] = s * vrp + c * vrq;
        }
        if (lane == 0) {
          A[p * k + p] = app - t * apq;
          A[q * k + q] = aqq + t * apq;
          A[p * k + q] = 0.0;
          A[q * k + p] = 0.0;
        }
        wave_lds_sync();
      }
    }
    if (!rotated) break;
  }
}

// Orthonormalise the columns of Z [D][k] with the whole workgroup:
// column equilibration, then CholeskyQR twice (W = Z^T Z by all waves,
// Cholesky + triangular inverse by one wave, Z <- Z L^{-T} row-parallel).
// Falls back to wave-0 MGS^2 if a Cholesky pivot is not positive (only for
// extreme ill-conditioning, kappa >~ 1e8).
__device__ void orth_block(double* Z, int D, int k, double* sW, double* sL, double* sLi,
                           int* s_fail) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  for (int pass = 0; pass < 3; ++pass) {
    small_gram(Z, Z, sW, D, k);
    if (tid == 0) *s_fail = 0;
    __syncthreads();
    if (pass == 0) {  // equilibrate: unit column norms
      if (tid < D) {
        for (int j = 0; j < k; ++j) Z[tid * k + j] *= 1.0 / sqrt(sW[j * k + j]);
      }
      __syncthreads();
      continue;
    }
    if (wave == 0) {
      for (int e = lane; e < k * k; e += kWave) sL[e] = 0.0;
      wave_lds_sync();
      for (int j = 0; j < k; ++j) {
        if (lane == 0) {
          double s = sW[j * k + j];
          for (int m = 0; m < j; ++m) s -= sL[j * k + m] * sL[j * k + m];
          if (!(s > 0.0)) *s_fail = 1;
          sL[j * k + j] = sqrt(s > 0.0 ? s : 1.0);
        }
        wave_lds_sync();
        if (lane > j && lane < k) {
          double s = sW[lane * k + j];
          for (int m = 0; m < j; ++m) s -= sL[lane * k + m] * sL[j * k + m];
          sL[lane * k + j] = s / sL[j * k + j];
        }
        wave_lds_sync();
      }
      if (lane < k) {  // Linv column `lane`
        const int c = lane;
        for (int i = 0; i < k; ++i) {
          double s = (i == c) ? 1.0 : 0.0;
          for (int m = c; m < i; ++m) s -= sL[i * k + m] * sLi[m * k + c];
          sLi[i * k + c] = (i < c) ? 0.0 : s / sL[i * k + i];
        }
      }
    }
    __syncthreads();
    if (*s_fail) {
      if (wave == 0) orth_wave(Z, D, k, lane);
      __syncthreads();
      return;
    }
    if (tid < D) {  // row p: z <- z L^{-T}, i.e. z_new[j] = sum_{m<=j} z[m] Linv[j][m]
      double z[kMaxK];
#pragma unroll
      for (int m = 0; m < kMaxK; ++m) z[m] = (m < k) ? Z[tid * k + m] : 0.0;
      for (int j = 0; j < k; ++j) {
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < kMaxK; ++m)
          if (m <= j) s += z[m] * sLi[j * k + m];
        Z[tid * k + j] = s;
      }
    }
    __syncthreads();
  }
}

__device__ void symmetrize(double* M, int k) {
  for (int e = threadIdx.x; e < k * k; e += blockDim.x) {
    const int i = e / k, j = e % k;
    if (i < j) {
      const double m = 0.5 * (M[i * k + j] + M[j * k + i]);
      M[i * k + j] = m;
      M[j * k + i] = m;
    }
  }
}

__global__ __launch_bounds__(kSolveNT) void pc_solve_kernel(const double* __restrict__ G, int D,
                                                            const double* __restrict__ z0, int k,
                                                            int npc, int n_iter, int transposed,
                                                            double* __restrict__ pc_out) {
  __shared__ double sZ[kMaxD * kMaxK];
  __shared__ double sGZ[kMaxD * kMaxK];
  __shared__ double sA[kMaxK * kMaxK], sV[kMaxK * kMaxK], sW[kMaxK * kMaxK];
  __shared__ double sL[kMaxK * kMaxK], sLi[kMaxK * kMaxK], sT[kMaxK * kMaxK];
  __shared__ double sy[kMaxK], sv[kMaxD];
  __shared__ double s_rd[kSolveNT / kWave];
  __shared__ double s_rv[kSolveNT / kWave];
  __shared__ int s_ri[kSolveNT / kWave];
  __shared__ int s_order[kMaxK];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;

  __shared__ int s_fail;
  PC_MARK(0);
  for (int e = tid; e < D * k; e += kSolveNT) sZ[e] = z0[e];
  __syncthreads();
  orth_block(sZ, D, k, sW, sL, sLi, &s_fail);
  PC_MARK(1);
  for (int it = 0; it < n_iter; ++it) {
    gz_product(G, sZ, sGZ, D, k);
    __syncthreads();
    PC_MARK(2 + 2 * it);
    for (int e = tid; e < D * k; e += kSolveNT) sZ[e] = sGZ[e];
    __syncthreads();
    orth_block(sZ, D, k, sW, sL, sLi, &s_fail);
    PC_MARK(3 + 2 * it);
  }
  gz_product(G, sZ, sGZ, D, k);
  __syncthreads();
  PC_MARK(40);

  if (transposed) {
    small_gram(sZ, sGZ, sA, D, k);  // Q^T G Q
    __syncthreads();
    symmetrize(sA, k);
    __syncthreads();
  } else {
    small_gram(sZ, sGZ, sW, D, k);   // W = Z^T G Z
    small_gram(sGZ, sGZ, sT, D, k);  // H = (GZ)^T (GZ)
    __syncthreads();
    symmetrize(sW, k);
    symmetrize(sT, k);
    __syncthreads();
    if (wave == 0) {
      // Cholesky W = L L^T
      for (int e = lane; e < k * k; e += kWave) sL[e] = 0.0;
      wave_lds_sync();
      for (int j = 0; j < k; ++j) {
        if (lane == 0) {
          double s = sW[j * k + j];
          for (int m = 0; m < j; ++m) s -= sL[j * k + m] * sL[j * k + m];
          sL[j * k + j] = sqrt(s);
        }
        wave_lds_sync();
        if (lane > j && lane < k) {
          double s = sW[lane * k + j];
          for (int m = 0; m < j; ++m) s -= sL[lane * k + m] * sL[j * k + m];
          sL[lane * k + j] = s / sL[j * k + j];
        }
        wave_lds_sync();
      }
      // Linv: lane c solves L x = e_c (column c)
      if (lane < k) {
        const int c = lane;
        for (int i = 0; i < k; ++i) {
          double s = (i == c) ? 1.0 : 0.0;
          for (int m = c; m < i; ++m) s -= sL[i * k + m] * sLi[m * k + c];
          sLi[i * k + c] = (i < c) ? 0.0 : s / sL[i * k + i];
        }
      }
      wave_lds_sync();
      // A = Linv H Linv^T
      for (int e = lane; e < k * k; e += kWave) {
        const int i = e / k, j = e % k;
        double s = 0.0;
        for (int m = 0; m < k; ++m) s += sLi[i * k + m] * sT[m * k + j];
        sV[e] = s;  // scratch: Linv H
      }
      wave_lds_sync();
      for (int e = lane; e < k * k; e += kWave) {
        const int i = e / k, j = e % k;
        double s = 0.0;
        for (int m = 0; m < k; ++m) s += sV[i * k + m] * sLi[j * k + m];
        sA[e] = s;
      }
      wave_lds_sync();
      for (int e = lane; e < k * k; e += kWave) {
        const int i = e / k, j = e % k;
        if (i < j) {
          const double m = 0.5 * (sA[i * k + j] + sA[j * k + i]);
          sA[i * k + j] = m;
          sA[j * k + i] = m;
        }
      }
      wave_lds_sync();
    }
    __syncthreads();
  }

  PC_MARK(41);
  if (wave == 0) {
    jacobi_wave(sA, sV, k, lane);
    if (lane == 0) {  // eigenvalues descending (selection; first max wins ties)
      bool used[kMaxK];
      for (int j = 0; j < k; ++j) used[j] = false;
      for (int c = 0; c < k; ++c) {
        int best = -1;
        for (int j = 0; j < k; ++j)
          if (!used[j] && (best < 0 || sA[j * k + j] > sA[best * k + best])) best = j;
        used[best] = true;
        s_order[c] = best;
      }
    }
  }
  __syncthreads();
  PC_MARK(42);

  for (int c = 0; c < npc; ++c) {
    const int col = s_order[c];
    if (!transposed) {
      if (tid < k) {  // y = Linv^T u
        double s = 0.0;
        for (int m = 0; m < k; ++m) s += sLi[m * k + tid] * sV[m * k + col];
        sy[tid] = s;
      }
      __syncthreads();
    }
    double v = 0.0;
    if (tid < D) {
      if (transposed) {
        for (int j = 0; j < k; ++j) v += sZ[tid * k + j] * sV[j * k + col];
      } else {
        for (int j = 0; j < k; ++j) v += sGZ[tid * k + j] * sy[j];
      }
      sv[tid] = v;
    }
    // norm and first argmax |v|
    double nn = wave_sum(v * v);
    double best = (tid < D) ? fabs(v) : -1.0;
    int bidx = (tid < D) ? tid : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ob = __shfl_xor(best, o, kWave);
      const int oi = __shfl_xor(bidx, o, kWave);
      if (ob > best || (ob == best && oi < bidx)) {
        best = ob;
        bidx = oi;
      }
    }
    if (lane == 0) {
      s_rd[wave] = nn;
      s_rv[wave] = best;
      s_ri[wave] = bidx;
    }
    __syncthreads();
    double tot = 0.0, bb = -1.0;
    int bi = 0x7fffffff;
    for (int w = 0; w < kSolveNT / kWave; ++w) {
      tot += s_rd[w];
      if (s_rv[w] > bb || (s_rv[w] == bb && s_ri[w] < bi)) {
        bb = s_rv[w];
        bi = s_ri[w];
      }
    }
    const double scale = (sv[bi] < 0.0 ? -1.0 : 1.0) / sqrt(tot);
    if (tid < D) pc_out[c * D + tid] = v * scale;
    __syncthreads();
  }
  PC_MARK(43);
}

// ------------------------------------------------------------------ pc_solve (D <= 320)
// The same solve with every D-long contraction on the fp64 matrix pipe
// (MFMA 16x16x4): the block is kept 16 columns wide in LDS (columns >= k and
// rows >= D zero), so
//   G Z      = 16-row tiles of G (A operand, read straight from L2: G is
//              symmetric, so a fragment is 16 consecutive doubles of 4 rows)
//              times Z (B operand from LDS);
//   X^T Y    = one 16x16 MFMA accumulator per wave over a quarter-strided
//              share of the rows, the 16 partials summed in a fixed order.
// Everything k x k (Cholesky, triangular inverse, Jacobi) stays on one wave.
constexpr int kP16MaxD = 320;
// 16 waves.  (8 waves with a software-pipelined G.Z product -- two 16-deep
// batches of G per lane in flight, which 128 VGPRs cannot hold -- measured
// slower: 0.340 vs 0.310 ms per solve; the products are not what bounds it.)
constexpr int kP16NT = 1024;
constexpr int kP16W = 16;  // block width (k <= 16)

struct P16Lds {
  double* Z;     // [Dp][16]
  double* GZ;    // [Dp][16]
  double* part;  // [16 waves][256]
};

// M (k x k, compact) = X^T Y over the Dp rows of two [Dp][16] blocks (NW
// waves: every thread of the workgroup).
template <int NW = kP16NT / kWave>
__device__ __forceinline__ void p16_gram(const double* X, const double* Y, int Dp, int k, double* part, double* M) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  f64x4 acc = {0, 0, 0, 0};
  for (int p = 4 * wave; p < Dp; p += 4 * NW) {
    const int o = (p + (lane >> 4)) * kP16W + (lane & 15);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(X[o], Y[o], acc, 0, 0, 0);
  }
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) part[wave * 256 + ((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = acc[reg];
  __syncthreads();
  if (tid < 256) {
    const int i = tid >> 4, j = tid & 15;
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += part[w * 256 + tid];
    if (i < k && j < k) M[i * k + j] = s;
  }
  __syncthreads();
}

// M1 = X1^T Y1 and M2 = X2^T Y2 (k x k, compact) in one pass over the Dp rows
// (the two sums as p16_gram's, one barrier pair instead of two).
template <int NW>
__device__ __forceinline__ void p16_gram2(const double* X1, const double* Y1, double* M1, const double* X2,
                                          const double* Y2, double* M2, int Dp, int k, double* part) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  f64x4 a1 = {0, 0, 0, 0}, a2 = {0, 0, 0, 0};
  for (int p = 4 * wave; p < Dp; p += 4 * NW) {
    const int o = (p + (lane >> 4)) * kP16W + (lane & 15);
    a1 = __builtin_amdgcn_mfma_f64_16x16x4f64(X1[o], Y1[o], a1, 0, 0, 0);
    a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(X2[o], Y2[o], a2, 0, 0, 0);
  }
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    part[wave * 256 + ((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = a1[reg];
    part[(NW + wave) * 256 + ((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = a2[reg];
  }
  __syncthreads();
  if (tid < 512) {
    const int e = tid & 255, i = e >> 4, j = e & 15, h = tid >> 8;
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += part[(h * NW + w) * 256 + e];
    if (i < k && j < k) (h ? M2 : M1)[i * k + j] = s;
  }
  __syncthreads();
}

// GZ = G Z (G symmetric [D][D] in global memory / L2).  16 k-steps of loads
// are issued before their MFMAs (one L2 latency per batch, not per step);
// two accumulators alternate so consecutive MFMAs are independent.  (32-step
// batches measured slower on MI355X: 24.3 vs 19.5 us per product.)  The p16
// helpers are force-inlined: as called functions they were compiled with
// flat loads and spilled their operands to scratch around every call
// (pc_solve 0.316 -> 0.310 ms).
constexpr int kGzBatch = 16;
__device__ __forceinline__ void p16_gz(const double* __restrict__ G, int D, int Dp, const double* Z, double* GZ) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int mt = Dp / 16;
  const int nbat = (Dp + 4 * kGzBatch - 1) / (4 * kGzBatch);
  for (int t = wave; t < mt; t += kP16NT / kWave) {
    const int p = t * 16 + (lane & 15);
    const int pc = min(p, D - 1);
    f64x4 acc0 = {0, 0, 0, 0}, acc1 = acc0;
    // clamped addresses, unconditional loads, selected after (keeps loads in
    // flight; a batch index past the last re-reads it, an L2 hit)
    auto load = [&](int bt, double (&g)[kGzBatch]) {
      const int q0 = 4 * kGzBatch * min(bt, nbat - 1);
#pragma unroll
      for (int s = 0; s < kGzBatch; ++s) {
        const int q = q0 + 4 * s + (lane >> 4);
        g[s] = G[static_cast<int64_t>(min(q, D - 1)) * D + pc];
      }
    };
    auto comp = [&](int bt, const double (&g)[kGzBatch]) {
      const int q0 = 4 * kGzBatch * bt;
#pragma unroll
      for (int s = 0; s < kGzBatch; ++s) {
        const int q = q0 + 4 * s + (lane >> 4);
        const double a = (p < D && q < D) ? g[s] : 0.0;
        const double b = Z[min(q, Dp - 1) * kP16W + (lane & 15)];
        if (s & 1) {
          acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc1, 0, 0, 0);
        } else {
          acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc0, 0, 0, 0);
        }
      }
    };
    double g0[kGzBatch];
    for (int bt = 0; bt < nbat; ++bt) {
      load(bt, g0);
      comp(bt, g0);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
      GZ[(t * 16 + (lane >> 4) + 4 * reg) * kP16W + (lane & 15)] = acc0[reg] + acc1[reg];
  }
}

// 1 / sqrt(x) to f64 precision: the v_rsq_f64 estimate + two Newton steps
// (r03: replaces sqrt + an f64 division per Cholesky pivot)
__device__ __forceinline__ double rsqrt_f64(double x) {
  double y = __builtin_amdgcn_rsq(x);
  const double h = 0.5 * x;
  y = y * fma(-h * y, y, 1.5);
  y = y * fma(-h * y, y, 1.5);
  return y;
}

// Cholesky of the k x k SPD matrix whose row `lane` (lane < k) is w[]
// (registers; zero elsewhere) by one wave, pivots inverted once (rsqrt_f64).
// Writes L^{-1} (compact, sLi) and returns, in x[], lane c's column of
// L^{-1}; L itself goes to sL column by column (sL[j * 16 + i], internal).
// *fail is set if a pivot is not positive (the pivot is then replaced by 1).
//
// r06b: both loops run over the pivots at run time -- one copy of a step,
// where r05 unrolled all 16 (~6 KB of code per instance, five instances in
// the multi-workgroup solve: after other kernels the solve's first pass
// through each missed in the instruction cache, +16 us over a warm solve,
// tools/pc_probe "cold").  Lane i keeps row i of the trailing matrix
// SHIFTED, so pivot j is always w[0]: d_jj = lane j's w[0], l_ij = w[0] /
// sqrt(d_jj), and w[m - 1] <- w[m] - l_ij l_(j+m)j (a readlane of lane j + m).  The substitution is right-looking in the same
// shifted form: lane c's t = e_c, step i: x_i = t_0 / L_ii to LDS, t_(m-1) <-
// t_m - L_(i+m)i x_i (column i of L as LDS broadcasts).
//
// REL: *fail is also set where a pivot is not above tau times its diagonal
// entry dg (lane j: W_jj).  That ratio is sin^2 of the angle between column
// j of the block and the columns before it: below it the factor is positive
// but Z = B L^-T cancels 1 / sqrt(ratio) digits of B.
template <bool REL = false>
__device__ __forceinline__ void p16_chol_regs(double (&w)[kMaxK], double* sL, double* sLi, int k,
                                              int lane, int* fail, double (&x)[kMaxK], int mark = 31,
                                              double dg = 0.0, double tau = 0.0) {
  double* rl = sLi + kMaxK * kMaxK - kMaxK;  // the reciprocal pivots: sLi's last row until the end
  bool bad = false;
  PC_WMARK(mark);
#pragma unroll 1
  for (int j = 0; j < k; ++j) {
    const double djj = readlane_f64(w[0], j);
    bad = bad || !(djj > 0.0);
    if constexpr (REL) bad = bad || !(djj > tau * readlane_f64(dg, j));
    const double p = djj > 0.0 ? djj : 1.0;
    const double r = rsqrt_f64(p);
    const double lij = (lane == j) ? p * r : (lane > j ? w[0] * r : 0.0);
    if (lane < kMaxK) sL[j * kMaxK + lane] = lij;
    if (lane == 0) rl[j] = r;
    // every lane's l_(j+m)j first (lanes past k hold zero rows: l = 0
    // there), then the updates -- no per-column branches, so the broadcasts
    // issue back to back
    double lm[kMaxK];
#pragma unroll
    for (int m = 1; m < kMaxK; ++m) lm[m] = readlane_f64(lij, j + m);
#pragma unroll
    for (int m = 1; m < kMaxK; ++m) w[m - 1] = w[m] - lij * lm[m];
    w[kMaxK - 1] = 0.0;
  }
  if (bad && lane == 0) *fail = 1;
  wave_lds_sync();
  PC_WMARK(mark + 1);
  double t[kMaxK];
#pragma unroll
  for (int m = 0; m < kMaxK; ++m) t[m] = (m == lane) ? 1.0 : 0.0;
  // in order within the wave: step i reads rl[i] before any lane's store of
  // row i can reach it (k = 16: row 15 is rl's storage)
#pragma unroll 1
  for (int i = 0; i < k; ++i) {
    // column i of L below the diagonal (rows past 15 clamped: they only
    // reach t's rows past k, which never become t[0] before the loop ends)
    double li[kMaxK];
#pragma unroll
    for (int m = 1; m < kMaxK; ++m) li[m] = sL[i * kMaxK + min(i + m, kMaxK - 1)];
    const double xi = t[0] * rl[i];
    if (lane < k) sLi[i * k + lane] = (i < lane) ? 0.0 : xi;
#pragma unroll
    for (int m = 1; m < kMaxK; ++m) t[m - 1] = t[m] - li[m] * xi;
    t[kMaxK - 1] = 0.0;
  }
  PC_WMARK(mark + 2);
  wave_lds_sync();
#pragma unroll
  for (int i = 0; i < kMaxK; ++i) x[i] = (i < k && lane < k) ? sLi[i * k + lane] : 0.0;
}

// Cholesky W = L L^T (k x k, compact, LDS) and Linv = L^{-1} by one wave.
__device__ __forceinline__ void p16_chol(const double* sW, double* sL, double* sLi, int k, int lane, int* fail) {
  double w[kMaxK], x[kMaxK];
#pragma unroll
  for (int m = 0; m < kMaxK; ++m) w[m] = (lane < k && m < k) ? sW[lane * k + m] : 0.0;
  p16_chol_regs(w, sL, sLi, k, lane, fail, x);
}

// Top eigenvector of the symmetric positive semi-definite A (k x k, compact,
// LDS) by one wave: B = A (16 x 16, zero padded) is squared 32 times on the
// fp64 matrix pipe, B <- B B / trace(B B), so B -> v v^T along the top
// eigenvector (any ratio lambda_2 / lambda_1 < 1 - 1e-9 is resolved); the
// f64 16x16 accumulator layout (row (l>>4) + 4 r, column l&15) IS the operand
// layout of the next squaring (B symmetric), so B never leaves the
// registers.  v = the column of B with the largest diagonal, normalised, then
// two Rayleigh steps on A.  Returns lambda = v^T A v; u[0..k) = v.
__device__ double p16_top_eig(const double* A, int k, int lane, double* u) {
  const int c = lane & 15, r0 = lane >> 4;
  f64x4 b;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = r0 + 4 * r;
    b[r] = (row < k && c < k) ? A[row * k + c] : 0.0;
  }
  for (int it = 0; it < 32; ++it) {
    f64x4 acc = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(b[s], b[s], acc, 0, 0, 0);
    double tr = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r0 + 4 * r == c) tr += acc[r];
    tr = wave_sum_dpp(tr);
    const double inv = tr > 0.0 ? 1.0 / tr : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) b[r] = acc[r] * inv;
    // from the second squaring on trace(B) = 1, and trace(B B) = 1 exactly
    // when B is rank one: B is then v v^T to rounding and more squarings
    // change nothing (r03: 32 -> ~5 squarings on separated spectra, ~8 us)
    if (it >= 1 && tr >= 1.0 - 1e-14) break;
  }
  // column with the largest diagonal entry (first index on ties)
  double dg = -1.0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (r0 + 4 * r == c && c < k) dg = b[r];
  int jb = c;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double od = __shfl_xor(dg, o, kWave);
    const int oj = __shfl_xor(jb, o, kWave);
    if (od > dg || (od == dg && oj < jb)) {
      dg = od;
      jb = oj;
    }
  }
  if (c == jb) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r0 + 4 * r < k) u[r0 + 4 * r] = b[r];
  }
  wave_lds_sync();
  double lam = 0.0;
  for (int step = 0; step < 3; ++step) {
    // lane i < k: y_i = (A u)_i; normalise
    double y = 0.0;
    if (lane < k) {
      for (int m = 0; m < k; ++m) y += A[lane * k + m] * u[m];
    }
    const double ui = lane < k ? u[lane] : 0.0;
    const double nrm2 = wave_sum_dpp(lane < k ? ui * ui : 0.0);
    lam = wave_sum_dpp(ui * y) / nrm2;  // Rayleigh quotient of the current u
    if (step == 2) {
      if (lane < k) u[lane] = ui / sqrt(nrm2);
    } else {
      const double yn = sqrt(wave_sum_dpp(y * y));
      wave_lds_sync();
      if (lane < k) u[lane] = yn > 0.0 ? y / yn : ui;
    }
    wave_lds_sync();
  }
  return lam;
}

// Orthonormalise the k columns of Z [Dp][16]: equilibration, CholeskyQR twice;
// wave-0 MGS^2 on a compact copy if a pivot fails (extreme ill-conditioning).
// npass = 3: equilibration + CholeskyQR2 (orthonormal to rounding); npass =
// 2: equilibration + one CholeskyQR -- a well-conditioned basis of the same
// span, all the subspace iteration needs between products (the span, not the
// basis, fixes the result: span(Q) = span(G^q Omega)).
__device__ __forceinline__ void p16_orth(double* Z, int D, int Dp, int k, double* part, double* sW, double* sL,
                         double* sLi, int* s_fail, int npass = 3) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  for (int pass = 0; pass < npass; ++pass) {
    p16_gram(Z, Z, Dp, k, part, sW);
    if (pass == 0) {
      if (tid < D) {
        for (int j = 0; j < k; ++j) Z[tid * kP16W + j] *= 1.0 / sqrt(sW[j * k + j]);
      }
      __syncthreads();
      continue;
    }
    if (wave == 0) {
      if (lane == 0) *s_fail = 0;
      wave_lds_sync();
      p16_chol(sW, sL, sLi, k, lane, s_fail);
    }
    __syncthreads();
    if (*s_fail) {
      if (wave == 0) {
        // compact [D][k] copy through the partial buffer (D*k <= 16*256 doubles)
        for (int e = lane; e < D * k; e += kWave) part[e] = Z[(e / k) * kP16W + e % k];
        wave_lds_sync();
        orth_wave(part, D, k, lane);
        for (int e = lane; e < D * k; e += kWave) Z[(e / k) * kP16W + e % k] = part[e];
      }
      __syncthreads();
      return;
    }
    if (tid < D) {  // row p: z <- z L^{-T}
      double z[kP16W];
#pragma unroll
      for (int m = 0; m < kP16W; ++m) z[m] = Z[tid * kP16W + m];
      for (int j = 0; j < k; ++j) {
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < kP16W; ++m)
          if (m <= j) s += z[m] * sLi[j * k + m];
        Z[tid * kP16W + j] = s;
      }
    }
    __syncthreads();
  }
}

// The k x k scratch of the solve's tail (LDS, one set per workgroup).
struct P16Small {
  double *A, *V, *W, *L, *Li, *T, *y, *U;  // [16 x 16] each (y: [16]; U: npc x 16)
  double *rd, *rv;                         // [16 waves]
  int *ri, *fail;
};

// The Rayleigh-Ritz tail of the solve (every thread of a 16-wave workgroup):
// from the final block Z and its product GZ = G Z (both [Dp][16] in LDS) to
// the npc components in pc_out -- sklearn's randomized_svd after its range
// finder: W = Z^T G Z, H = (GZ)^T (GZ), the k x k generalised eigenproblem
// H y = s^2 W y (Cholesky of W, A = L^-1 H L^-T), v = GZ L^-T u, svd_flip
// (extmath.py:537-566); the transposed branch takes A = Q^T G Q, v = Q u.
template <int NW = kP16NT / kWave>
__device__ __forceinline__ void p16_tail(const double* Z, const double* GZ, int D, int Dp, int k,
                                         int npc, int transposed, double* part, const P16Small& sm,
                                         double* __restrict__ pc_out, const double* Hpre = nullptr,
                                         bool wpre = false) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  if (transposed) {
    p16_gram<NW>(Z, GZ, Dp, k, part, sm.A);  // Q^T G Q
    symmetrize(sm.A, k);
    __syncthreads();
  } else {
    if (!wpre) p16_gram<NW>(Z, GZ, Dp, k, part, sm.W);  // W = Z^T G Z (wpre: the caller's, in sm.W)
    if (Hpre) {                           // H = (GZ)^T (GZ), summed by the caller
      if (threadIdx.x < k * k) sm.T[threadIdx.x] = Hpre[threadIdx.x];
      __syncthreads();
    } else {
      p16_gram<NW>(GZ, GZ, Dp, k, part, sm.T);
    }
    symmetrize(sm.W, k);
    symmetrize(sm.T, k);
    __syncthreads();
    if (wave == 0) {
      p16_chol(sm.W, sm.L, sm.Li, k, lane, sm.fail);  // a failed pivot is clamped (W is SPD here)
      // A = Linv H Linv^T on the matrix pipe (r05; two k^3 LDS loops before):
      // U^T = H Linv^T lands in the accumulator layout that is the B operand
      // of A = Linv U^T (k-step st = U^T's rows 4 st .. 4 st + 3), zero padded
      // past k
      const int r = lane & 15, g = lane >> 4;
      f64x4 ut = {0, 0, 0, 0}, av = {0, 0, 0, 0};
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const int m = 4 * st + g;
        const bool in = r < k && m < k;
        ut = __builtin_amdgcn_mfma_f64_16x16x4f64(in ? sm.T[r * k + m] : 0.0, in ? sm.Li[r * k + m] : 0.0, ut, 0, 0,
                                                  0);
      }
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const int m = 4 * st + g;
        av = __builtin_amdgcn_mfma_f64_16x16x4f64((r < k && m < k) ? sm.Li[r * k + m] : 0.0, ut[st], av, 0, 0, 0);
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int i = g + 4 * reg;
        if (i < k && r < k) sm.A[i * k + r] = av[reg];
      }
      wave_lds_sync();
      for (int e = lane; e < k * k; e += kWave) {
        const int i = e / k, j = e % k;
        if (i < j) {
          const double m = 0.5 * (sm.A[i * k + j] + sm.A[j * k + i]);
          sm.A[i * k + j] = m;
          sm.A[j * k + i] = m;
        }
      }
      wave_lds_sync();
    }
    __syncthreads();
  }
  PC_MARK(41);
  if (wave == 0) {  // top npc eigenvectors of A, largest first (deflation)
    for (int c = 0; c < npc; ++c) {
      double* u = sm.U + c * kMaxK;
      const double lam = p16_top_eig(sm.A, k, lane, u);
      if (c + 1 < npc) {
        for (int e = lane; e < k * k; e += kWave) sm.A[e] -= lam * u[e / k] * u[e % k];
        wave_lds_sync();
      }
    }
  }
  __syncthreads();
  PC_MARK(42);

  for (int c = 0; c < npc; ++c) {
    const double* u = sm.U + c * kMaxK;
    if (!transposed) {
      if (tid < k) {  // y = Linv^T u
        double s = 0.0;
        for (int m = 0; m < k; ++m) s += sm.Li[m * k + tid] * u[m];
        sm.y[tid] = s;
      }
      __syncthreads();
    }
    // v = row tid of Z u (transposed) or GZ y; each thread starts its row at
    // column tid mod k: rows are 128 B apart, so lanes reading one column
    // fell on 2 bank pairs (8-way conflicts)
    double v = 0.0;
    if (tid < D) {
      const double* row = (transposed ? Z : GZ) + tid * kP16W;
      const double* c = transposed ? u : sm.y;
      int j = tid % k;
      for (int q = 0; q < k; ++q) {
        v += row[j] * c[j];
        j = j + 1 == k ? 0 : j + 1;
      }
    }
    // norm and first argmax |v|
    double nn = wave_sum(v * v);
    double best = (tid < D) ? fabs(v) : -1.0;
    int bidx = (tid < D) ? tid : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ob = __shfl_xor(best, o, kWave);
      const int oi = __shfl_xor(bidx, o, kWave);
      if (ob > best || (ob == best && oi < bidx)) {
        best = ob;
        bidx = oi;
      }
    }
    if (lane == 0) {
      sm.rd[wave] = nn;
      sm.rv[wave] = best;
      sm.ri[wave] = bidx;
    }
    __syncthreads();
    double tot = 0.0, bb = -1.0;
    int bi = 0x7fffffff;
    for (int w = 0; w < NW; ++w) {
      tot += sm.rd[w];
      if (sm.rv[w] > bb || (sm.rv[w] == bb && sm.ri[w] < bi)) {
        bb = sm.rv[w];
        bi = sm.ri[w];
      }
    }
    if (tid == bi) part[0] = v;  // sign of the largest-|.| entry (svd_flip)
    __syncthreads();
    const double vbest = part[0];
    const double scale = (vbest < 0.0 ? -1.0 : 1.0) / sqrt(tot);
    if (tid < D) pc_out[c * D + tid] = v * scale;
    __syncthreads();
  }
  PC_MARK(43);
}

#define P16_SMALL_DECL                                                                      \
  __shared__ double sA[kMaxK * kMaxK], sV[kMaxK * kMaxK], sW[kMaxK * kMaxK];                 \
  __shared__ double sL[kMaxK * kMaxK], sLi[kMaxK * kMaxK], sT[kMaxK * kMaxK];                \
  __shared__ double sy[kMaxK];                                                               \
  __shared__ double s_rd[kP16NT / kWave];                                                    \
  __shared__ double s_rv[kP16NT / kWave];                                                    \
  __shared__ int s_ri[kP16NT / kWave];                                                       \
  __shared__ double sU[kMaxK * kMaxK]; /* eigenvectors of A, largest first */               \
  __shared__ int s_fail;                                                                     \
  const P16Small sm{sA, sV, sW, sL, sLi, sT, sy, sU, s_rd, s_rv, s_ri, &s_fail};

__global__ __launch_bounds__(kP16NT) void pc_solve16_kernel(const double* __restrict__ G, int D,
                                                              const double* __restrict__ z0, int k,
                                                              int npc, int n_iter, int transposed,
                                                              double* __restrict__ pc_out) {
  extern __shared__ __attribute__((aligned(16))) double p16_lds[];
  const int Dp = (D + 15) / 16 * 16;
  double* sZ = p16_lds;
  double* sGZ = sZ + Dp * kP16W;
  double* part = sGZ + Dp * kP16W;  // max(16 x 256, Dp x 16): partials / fallback copy
  P16_SMALL_DECL
  const int tid = threadIdx.x;

  PC_MARK(0);
  for (int e = tid; e < Dp * kP16W; e += kP16NT) {
    const int p = e / kP16W, j = e % kP16W;
    sZ[e] = (p < D && j < k) ? z0[p * k + j] : 0.0;
    sGZ[e] = 0.0;
  }
  __syncthreads();
  // one CholeskyQR pass between products, CholeskyQR2 for the block the
  // final Rayleigh-Ritz step uses (orthonormal to rounding, as before)
  p16_orth(sZ, D, Dp, k, part, sW, sL, sLi, &s_fail, n_iter > 0 ? 2 : 3);
  PC_MARK(1);
  double* Z = sZ;
  double* GZ = sGZ;
  for (int it = 0; it < n_iter; ++it) {
    p16_gz(G, D, Dp, Z, GZ);
    __syncthreads();
    PC_MARK(2 + 2 * it);
    double* t = Z; Z = GZ; GZ = t;  // the product becomes the block
    p16_orth(Z, D, Dp, k, part, sW, sL, sLi, &s_fail, it == n_iter - 1 ? 3 : 2);
    PC_MARK(3 + 2 * it);
  }
  p16_gz(G, D, Dp, Z, GZ);
  __syncthreads();
  PC_MARK(40);
  p16_tail(Z, GZ, D, Dp, k, npc, transposed, part, sm, pc_out);
  PC_PROBE_FLUSH();
}

// ------------------------------------------------------------------ pc_solve, multi-workgroup (r03)
// The same randomized-SVD replay with the D-long products spread over
// T = Dp / 16 workgroups (19 at D = 300), one per 16-row tile of G.  The
// single-workgroup solve spent ~20 us per G Z product (76 dependent MFMA
// k-steps per tile, two rounds of tiles over 16 waves, G re-read from L2)
// and ~16 us per orthonormalisation; here each workgroup keeps its 16 rows of
// G in registers for the whole solve (wave w: k-steps w, w + 16, ..), so a
// product is <= 5 MFMAs per wave plus a 16-way LDS sum, and the
// orthonormalisation needs only the block's k x k Gram, which the tiles
// contribute as partials.  Per power iteration ONE exchange: every workgroup
// publishes its tile Y_t = G_t Z (16 x 16) and P_t = Y_t^T Y_t with
// write-through (sc1) stores, drains them and adds one to an arrival counter
// (agent scope, relaxed); each polls the counter for T (it + 1) arrivals
// (bounded), acquires, and gathers all tiles with sc1 loads (CDNA guide
// Guideline 16, R1).  Then EVERY workgroup runs the identical equilibrated
// CholeskyQR on the identical data (W = sum_t P_t in tile order), so the next
// block Z is the same in all of them with no second exchange.  After the
// n_iter-th block, one more exchange gives the final product, and workgroup 0
// runs the Rayleigh-Ritz tail (p16_tail).  Between products the
// equilibration scales W itself (W' = d W d) instead of recomputing the Gram
// of the scaled block; the block entering the tail still gets CholeskyQR2.
// ws: [2][T][512] doubles of tiles (double-buffered by round parity: a round
// r + 2 write needs every workgroup past round r + 1's wait, hence done
// reading round r), then the arrival counter and the abort word (zero when
// the caller first hands ws over; workgroup 0 returns the counter to zero
// once every workgroup has made its last arrival, so a launch -- eager or a
// graph replay -- leaves ws ready for the next one).
constexpr int kPmMaxT = kP16MaxD / 16;  // tiles (20)

// tools/diag: a test shortens the bounded waits (mmb_diag_pc_wait_iters) and
// names one workgroup that never arrives (mmb_diag_pc_skip_arrival), so the
// count a wait polls for cannot be reached whatever the arrival skew: the
// timeout path runs deterministically
#ifndef MMB_HOOK_PM_WAIT_ITERS
#define MMB_HOOK_PM_WAIT_ITERS (1 << 20)
#endif
#ifndef MMB_HOOK_PM_SKIP_ARRIVAL
#define MMB_HOOK_PM_SKIP_ARRIVAL false
#endif
__device__ __forceinline__ bool pm_wait(unsigned* ctr, unsigned target, unsigned* abort_w,
                                        int32_t* flag) {
  const int iters = MMB_HOOK_PM_WAIT_ITERS;
  for (int it = 0; it < iters; ++it) {
    // the abort word first: a set word (another workgroup gave up, or a
    // workspace handed over dirty) ends the wait even where the count is met
    if (__hip_atomic_load(abort_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
    if (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target) return true;
    __builtin_amdgcn_s_sleep(4);
  }
  // ~0.5-1 s without the other workgroups, or an abort seen: give up, release
  // every waiter, and say so in the flag word whichever way the abort came (a
  // launch that found the word already set would otherwise leave only a NaN PC)
  __hip_atomic_store(abort_w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (flag) atomicOr(flag, MMB_FLAG_SYNC_TIMEOUT);
  return false;
}

// An arrival of round r must find the counter in [T r, T (r + 1)): every
// workgroup arrives at round r only after seeing T r arrivals, and no
// workgroup arrives at round r + 1 before all T of round r have.  A count
// outside that range is a counter this launch did not start from zero (a
// workspace handed over dirty): abort like a timeout instead of letting the
// waits pass before the other workgroups' tiles are written.
__device__ __forceinline__ bool pm_arrive(unsigned* ctr, int T, int r, unsigned* abort_w,
                                          int32_t* flag) {
  if (MMB_HOOK_PM_SKIP_ARRIVAL) return true;  // (tools/diag) never arrives
  const unsigned old = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (old >= static_cast<unsigned>(T * r) && old < static_cast<unsigned>(T * (r + 1))) return true;
  __hip_atomic_store(abort_w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (flag) atomicOr(flag, MMB_FLAG_SYNC_TIMEOUT);
  return false;
}

// Out [Dp][16] = In [Dp][16] M^T for a 16 x 16 M (row-major, zero past k;
// MT: M holds M^T, whose reads are conflict-free): the 16-row tiles over the
// NW waves, 4 MFMA k-steps each.  In != Out.
template <int NW = kP16NT / kWave, bool MT = false>
__device__ __forceinline__ void p16_rmul(const double* In, const double* M, double* Out, int Dp) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int t = wave; t < Dp / 16; t += NW) {
    f64x4 acc = {0, 0, 0, 0};
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const int m = 4 * st + (lane >> 4);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(In[(t * 16 + (lane & 15)) * kP16W + m],
                                                 MT ? M[m * kP16W + (lane & 15)] : M[(lane & 15) * kP16W + m],
                                                 acc, 0, 0, 0);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) Out[(t * 16 + (lane >> 4) + 4 * reg) * kP16W + (lane & 15)] = acc[reg];
  }
}

// Wave 0: the equilibrated Cholesky factor of a block's Gram W (k x k
// compact, LDS): d_j = 1 / sqrt(W_jj), d W d = L L^T, and on return
// M = L^-1 diag(d) (16 x 16, zero past k) is the right factor that
// orthonormalises the block: Z = B M^T (one CholeskyQR pass after
// equilibration, from the Gram alone).  d[] = the scales.  All in registers
// (lane i = row i); *fail as p16_chol.  Mt (optional) receives M^T, the
// layout whose MFMA B-operand reads are conflict-free (M's own reads
// M[j][m] for lanes j = 0..15 fall 16 doubles apart: 8-way LDS conflicts).
// EQ = false (r05, pc_solve_mc_kernel): no equilibration -- M = L^-1 of W
// itself.  Cholesky's backward error is invariant to diagonal scaling (the
// factor of D W D is D times W's, to rounding), so scaling W first changes
// neither which blocks factor nor the span Z keeps; it only put ~1 us of
// broadcasts and scalings on the round's critical path.  d is then not
// written (the MGS^2 fallback forms its scales from W).
// REL: a pivot at or below tau times its diagonal entry of W also sets *fail
// (p16_chol_regs).
template <bool EQ = true, bool REL = false>
__device__ __forceinline__ void p16_eq_chol(const double* W, double* L, double* Li, double* M,
                                            double* d, int k, int lane, int* fail, double* Mt = nullptr,
                                            double tau = 0.0) {
  double w[kMaxK], x[kMaxK];
  const double dg = (REL && !EQ && lane < k) ? W[lane * k + lane] : 1.0;  // (equilibrated: 1)
  PC_WMARK(30);
#pragma unroll
  for (int m = 0; m < kMaxK; ++m) w[m] = (lane < k && m < k) ? W[lane * k + m] : 0.0;
  double di = 1.0;
  if constexpr (EQ) {
    di = rsqrt_f64(lane < k ? W[lane * k + lane] : 1.0);
#pragma unroll
    for (int m = 0; m < kMaxK; ++m) w[m] *= di * readlane_f64(di, m);
    if (lane < kMaxK) d[lane] = lane < k ? di : 0.0;
  }
  if (lane == 0) *fail = 0;
  p16_chol_regs<REL>(w, L, Li, k, lane, fail, x, 37, dg, tau);  // probe marks 37-39
  if (lane < kP16W) {  // lane c: column c of L^-1 diag(d)
#pragma unroll
    for (int i = 0; i < kP16W; ++i) {
      const double v = (lane < k && i < k) ? (EQ ? x[i] * di : x[i]) : 0.0;
      M[i * kP16W + lane] = v;
      if (Mt) Mt[lane * kP16W + i] = v;
    }
  }
  wave_lds_sync();
  PC_WMARK(34);
}

// G2 = G G for the multi-workgroup solve's squared rounds (r06): one
// upper-triangle 16 x 16 tile (a <= b) per 4 waves, which split the MFMA
// k-steps (f64 16x16x4) and are summed in wave order; each element is written
// at (i, j) and (j, i) by ONE thread, so G2 is exactly symmetric.  190 tiles
// of ~19 k-steps each at d = 300.  Run by the solve's own extra workgroups
// (pc_solve_mc_kernel, beside its first round) or by pc_prep_kernel (the
// transposed start); the same k-steps per wave and the same sum order either
// way, so G2 is the same bit for bit.
constexpr int kSqNT = 256;
// G2 tiles per squaring workgroup of the solve's launch (two at a time): 2
// puts 95 workgroups beside the solve's 19 at d = 300, 4 puts 48 (fewer CUs
// held with the solve's LDS allocation).  Measured (r06, profiles/r06/sq2/):
// the solve alone 75.1 vs 76.7 us, MOSI's three-split graph 0.215 vs
// 0.216 ms, POM's 0.343 vs 0.344
constexpr int kSqPerWg = 2;
static_assert(kSqPerWg % 2 == 0, "two tiles per pass");
__device__ __forceinline__ void square_tile_ab(int blk, int T, int& a, int& b) {
  int rem = blk;
  a = 0;  // blk -> (a, b), a <= b, row-major over the upper triangle
  while (rem >= T - a) {
    rem -= T - a;
    ++a;
  }
  b = a + rem;
}
// wave wv (0-3) of the tile's group: its k-steps' MFMA partial into part4[wv]
__device__ __forceinline__ void square_tile_partials(const double* __restrict__ G, int D, int blk,
                                                     int wv, int lane, double* part4) {
  const int T = (D + 15) / 16;
  int a, b;
  square_tile_ab(blk, T, a, b);
  const int Ks = (D + 3) / 4;
  const int pa = a * 16 + (lane & 15), pb = b * 16 + (lane & 15);
  // every k-step's two operands loaded before the first MFMA (<= 20 k-steps
  // per wave at D <= 320): one round trip of G reads, not one per k-step group
  constexpr int kSqKs = (kP16MaxD / 4 + kSqNT / kWave - 1) / (kSqNT / kWave);  // 20
  double x[kSqKs], y[kSqKs];
#pragma unroll
  for (int u = 0; u < kSqKs; ++u) {
    const int st = wv + (kSqNT / kWave) * u;
    const int q = 4 * st + (lane >> 4);
    const bool okq = st < Ks && q < D;
    // A[i][k] = G[a16 + i][q] = G[q][a16 + i] (symmetric), B[k][j] = G[q][b16 + j]
    x[u] = (okq && pa < D) ? G[static_cast<int64_t>(q) * D + pa] : 0.0;
    y[u] = (okq && pb < D) ? G[static_cast<int64_t>(q) * D + pb] : 0.0;
  }
  f64x4 acc = {0, 0, 0, 0};
#pragma unroll
  for (int u = 0; u < kSqKs; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x[u], y[u], acc, 0, 0, 0);
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) part4[wv * 256 + ((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = acc[reg];
}
// element e (0-255) of the tile: the four partials in wave order, stored at
// (i, j) and (j, i); WT: write-through (agent-scope) stores for readers of
// the same launch on other XCDs
template <bool WT>
__device__ __forceinline__ void square_tile_store(int D, double* __restrict__ G2, int blk, int e,
                                                  const double* part4) {
  const int T = (D + 15) / 16;
  int a, b;
  square_tile_ab(blk, T, a, b);
  const int i = e >> 4, j = e & 15;
  double v = 0.0;
#pragma unroll
  for (int w = 0; w < kSqNT / kWave; ++w) v += part4[w * 256 + e];
  const int r = a * 16 + i, c = b * 16 + j;
  if (r < D && c < D && (a != b || i <= j)) {
    if (WT) {
      const unsigned long long bits = __builtin_bit_cast(unsigned long long, v);
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(G2 + static_cast<int64_t>(r) * D + c), bits,
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(G2 + static_cast<int64_t>(c) * D + r), bits,
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      G2[static_cast<int64_t>(r) * D + c] = v;
      G2[static_cast<int64_t>(c) * D + r] = v;
    }
  }
}

// Since r05 an implicit round exchanges the RAW product H_t = G_t B_r, which
// needs no factor of W_r, so the equilibrated Cholesky of W_r (the last wave) runs
// beside the whole exchange -- partials, publish, the wait for the other
// workgroups and the gather of H = G B_r -- instead of before it.  After the
// join every workgroup forms B_{r+1} = H M_r^T (the tiles Y_t of r04, the
// same MFMAs on the same operands) and W_{r+1} = B_{r+1}^T B_{r+1} from its
// own copy of the rows (per-wave partial Grams summed in a fixed wave order:
// identical in all workgroups), so the exchange carries 16 x 16 per tile
// instead of 16 x 32.  The partial waves synchronise among themselves through
// an LDS arrival counter while the last wave factors (s_barrier would wait
// for it).  A round whose factor fails (a pivot <= 0) drops H and runs a
// second exchange of G_t Z for the MGS^2-orthonormalised block; the round
// entering the tail is the r04 round (the factor beside the partials,
// explicit CholeskyQR2 rows for the transposed branch).  Exchange x
// (counting the extra ones) arrives at T x .. T (x + 1) - 1 and uses tile
// buffer x & 1.
//
// 8 waves, not r04's 16: at 1024 threads a wave has 128 VGPRs, and with the
// factor's 16-entry rows, the G fragments and the gather's loads in one
// kernel the compiler spilled ~70 VGPRs -- the G fragments reloaded from
// scratch before every MFMA, the gather's addresses spilled and reloaded
// around every load (probe: the round's non-factor work 2x slower than its
// operations).  At 512 threads there are 256.
constexpr int kPnNT = 512;
constexpr int kPnNW = kPnNT / kWave;                   // 8
constexpr int kPnPw = kPnNW - 1;                       // waves holding G (the last one factors)
constexpr int kPnKs = (kP16MaxD / 4 + kPnPw - 1) / kPnPw;  // k-steps of G per wave (12)
constexpr int kPnGu = (kPmMaxT * 256 + kPnPw * kWave - 1) / (kPnPw * kWave);  // gather loads per thread (12)
// The direct branch's last factor: the smallest pivot / diagonal ratio at
// which the implicit round (raw products times M^T) still enters the tail;
// below it the explicit MGS^2 block does.  The first component then stays
// within ~eps / sqrt(ratio) = 1e-13 of the oracle; at n_iter = 7 mild
// spectra (l1/l11 <= ~300) leave this ratio at 0.7 to 1, so they never take
// the fallback (it fires from about l1/l2 = 1e5, or l1/l11 = 1e8 spread
// evenly).
constexpr double kPnTailPivot = 1e-6;

// ABL (tools build only, timing ablations, results invalid): 1 skips the
// round's B_{r+1} / W_{r+1} update, 2 skips the round's factor
template <int ABL = 0>
__global__ __launch_bounds__(kPnNT) void pc_solve_mc_kernel(const double* __restrict__ G,
                                                               double* __restrict__ G2, int nsq_wg, int D,
                                                               const double* __restrict__ z0, int k,
                                                               int npc, int n_iter, int transposed,
                                                               double* __restrict__ pc_out,
                                                               double* xbuf, unsigned* ctl,
                                                               int32_t* flag) {
  extern __shared__ __attribute__((aligned(16))) double p16_lds[];
  const int Dp = (D + 15) / 16 * 16;
  int T = Dp / 16;
  double* sZ = p16_lds;          // H = G B_r (implicit rounds); the explicit block Z
  double* sY = sZ + Dp * kP16W;  // the raw block B_r (z0, then G Z_{r-1}); G Z for the tail
  double* part = sY + Dp * kP16W;  // max(16 x 256, Dp x 16)
  P16_SMALL_DECL
  __shared__ double sHt[256], sYt[256], sM[256], sM2[256], sd[kMaxK];
  __shared__ int s_abort;
  __shared__ unsigned s_bar;
  int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int t = blockIdx.x;
  unsigned* ctr = ctl;
  unsigned* abort_w = ctl + 1;
  unsigned* sq_ctr = ctl + 2;  // the squaring workgroups' arrivals

  if (t >= T) {
    // workgroups T .. T + nsq_wg - 1 (r06b): G2 = G G, kSqPerWg tiles each,
    // two at a time (waves 0-3 and 4-7), while the solve's workgroups run
    // their first round by G.  Write-through stores, drained by every wave,
    // then one arrival; the solve waits for all nsq_wg before its first
    // squared round.  An arrival that finds the count already met is a
    // workspace handed over dirty.
    double* part4 = p16_lds + 2 * Dp * kP16W + (wave >> 2) * 4 * 256;
    const int ntiles = T * (T + 1) / 2;
#pragma unroll 1
    for (int pass = 0; pass < kSqPerWg / 2; ++pass) {
      const int blk = kSqPerWg * (t - T) + 2 * pass + (wave >> 2);
      if (blk < ntiles) square_tile_partials(G, D, blk, wave & 3, lane, part4);
      __syncthreads();
      if (blk < ntiles) square_tile_store<true>(D, G2, blk, tid & 255, part4);
      __syncthreads();  // part4 is read before the next pass writes it
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      const unsigned old = __hip_atomic_fetch_add(sq_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old >= static_cast<unsigned>(nsq_wg)) {
        __hip_atomic_store(abort_w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (flag) atomicOr(flag, MMB_FLAG_SYNC_TIMEOUT);
      }
    }
    return;
  }

  // this workgroup's 16 rows of the round's matrix as MFMA A fragments on
  // waves 0-6 (symmetric: row p of the tile = column p, 16 consecutive
  // doubles per k-row: coalesced); wave 7 is free for the k x k factor that
  // overlaps the rest.  Since r06 n_sq = (n_iter - 1) / 2 rounds multiply
  // by G2 = G G, each standing for two power iterations: span(G^7 Z0) =
  // span(G2^3 G Z0), so the PC is sklearn's to rounding, with 4 exchange
  // rounds instead of 7.  The schedule is G, then the n_sq rounds by G2, then
  // what is left (n_iter even: one more) by G, and the tail by G: the first
  // round needs no G2, so the squaring workgroups of this launch (nsq_wg > 0)
  // form it beside that round instead of a launch in front of the solve
  const int n_sq = (G2 && n_iter >= 3) ? (n_iter - 1) / 2 : 0;
  double ga[kPnKs];
  // (G2 from this launch's squaring workgroups is read after the acquire
  // that follows their arrivals, so plain loads see it)
  auto load_rows = [&](const double* M) {
    const int p = t * 16 + (lane & 15);
#pragma unroll
    for (int j = 0; j < kPnKs; ++j) {
      const int q = 4 * (wave + kPnPw * j) + (lane >> 4);
      ga[j] = (wave < kPnPw && p < D && q < D) ? M[static_cast<int64_t>(q) * D + p] : 0.0;
    }
  };
  load_rows(G);
  // waves 0-6: their partial products of this tile of G with a [Dp][16] block
  auto tile_partials = [&](const double* B) {
    if (wave < kPnPw) {
      f64x4 acc = {0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < kPnKs; ++j) {
        const int q = 4 * (wave + kPnPw * j) + (lane >> 4);
        if (4 * (wave + kPnPw * j) < Dp)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ga[j], B[q * kP16W + (lane & 15)], acc, 0, 0, 0);
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) part[wave * 256 + ((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = acc[reg];
    }
  };
  // ... summed over the waves in a fixed order (threads 0-255; the caller
  // synchronises before and after); tr: the tile's transpose
  auto tile_sum = [&](double* out, bool tr = false) {
    if (tid < 256) {
      double s = 0.0;
#pragma unroll
      for (int w = 0; w < kPnPw; ++w) s += part[w * 256 + tid];
      out[tr ? (tid & 15) * 16 + (tid >> 4) : tid] = s;
    }
  };
  auto tile_product = [&](const double* B, double* out) {
    tile_partials(B);
    __syncthreads();
    tile_sum(out);
    __syncthreads();
  };
  // the barrier of waves 0-6 while wave 7 factors: every wave adds one
  // arrival to an LDS counter after its LDS writes, then polls for the
  // phase's 7 arrivals (the counter only grows within a launch)
  unsigned bar_target = 0;
  auto bar_pw = [&]() {
    bar_target += kPnPw;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) {
      __hip_atomic_fetch_add(&s_bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      while (__hip_atomic_load(&s_bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < bar_target)
        __builtin_amdgcn_s_sleep(1);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
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
  // wave 0: publishes this workgroup's 16 x 16 tile for exchange x with
  // write-through 8-byte stores, drains them and adds one arrival; then waits
  // for all T (not after the final exchange, except workgroup 0, which then
  // returns the counter to zero: every workgroup has made its last arrival,
  // so the next launch -- eager or a graph replay -- finds it at 0 with no
  // memset node in front of it).  A failed arrival or wait sets s_abort.
  auto publish = [&](const double* tile, int x, bool final_x) {
    double* xb = xbuf + static_cast<int64_t>(x & 1) * T * 256;
    wave_lds_sync();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = lane + kWave * u;
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(xb + t * 256 + e),
                         __builtin_bit_cast(unsigned long long, tile[e]), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) {
      // release: the tile stores above are visible at agent scope before
      // the arrival that announces them
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      if (!pm_arrive(ctr, T, x, abort_w, flag)) {
        s_abort = 1;
      } else if (!(final_x && t != 0)) {
        if (!pm_wait(ctr, static_cast<unsigned>(T * (x + 1)), abort_w, flag)) {
          s_abort = 1;
        } else if (final_x) {
          __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(sq_ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // acquire: the gather reads the other workgroups' tiles only after
        // their arrivals were observed (the barrier that follows releases the
        // other waves of this workgroup)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      }
    }
  };
  // every tile of exchange x into dst by the first nthr threads (element f =
  // tid + nthr u of the T x 256 published doubles, copied to dst[f]: a
  // row-major tile lands as rows t*16.. of a [Dp][16] block, a transposed one
  // as a [T][16][16] stack of transposed tiles), all of a thread's loads (sc1,
  // 8 B) issued before any is used (a load-then-store loop waited ~1.5 us per
  // load)
  auto gather = [&](double* dst, int x, int nthr) {
    if (tid < nthr) {
      const double* xb = xbuf + static_cast<int64_t>(x & 1) * T * 256;
      double v[kPnGu];
#pragma unroll
      for (int u = 0; u < kPnGu; ++u) {
        const int f = tid + nthr * u;
        v[u] = f < T * 256 ? __builtin_bit_cast(double, __hip_atomic_load(reinterpret_cast<const unsigned long long*>(xb + f),
                                                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                           : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kPnGu; ++u) {
        const int f = tid + nthr * u;
        if (f < T * 256) dst[f] = v[u];
      }
    }
  };
  // no caller may go on with a stale PC: an aborted solve leaves NaN in
  // pc_out (every aborting workgroup writes the same NaNs; workgroup 0
  // cannot complete the tail once any workgroup has left).  After a barrier.
  auto aborted = [&]() -> bool {
    if (!s_abort) return false;
    for (int e = tid; e < npc * D; e += kPnNT) pc_out[e] = __builtin_nan("");
    return true;
  };

  for (int e = tid; e < Dp * kP16W; e += kPnNT) {
    const int p = e / kP16W, j = e % kP16W;
    sY[e] = (p < D && j < k) ? z0[p * k + j] : 0.0;
    sZ[e] = 0.0;
  }
  if (tid == 0) {
    s_abort = 0;
    s_bar = 0;
  }
  __syncthreads();
  PC_MARK(0);
  p16_gram<kPnNW>(sY, sY, Dp, k, part, sW);  // W_0 = B_0^T B_0 (every workgroup: identical)
  PC_MARK(1);

  int x = 0;  // the exchange
  const int T0 = T, k0 = k;
  const int n_rounds = n_iter - n_sq;  // 1 + n_sq + (n_iter - 1 - 2 n_sq)
  for (int r = 0; r < n_rounds; ++r) {
    if (n_sq > 0 && r == 1) {
      if (nsq_wg > 0) {  // G2 from this launch's squaring workgroups
        if (tid == 0) {
          if (!pm_wait(sq_ctr, static_cast<unsigned>(nsq_wg), abort_w, flag)) s_abort = 1;
          // the acquire's L1 invalidate completes asynchronously: wait for it
          // before the barrier releases the other waves' plain loads of G2
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        if (aborted()) return;
      }
      load_rows(G2);
    }
    if (n_sq > 0 && r == 1 + n_sq) load_rows(G);  // G2's rounds done
    {
      // the round's LDS addresses, bounds and per-lane indices are rebuilt
      // from an opaque zero every round: left loop-invariant, the compiler
      // hoisted all of them out of the loop (hundreds of values held across
      // the kernel) and spilled the G fragments and the gather's addresses
      int zo = 0;
      asm volatile("" : "+s"(zo));
      sZ = p16_lds + zo;
      sY = sZ + Dp * kP16W;
      part = sY + Dp * kP16W;
      T = T0 + zo;
      k = k0 + zo;
      tid = static_cast<int>(threadIdx.x) + zo;
      lane = tid & (kWave - 1);
    }
    if (wave == kPnPw) {
      if (!(ABL & 2)) p16_eq_chol<false>(sW, sL, sLi, sM, sd, k, lane, &s_fail, sM2);  // M_r, beside the exchange
    } else {
      tile_partials(sY);
      bar_pw();
      tile_sum(sHt, true);  // H_t^T, H_t = G_t B_r
      bar_pw();
      if (wave == 0) {
        publish(sHt, x, false);
        PC_WMARK(2 + 3 * r);
      }
      bar_pw();
      gather(sZ, x, kPnPw * kWave);  // H = G B_r as T transposed tiles
      if (wave == 0) PC_WMARK(3 + 3 * r);
    }
    ++x;
    __syncthreads();  // the join: M_r, s_fail and H
    PC_MARK(44 + 2 * r);
    if (aborted()) return;
    if (s_fail) {
      // the equilibrated rows of B_r orthonormalised by MGS^2 (H is dropped),
      // then a second exchange of G_t Z
      for (int e = tid; e < Dp * kP16W; e += kPnNT) {
        const int p = e / kP16W, j = e % kP16W;
        sZ[e] = (p < D && j < k) ? sY[e] * rsqrt_f64(sW[j * k + j]) : 0.0;  // the equilibrated rows
      }
      __syncthreads();
      mgs(sZ);
      tile_product(sZ, sHt);
      if (wave == 0) publish(sHt, x, false);
      __syncthreads();
      if (aborted()) return;
      gather(sY, x, kPnNT);  // B_{r+1} = G Z
      ++x;
      __syncthreads();
      p16_gram<kPnNW>(sY, sY, Dp, k, part, sW);  // W_{r+1}
    } else if (!(ABL & 1)) {
      // B_{r+1} = H M_r^T tile by tile (all 8 waves), each wave's tiles' Grams
      // accumulated in its MFMA registers; W_{r+1} = their fixed-order sum.
      // Both operands are read from transposed copies (H's tiles as
      // gathered, M^T from the factor): lane (i, k) reads element 16 k + i,
      // conflict-free, where the rows' own layout put the 16 i of a read 128 B
      // apart (8-way bank conflicts: the update took ~5 us a round, r05
      // tools/pc_probe/rmul_bench.hip).  The tile's Gram Y^T Y takes its
      // operands straight from the accumulator: its k-step st is Y's rows
      // 4 st .. 4 st + 3, which is acc[st] in both operand layouts.
      f64x4 pa = {0, 0, 0, 0};
      for (int tt = wave; tt < T; tt += kPnNW) {
        f64x4 acc = {0, 0, 0, 0};
#pragma unroll
        for (int st = 0; st < 4; ++st) {
          const int m = 4 * st + (lane >> 4);
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sZ[tt * 256 + m * 16 + (lane & 15)],
                                                     sM2[m * kP16W + (lane & 15)], acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) sY[(tt * 16 + (lane >> 4) + 4 * reg) * kP16W + (lane & 15)] = acc[reg];
#pragma unroll
        for (int st = 0; st < 4; ++st) pa = __builtin_amdgcn_mfma_f64_16x16x4f64(acc[st], acc[st], pa, 0, 0, 0);
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) part[wave * 256 + ((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = pa[reg];
      if (wave == 0) PC_WMARK(35);
      __syncthreads();
      if (wave == 0) PC_WMARK(36);
      if (tid < 256) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kPnNW; ++w) s += part[w * 256 + tid];
        const int i = tid >> 4, j = tid & 15;
        if (i < k && j < k) sW[i * k + j] = s;
      }
      __syncthreads();
    }
    PC_MARK(45 + 2 * r);
  }

  if (n_sq > 0 && n_rounds == 1 + n_sq) load_rows(G);  // (the tail's product is by G)
  if (!transposed) {
    // The direct branch's last round (r06) as an implicit round: the RAW
    // product H_t = G_t B is exchanged beside the factor of W (as in the
    // loop), and workgroup 0 alone forms Z = B M^T and G Z = H M^T after the
    // join -- the factor no longer precedes the exchange (r05: factor 5.6 us,
    // then the Y_t exchange 4.5 us, back to back).  The other workgroups
    // arrive without waiting; workgroup 0 waits for all T and, once the
    // factor held, returns the counter to zero.  A failed factor (pivot <= 0)
    // falls through to the explicit MGS^2 block below with exchange x + 1:
    // every workgroup is still there (they return only after the join).
    // So does a factor with a pivot at or below kPnTailPivot of its diagonal
    // entry: Z = B M^T and G Z = H M^T then cancel 1 / sqrt(ratio) digits of
    // the raw B and H, and no later product damps what the tail's W and H
    // get from that (a dominant first component and few iterations -- the
    // block after a squared round straight into the tail: 1e-11 in the first
    // component at l1/l11 = 1e6, n_iter = 3, with every pivot positive).
    if (wave == kPnPw) {
      p16_eq_chol<false, true>(sW, sL, sLi, sM, sd, k, lane, &s_fail, sM2, kPnTailPivot);
    } else {
      tile_partials(sY);
      bar_pw();
      tile_sum(sHt, true);  // H_t^T
      bar_pw();
      if (wave == 0) {
        double* xb = xbuf + static_cast<int64_t>(x & 1) * T * 256;
        wave_lds_sync();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int e = lane + kWave * u;
          __hip_atomic_store(reinterpret_cast<unsigned long long*>(xb + t * 256 + e),
                             __builtin_bit_cast(unsigned long long, sHt[e]), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
          if (!pm_arrive(ctr, T, x, abort_w, flag)) {
            s_abort = 1;
          } else if (t == 0) {
            if (!pm_wait(ctr, static_cast<unsigned>(T * (x + 1)), abort_w, flag)) s_abort = 1;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
          }
        }
      }
    }
    __syncthreads();  // the join: M, s_fail, the arrival
    PC_MARK(44 + 2 * n_iter);
    if (aborted()) return;
    if (!s_fail) {
      if (t != 0) return;  // the tail runs on workgroup 0 only
      if (tid == 0) {
        __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(sq_ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      p16_rmul<kPnNW, true>(sY, sM2, part, Dp);  // Z = B M^T (into the scratch block)
      gather(sZ, x, kPnNT);                        // H as T transposed tiles
      __syncthreads();
      for (int tt = wave; tt < T; tt += kPnNW) {  // G Z = H M^T (sY free: B is in Z)
        f64x4 acc = {0, 0, 0, 0};
#pragma unroll
        for (int st = 0; st < 4; ++st) {
          const int m = 4 * st + (lane >> 4);
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sZ[tt * 256 + m * 16 + (lane & 15)],
                                                     sM2[m * kP16W + (lane & 15)], acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) sY[(tt * 16 + (lane >> 4) + 4 * reg) * kP16W + (lane & 15)] = acc[reg];
      }
      __syncthreads();
      if (Dp * kP16W >= 2 * kPnNW * 256) {
        double* zb = part;  // Z into sZ's place, the H tiles' block becomes the scratch
        part = sZ;
        sZ = zb;
      } else {
        // Dp < 256: the H tiles' block ([Dp][16]) is smaller than the scratch
        // the two Grams below need (2 x 8 waves x 256 partials), and G Z lies
        // right behind it -- as the scratch it let those partials overwrite
        // G Z's first rows (a wrong PC at every d <= 240 of the direct
        // branch).  Copy Z over H instead; `part` keeps its own block.
        for (int e = tid; e < Dp * kP16W; e += kPnNT) sZ[e] = part[e];
        __syncthreads();
      }
      PC_MARK(45 + 2 * n_iter);
    } else {
      // the explicit block's exchange follows: no workgroup may arrive at
      // x + 1 before all T arrived at x (pm_arrive's range check), so the
      // workgroups that did not wait above wait now
      if (t != 0 && tid == 0 && !pm_wait(ctr, static_cast<unsigned>(T * (x + 1)), abort_w, flag))
        s_abort = 1;
      __syncthreads();
      if (aborted()) return;
      ++x;
    }
  }
  // the transposed branch (an orthonormal Q: CholeskyQR2 rows) and a failed
  // pivot (MGS^2): explicit rows Z, then the final exchange of Y_t = G_t Z
  if (transposed || s_fail) {
    if (transposed) {  // (the direct branch factored above)
      if (wave == kPnPw) {
        p16_eq_chol<false>(sW, sL, sLi, sM, sd, k, lane, &s_fail, sM2);
      } else {
        tile_partials(sY);
      }
      __syncthreads();
      PC_MARK(44 + 2 * n_iter);
    }
    if (s_fail) {  // the equilibrated rows, orthonormalised by MGS^2
      for (int e = tid; e < Dp * kP16W; e += kPnNT) {
        const int p = e / kP16W, j = e % kP16W;
        sZ[e] = (p < D && j < k) ? sY[e] * rsqrt_f64(sW[j * k + j]) : 0.0;  // the equilibrated rows
      }
      __syncthreads();
      mgs(sZ);
    } else {
      p16_rmul<kPnNW>(sY, sM, sZ, Dp);  // Z1 = B M1^T
      __syncthreads();
      p16_gram<kPnNW>(sZ, sZ, Dp, k, part, sW);  // second CholeskyQR pass on the rows
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
        p16_rmul<kPnNW>(sZ, sM2, sY, Dp);  // Z = Z1 L2^-T (sY free: B is no longer needed)
        __syncthreads();
        for (int e = tid; e < Dp * kP16W; e += kPnNT) sZ[e] = sY[e];
        __syncthreads();
      }
    }
    tile_product(sZ, sYt);  // Y_t = G_t Z
    if (wave == 0) publish(sYt, x, true);
    if (t != 0) return;  // the tail runs on workgroup 0 only
    __syncthreads();
    PC_MARK(45 + 2 * n_iter);
    if (aborted()) return;
    gather(sY, x, kPnNT);  // G Z
    __syncthreads();
  }
  // the direct branch's two Grams in one pass: H = (G Z)^T (G Z), W = Z^T G Z
  // (the transposed branch forms its own Q^T G Q in the tail)
  if (!transposed) p16_gram2<kPnNW>(sY, sY, sT, sZ, sY, sW, Dp, k, part);
  PC_MARK(40);
  p16_tail<kPnNW>(sZ, sY, D, Dp, k, npc, transposed, part, sm, pc_out, sT, !transposed);
  // a workspace handed over with a stale count in (0, T) lets the final wait
  // pass early; the overshooting arrivals set the abort word.  Re-read it
  // after the tail so a PC that raced them is overwritten with NaN (the flag
  // word stays the primary signal)
  __syncthreads();
  if (__hip_atomic_load(abort_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    for (int e = tid; e < npc * D; e += kPnNT) pc_out[e] = __builtin_nan("");
  PC_PROBE_FLUSH();
}

__device__ __forceinline__ void gram_square_tile(const double* __restrict__ G, int D,
                                                 double* __restrict__ G2, int blk) {
  __shared__ double part[kSqNT / kWave][256];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  square_tile_partials(G, D, blk, wave, lane, &part[0][0]);
  __syncthreads();
  square_tile_store<false>(D, G2, blk, threadIdx.x, &part[0][0]);
}

// The transposed branch's start in ONE launch (r06): workgroups [0, nsq)
// square G (gram_square_tile), the next ceil(D / 4) form z0 = X^T Omega_n
// (xt_omega_wave_kernel's body: one wave per feature).  Two launches of ~5
// and ~11 us back to back before the solve of every dataset split (POM's
// and MOSI's small ones: n < d).
__global__ __launch_bounds__(kSqNT) void pc_prep_kernel(const double* __restrict__ G, int D,
                                                        double* __restrict__ G2, int nsq,
                                                        const float* __restrict__ X, int64_t N,
                                                        const double* __restrict__ om, int k,
                                                        double* __restrict__ z0) {
  if (static_cast<int>(blockIdx.x) < nsq) {
    gram_square_tile(G, D, G2, blockIdx.x);
    return;
  }
  xt_omega_wave_body<float, false>(X, nullptr, N, D, om, k, z0, static_cast<int>(blockIdx.x) - nsq);
}

inline size_t p16_lds_bytes(int d) {
  const size_t dp = (d + 15) / 16 * 16;
  return (2 * dp * kP16W + (dp * kP16W > 16 * 256 ? dp * kP16W : 16 * 256)) * sizeof(double);
}

}  // namespace mmb

using namespace mmb;

extern "C" int mmb_xt_omega(const float* num, const float* cnt, int64_t n, int d,
                            const double* omega, int k, double* z0, hipStream_t stream) {
  MMB_REQUIRE(num && omega && z0 && n >= 0 && d > 0 && k > 0);
  // the wave kernel is for the transposed branch's small splits: at large N
  // each of its d waves would re-read all of Omega (N x k)
  if (k <= kXtK && n <= kXtMaxN && cnt)  // (the solver's k = npc + 10 <= 16)
    xt_omega_wave_kernel<float, true><<<static_cast<int>(ceil_div(d, 16)), 256, 0, stream>>>(num, cnt, n, d, omega, k, z0);
  else if (k <= kXtK && n <= kXtMaxN)
    xt_omega_wave_kernel<float><<<static_cast<int>(ceil_div(d, 16)), 256, 0, stream>>>(num, cnt, n, d, omega, k, z0);
  else
    xt_omega_kernel<float><<<static_cast<int>(ceil_div(static_cast<int64_t>(d) * k, 256)), 256, 0, stream>>>(num, cnt, n, d, omega, k, z0);
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

extern "C" int mmb_pc_solve(const double* g, int d, const double* z0, int k, int npc, int n_iter,
                            int transposed, double* pc_out, hipStream_t stream) {
  MMB_REQUIRE(g && z0 && pc_out && d > 1 && d <= kMaxD && k >= 1 && k <= kMaxK);
  MMB_REQUIRE(npc >= 1 && npc <= k && n_iter >= 0);
  // a block wider than the space: no k > d columns of R^d are orthonormal.
  // A rank-deficient block with k <= d is fine -- MGS^2 normalises the
  // columns past the rank into the complement of G's range, where they add
  // nothing -- but with k > d there is no complement: they land back inside
  // the span, Z^T Z is not the identity, and the tail, which takes Z as
  // orthonormal (the transposed branch's ordinary eigenproblem of Z^T G Z;
  // the direct branch's Cholesky of a singular W, its failed pivots clamped),
  // returns a wrong or NaN PC.  The caller narrows the block to d columns,
  // which already span everything (pipeline.pc_solve)
  MMB_REQUIRE(k <= d);
  if (d <= kP16MaxD) {
    const size_t lds = p16_lds_bytes(d);
    allow_dynamic_lds<&pc_solve16_kernel>(p16_lds_bytes(kP16MaxD));  // once, for the widest d
    pc_solve16_kernel<<<1, kP16NT, lds, stream>>>(g, d, z0, k, npc, n_iter, transposed, pc_out);
  } else {
    pc_solve_kernel<<<1, kSolveNT, 0, stream>>>(g, d, z0, k, npc, n_iter, transposed, pc_out);
  }
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

__global__ __launch_bounds__(256) void step_status_kernel(const int32_t* __restrict__ flag,
                                                          const double* __restrict__ pc, int n,
                                                          int32_t bit, int32_t* __restrict__ out) {
  bool bad = false;
  for (int e = threadIdx.x; e < n; e += blockDim.x) bad |= !isfinite(pc[e]);
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) out[0] = (flag ? flag[0] : 0) | (bad ? bit : 0);
}

extern "C" int mmb_step_status(const int32_t* flag, const double* pc, int n, int32_t nonfinite_bit,
                               int32_t* out, hipStream_t stream) {
  MMB_REQUIRE(pc && out && n >= 0);
  step_status_kernel<<<1, 256, 0, stream>>>(flag, pc, n, nonfinite_bit, out);
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

// The multi-workgroup solve's workspace, laid out from d in this one place:
//   control words | tiles | G2 | z0
// (byte offsets from ws; what mmb_pc_solve_mc_ws_bytes sizes, mmb_pc_solve_mc_xt
// fills and launch_solve_mc hands to the kernel)
namespace {
struct SolveWs {
  char* base;
  size_t xbuf_off, g2_off, z0_off, bytes;
  SolveWs(void* ws, int d) : base(static_cast<char*>(ws)) {
    const size_t n = d > 0 ? d : 0;
    xbuf_off = 16;  // after the arrival counter and the abort word (a 16-byte block)
    g2_off = xbuf_off + 2 * (n / 16 + 1) * 512 * sizeof(double);  // two rounds of tiles Y_t | P_t
    z0_off = g2_off + n * n * sizeof(double);       // (r06: the squared rounds' matrix)
    bytes = z0_off + n * kP16W * sizeof(double);    // (mmb_pc_solve_mc_xt: X^T Omega, d x 16)
  }
  unsigned* ctl() const { return reinterpret_cast<unsigned*>(base); }
  double* xbuf() const { return reinterpret_cast<double*>(base + xbuf_off); }
  double* g2() const { return reinterpret_cast<double*>(base + g2_off); }
  double* z0() const { return reinterpret_cast<double*>(base + z0_off); }
};
}  // namespace

// squared rounds for the top component only: npc = 2 lost the second
// component's last digits (3.4e-9 of the reference's g3b rows against the
// 1e-9 bar) -- G2 keeps the dominant directions to rounding, not the smaller
// ones the later components live in
static bool solve_squares(int npc, int n_iter) { return n_iter >= 3 && npc == 1; }

static int launch_solve_mc(const double* g, int d, const double* z0, int k, int npc, int n_iter,
                           int transposed, double* pc_out, void* ws, int32_t* flag, bool g2_ready,
                           hipStream_t stream) {
  const int T = (d + 15) / 16;
  const SolveWs w(ws, d);
  unsigned* ctl = w.ctl();
  double* xbuf = w.xbuf();
  double* g2 = w.g2();
  // G2 ready (pc_prep_kernel) or formed by nsq_wg extra workgroups of the
  // solve's own launch, two tiles each, beside its first round (r06b: a
  // launch in front of the solve before, ~5 us on the step's critical path)
  int nsq_wg = 0;
  if (!solve_squares(npc, n_iter)) {
    g2 = nullptr;
  } else if (!g2_ready) {
    nsq_wg = (T * (T + 1) / 2 + kSqPerWg - 1) / kSqPerWg;
  }
  allow_dynamic_lds<&pc_solve_mc_kernel<0>>(p16_lds_bytes(kP16MaxD));  // once, for the widest d
  // no memset node here: the counter / abort words must be zero when the
  // caller first hands ws over, and a completed solve leaves them zero.  The
  // r04 launcher enqueued a 16-byte hipMemsetAsync of them instead; captured
  // into a HIP graph, that node wrote an address-like 64-bit value over BOTH
  // words on every replay after the first (ctl = [0x14ABxxxx, 0x7BE2]:
  // tools/dbg/replay_cause.py, r05a).  The garbage count passed every wait at
  // once, so the workgroups gathered tiles that were not yet written: a wrong
  // PC (39 of 40 replays of the solve alone) or a NaN one where the Cholesky
  // of the inconsistent block broke down (the r04e split failure), with no
  // flag.  Since r05 every arrival checks the count it finds (pm_arrive) and
  // every wait the abort word first, so a dirty workspace aborts with
  // MMB_FLAG_SYNC_TIMEOUT and a NaN PC instead
#ifndef MMB_HOOK_SOLVE_LAUNCH  // (tools/diag: MMB_PC_SOLVE_V1, the r04 kernel; MMB_PC_ABL ablations)
#define MMB_HOOK_SOLVE_LAUNCH(rc) false
#endif
  {
    int rc_ = MMB_OK;
    if (MMB_HOOK_SOLVE_LAUNCH(rc_)) return rc_;
  }
  pc_solve_mc_kernel<<<T + nsq_wg, kPnNT, p16_lds_bytes(d), stream>>>(g, g2, nsq_wg, d, z0, k, npc, n_iter,
                                                                        transposed, pc_out, xbuf, ctl, flag);
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

extern "C" size_t mmb_pc_solve_mc_ws_bytes(int d) { return SolveWs(nullptr, d).bytes; }

extern "C" int mmb_pc_solve_mc(const double* g, int d, const double* z0, int k, int npc, int n_iter,
                               int transposed, double* pc_out, void* ws, int32_t* flag,
                               hipStream_t stream) {
  MMB_REQUIRE(g && z0 && pc_out && ws && d > 1 && d <= kP16MaxD && k >= 1 && k <= kP16W);
  MMB_REQUIRE(npc >= 1 && npc <= k && n_iter >= 0 && k <= d);  // (k <= d: as mmb_pc_solve)
  MMB_REQUIRE(aligned16(ws));
  return launch_solve_mc(g, d, z0, k, npc, n_iter, transposed, pc_out, ws, flag, false, stream);
}

extern "C" int mmb_pc_solve_mc_xt(const double* g, int d, const float* x, int64_t n,
                                  const double* omega, int k, int npc, int n_iter, double* pc_out,
                                  void* ws, int32_t* flag, hipStream_t stream) {
  MMB_REQUIRE(g && x && omega && pc_out && ws && d > 1 && d <= kP16MaxD && k >= 1 && k <= kP16W);
  MMB_REQUIRE(n >= 1 && n < d && n <= kXtMaxN && npc >= 1 && npc <= k && n_iter >= 0 && k <= d);
  MMB_REQUIRE(aligned16(ws));
  const int T = (d + 15) / 16;
  const SolveWs w(ws, d);
  double* g2 = w.g2();
  double* z0 = w.z0();
  const int nsq = solve_squares(npc, n_iter) ? T * (T + 1) / 2 : 0;
  pc_prep_kernel<<<nsq + static_cast<int>(ceil_div(d, 16)), kSqNT, 0, stream>>>(
      g, d, g2, nsq, x, n, omega, k, z0);
  MMB_LAUNCH_CHECK();
  return launch_solve_mc(g, d, z0, k, npc, n_iter, 1, pc_out, ws, flag, true, stream);
}

// float64 X (the numpy drop-in's general rows, not f32-representable): X^T Omega
// read from the f64 rows, no count
extern "C" int mmb_xt_omega_f64(const double* x, int64_t n, int d, const double* omega, int k,
                                double* z0, hipStream_t stream) {
  MMB_REQUIRE(x && omega && z0 && n >= 0 && d > 0 && k > 0);
  if (k <= kXtK && n <= kXtMaxN)
    xt_omega_wave_kernel<double><<<static_cast<int>(ceil_div(d, 16)), 256, 0, stream>>>(x, nullptr, n, d, omega, k, z0);
  else
    xt_omega_kernel<double><<<static_cast<int>(ceil_div(static_cast<int64_t>(d) * k, 256)), 256, 0, stream>>>(
        x, nullptr, n, d, omega, k, z0);
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

// the tools build's variant kernels, launches, knobs and entry points
// (tools/diag/); the product library includes an empty header here
#ifndef MMB_TOOLS_TAIL_PC
#define MMB_TOOLS_TAIL_PC "mmb_no_tools.h"
#endif
#include MMB_TOOLS_TAIL_PC
