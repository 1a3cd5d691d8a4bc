// The Gram matrix G = X^T X of the sentence rows for
// MI355X: the one pass over X of the principal-component removal (a3).
//
// The reference's randomized SVD makes ~15 passes over X
// (sif_functions.py:58-67).  Here X is read ONCE for its [d, d] Gram, the
// only thing that crosses GPUs (RCCL all-reduce, 720 KB at d = 300), and the
// solve runs on G (pc_kernels.hip).  Products of f32 values are exact in f64,
// so the fp64-MFMA kernels round only in the accumulation:
//   gram_small_kernel    n <= 4096, d <= 320: tile-parallel, one launch
//   gram_tri_kernel      d <= 320, d % 4 == 0: row ranges, 16x16 tiles in LDS
//   gram_partial_kernel  any d, f32 or f64 rows: 64x64 blocks per row chunk
//   gram_i8l_kernel      the fused step's rows on the int8 matrix pipe, exact
//                        level sums of base-256 digits (colmax_kernel's bounds)
// each but the first followed by a fixed-order reduction of its partials
// (gram_tri_reduce_kernel, gram_reduce_kernel); the host-side planners and the
// mmb_gram* / mmb_colmax entry points are at the end.
#include <algorithm>
#include <vector>

#include "mmb_pc.h"

namespace mmb {

constexpr int kGB = 64;  // Gram block edge per workgroup (4 waves x 32x32)

__host__ __device__ inline int gram_pair_index(int bp, int bq, int nb) {
  return bp * nb - bp * (bp - 1) / 2 + (bq - bp);
}

// One workgroup: a 64x64 block (bp,bq), bp<=bq, of G over one chunk of rows.
// fp64 MFMA 16x16x4: lane l holds A[l&15][l>>4] and B[l>>4][l&15]; with
// A = X^T and B = X both fragments are 16 consecutive columns of 4 rows of X.
template <typename TX>
__global__ __launch_bounds__(256) void gram_partial_kernel(const TX* __restrict__ num,
                                                           const float* __restrict__ cnt,
                                                           int64_t N, int D, int nb, int npairs,
                                                           int S, int64_t chunk, int xcd_map,
                                                           double* __restrict__ part) {
  int pair, s;
  if (xcd_map) {
    // blocks b and b+8 share an XCD (round-robin dispatch; speed only): give
    // every pair of one row chunk to one XCD so the chunk is fetched once per L2.
    const int b = blockIdx.x, x = b & 7, local = b >> 3;
    s = x + 8 * (local / npairs);
    pair = local % npairs;
  } else {
    pair = blockIdx.x % npairs;
    s = blockIdx.x / npairs;
  }
  int bp = 0, rem = pair;
  while (rem >= nb - bp) {
    rem -= nb - bp;
    ++bp;
  }
  const int bq = bp + rem;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wp = wave >> 1, wq = wave & 1;
  const int ca0 = bp * kGB + wp * 32 + (lane & 15), ca1 = ca0 + 16;
  const int cb0 = bq * kGB + wq * 32 + (lane & 15), cb1 = cb0 + 16;
  const int kr = lane >> 4;
  const int64_t n0 = s * chunk;
  const int64_t n1 = min(N, n0 + chunk);
  f64x4 acc00 = {0, 0, 0, 0}, acc01 = acc00, acc10 = acc00, acc11 = acc00;
#pragma unroll 4
  for (int64_t n = n0; n < n1; n += 4) {
    const int64_t row = n + kr;
    double a0 = 0, a1 = 0, b0 = 0, b1 = 0;
    if (row < n1) {
      a0 = load_x(num, cnt, row, ca0, D);
      a1 = load_x(num, cnt, row, ca1, D);
      b0 = load_x(num, cnt, row, cb0, D);
      b1 = load_x(num, cnt, row, cb1, D);
    }
    acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc00, 0, 0, 0);
    acc01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc01, 0, 0, 0);
    acc10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc10, 0, 0, 0);
    acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc11, 0, 0, 0);
  }
  // f64 C/D layout: col = lane&15, row = (lane>>4) + 4*reg
  double* out = part + (static_cast<int64_t>(s) * npairs + pair) * (kGB * kGB);
  const int c = lane & 15, r0 = lane >> 4;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int i0 = wp * 32 + r0 + 4 * reg, j0 = wq * 32 + c;
    out[i0 * kGB + j0] = acc00[reg];
    out[i0 * kGB + j0 + 16] = acc01[reg];
    out[(i0 + 16) * kGB + j0] = acc10[reg];
    out[(i0 + 16) * kGB + j0 + 16] = acc11[reg];
  }
}

// ------------------------------------------------------------------ Gram v2
// Upper triangle of G in 16x16 tiles (D <= 320: 20 tile rows, 210 tiles).  A
// PAIR of 16-wave workgroups owns one contiguous row range: each stages the
// range's rows once in LDS as f64 (16 rows per chunk, double-buffered, the
// next chunk's global loads in flight during the current chunk's MFMAs) and
// computes half of the tiles (~7 per wave, fp64 MFMA 16x16x4 — one k-step is
// 4 rows).  The pair sits on one XCD (blocks b and b+8) so the second read of
// the rows hits L2.  Per-range partials are summed in a fixed order.
constexpr int kG2NT = 1024;
constexpr int kG2Rows = 16;            // rows per LDS chunk (4 MFMA k-steps)
constexpr int kG2Stride = 336;         // doubles per LDS row: 320 + 16 (rows alternate bank halves)
constexpr int kG2MaxTiles = 8;         // tiles per wave

__device__ __forceinline__ void tri_tile(int tau, int nt, int& ti, int& tj) {
  int r = 0, rem = tau;
  while (rem >= nt - r) {
    rem -= nt - r;
    ++r;
  }
  ti = r;
  tj = r + rem;
}

// ------------------------------------------------------------------ Gram, small n (r05)
// Dataset splits (MOSI 229-1284 rows, POM 100-203) take the exact f64 Gram.
// The row-range kernel below spends its time there on fixed costs: 16 ranges
// of 80 rows, every workgroup writing 95 tiles of partials that a second
// launch reduces (37 us per split, r04 dataset_splits).  For n <= 4096 this
// kernel is tile-parallel instead: one workgroup per 16 x 16 tile of the
// upper triangle over ALL rows, its 16 waves taking strided 4-row k-steps
// (fp64 MFMA 16x16x4: f32 x f32 products exact in f64), the 16 partial tiles
// summed in a fixed order through LDS and written straight into G (and its
// mirror): one launch, no partials.
constexpr int kGsNT = 1024;
constexpr int64_t kGsMaxN = 4096;

template <int G = 8>
__global__ __launch_bounds__(kGsNT) void gram_small_kernel(const float* __restrict__ num,
                                                           const float* __restrict__ cnt,
                                                           int64_t N, int D, int nt, int accumulate,
                                                           double* __restrict__ g) {
  __shared__ double s_acc[kGsNT / kWave][256];
  int bi, bj;
  tri_tile(blockIdx.x, nt, bi, bj);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  constexpr int NW = kGsNT / kWave;
  const int ca = 16 * bi + (lane & 15), cb = 16 * bj + (lane & 15), kr = lane >> 4;
  f64x4 acc = {0, 0, 0, 0};
  // wave w: k-steps w, w + 16, ... (4 rows each), loads issued ahead in
  // groups of G k-steps (one round trip per group)
  const int64_t nks = (N + 3) / 4;
  for (int64_t s0 = wave; s0 < nks; s0 += NW * G) {
    double av[G], bv[G];
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const int64_t row = (s0 + NW * u) * 4 + kr;
      const bool ok = s0 + NW * u < nks && row < N;
      av[u] = ok ? static_cast<double>(load_x(num, cnt, row, ca, D)) : 0.0;
      bv[u] = ok ? static_cast<double>(load_x(num, cnt, row, cb, D)) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < G; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
  }
  // C/D layout: col = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) s_acc[wave][((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = acc[reg];
  __syncthreads();
  if (threadIdx.x >= 256) return;
  const int e = threadIdx.x, r = e >> 4, c = e & 15;
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < NW; ++w) s += s_acc[w][e];
  const int p = 16 * bi + r, q = 16 * bj + c;
  if (p >= D || q >= D) return;
  const int64_t e1 = static_cast<int64_t>(p) * D + q;
  g[e1] = accumulate ? g[e1] + s : s;
  if (bi != bj) {
    const int64_t e2 = static_cast<int64_t>(q) * D + p;
    g[e2] = accumulate ? g[e2] + s : s;
  }
}


__global__ __launch_bounds__(kG2NT) void gram_tri_kernel(const float* __restrict__ num,
                                                         const float* __restrict__ cnt, int64_t N,
                                                         int D, int nt, int R, int64_t chunk,
                                                         int xcd_map, int acc_part,
                                                         double* __restrict__ part) {
  extern __shared__ double s_x[];  // [2][kG2Rows][kG2Stride]
  const int T = nt * (nt + 1) / 2;
  int half, range;
  if (xcd_map) {
    const int b = blockIdx.x;
    half = (b >> 3) & 1;
    range = (b & 7) + 8 * (b >> 4);
  } else {
    half = blockIdx.x & 1;
    range = blockIdx.x >> 1;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t0 = half * ((T + 1) / 2), t1 = half ? T : (T + 1) / 2;
  // this wave's tiles: wave, wave+16, ... within [t0, t1)
  int ti[kG2MaxTiles], tj[kG2MaxTiles];
  int ntl = 0;
#pragma unroll
  for (int q = 0; q < kG2MaxTiles; ++q) {
    const int tau = t0 + wave + (kG2NT / kWave) * q;
    ti[q] = tj[q] = 0;
    if (tau < t1) {
      tri_tile(tau, nt, ti[q], tj[q]);
      ntl = q + 1;
    }
  }
  f64x4 acc[kG2MaxTiles];
#pragma unroll
  for (int q = 0; q < kG2MaxTiles; ++q) acc[q] = f64x4{0, 0, 0, 0};

  const int64_t r0 = range * chunk;
  const int64_t r1 = min(N, r0 + chunk);
  const int nchunks = static_cast<int>(r1 > r0 ? (r1 - r0 + kG2Rows - 1) / kG2Rows : 0);
  const int U = D >> 2;  // float4 units per row (D % 4 == 0)
  // staging map: thread -> (row, float4 unit); 16 rows x 80 units (padded to 320 cols)
  const int srow = tid / 80, sunit = tid % 80;  // tid < 1280 covers 16 x 80; 1024 threads: 2 passes
  auto load_regs = [&](int c, float4 (&v)[2], float (&sc)[2]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int idx = tid + kG2NT * q;
      const int rr = idx / 80, uu = idx % 80;
      const int64_t row = r0 + static_cast<int64_t>(c) * kG2Rows + rr;
      v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      sc[q] = 1.f;
      if (idx < kG2Rows * 80 && row < r1 && uu < U) {
        v[q] = *reinterpret_cast<const float4*>(num + row * D + 4 * uu);
        if (cnt) sc[q] = cnt[row];
      }
    }
  };
  auto store_lds = [&](int buf, const float4 (&v)[2], const float (&sc)[2]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int idx = tid + kG2NT * q;
      if (idx < kG2Rows * 80) {
        const int rr = idx / 80, uu = idx % 80;
        double* dst = s_x + (buf * kG2Rows + rr) * kG2Stride + 4 * uu;
        // x = num / count in f32 (sif_functions.py:55), then exact f64
        // widening; two 16-byte writes (ds_write_b128: the 8 lanes of a
        // write phase hit disjoint banks at this 32-byte lane stride, where
        // four 8-byte writes conflicted 2-way)
        using d2 = double __attribute__((ext_vector_type(2)));
        const d2 lo = {static_cast<double>(cnt ? v[q].x / sc[q] : v[q].x),
                       static_cast<double>(cnt ? v[q].y / sc[q] : v[q].y)};
        const d2 hi = {static_cast<double>(cnt ? v[q].z / sc[q] : v[q].z),
                       static_cast<double>(cnt ? v[q].w / sc[q] : v[q].w)};
        *reinterpret_cast<d2*>(dst) = lo;
        *reinterpret_cast<d2*>(dst + 2) = hi;
      }
    }
  };
  (void)srow;
  (void)sunit;
  float4 pv[2];
  float psc[2];
  if (nchunks > 0) {
    load_regs(0, pv, psc);
    store_lds(0, pv, psc);
  }
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {
    const int buf = c & 1;
    if (c + 1 < nchunks) load_regs(c + 1, pv, psc);
    const double* xb = s_x + buf * kG2Rows * kG2Stride;
#pragma unroll
    for (int s = 0; s < kG2Rows / 4; ++s) {
      const double* xr = xb + (4 * s + (lane >> 4)) * kG2Stride + (lane & 15);
#pragma unroll
      for (int q = 0; q < kG2MaxTiles; ++q) {
        if (q < ntl) {
          const double a = xr[16 * ti[q]];
          const double b = xr[16 * tj[q]];
          acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[q], 0, 0, 0);
        }
      }
    }
    if (c + 1 < nchunks) store_lds(buf ^ 1, pv, psc);
    __syncthreads();
  }
  // partial tiles: part[range][tau][16*16], C/D f64 layout col = lane&15, row = (lane>>4)+4*reg
  double* pr = part + static_cast<int64_t>(range) * T * 256;
#pragma unroll
  for (int q = 0; q < kG2MaxTiles; ++q) {
    if (q < ntl) {
      const int tau = t0 + wave + (kG2NT / kWave) * q;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        // acc_part: add to this range's partial of the previous row chunk (each
        // element has one owner wave: no race; chunks run in stream order)
        double* dst = pr + static_cast<int64_t>(tau) * 256 + ((lane >> 4) + 4 * reg) * 16 + (lane & 15);
        *dst = acc_part ? *dst + acc[q][reg] : acc[q][reg];
      }
    }
  }
}


// ------------------------------------------------------------------ Gram i8
// G = X^T X on the int8 matrix pipe (v_mfma_i32_16x16x64_i8: 64x the fp64
// MFMA rate per operation), for the fused step's x rows.  Each value becomes
// a 30-bit fixed-point integer of its column's power-of-two bound 2^e_j
// (colmax: max |x| of the column):  v = rint(x 2^(30 - e_j)), |v| < 2^30,
// cut into four balanced base-256 digits (the low three sign-extended bytes
// in [-128, 127], the top one in [-64, 64]):  v = sum_a d_a 2^(8 (3 - a)).
// G_ij = 2^(e_i + e_j - 60) sum_rows v_i v_j, keeping the digit pairs of
// level a + b <= 4 (13 of 16; the dropped (2,3), (3,2), (3,3) weigh 2^8 and
// 1 against the top pair's 2^48).  Per 64-row k-step the levels are summed
// EXACTLY in three int32 accumulators, H = acc_0 2^8 + acc_1 (< 2^27),
// M = acc_2 2^8 + acc_3 (< 2^30), L = acc_4, then added in f64 as
// H 2^-20 + M 2^-36 + L 2^-44.  The only roundings are v's (2^-31 of the
// column bound per value) and the f64 accumulation: G within 1e-10 of the
// exact f64 Gram on the golden splits (7e-10 on heavy-tailed t(3) columns),
// the PC within 6e-11 of the reference's (CPU restatement:
// oracle.sif_oracle.sliced_gram; the digit format was chosen by measuring
// it: base-128 digits of 33-bit values needed 22 pairs for the same error,
// because values far below their column's bound live in the low digits).
// Structure as gram_tri_kernel: a pair of workgroups per row range (same
// XCD), each with half of the 16x16 tiles of the upper triangle; per 64-row
// chunk every thread turns its (feature, 16-row) items into digit bytes in
// LDS ([digit][feature][4 slots of 16 rows], the conflict-free slot swizzle
// of the 16x16x32 f16 fragment reads, whose lane map this read shares), then
// each wave runs 13 MFMAs per tile and the f64 update.
constexpr int kGiRows = 64;
constexpr int kGiF = 320;       // padded feature count (D <= 320)
constexpr int kGiDig = 4;       // base-256 digits per value

// 16-byte slot swizzle of a feature's 64-byte digit row: slot kq of feature
// f sits at kq ^ gi_swz(f).  (f >> 1) & 3 keeps the MFMA operand reads
// (ds_read_b128 lane groups: features 16 t + (l & 15) at slot l >> 4)
// conflict-free AND the slicing writes (ds_write_b128 groups of 8 lanes = 8
// consecutive features at one slot) -- the r04 swizzle over f >> 2 left the
// writes 2-way (checked exhaustively, r05).
__host__ __device__ constexpr int gi_swz(int f) { return (f >> 1) & 3; }

using i32x4 = __attribute__((ext_vector_type(4))) int;

__device__ __forceinline__ int gi_exp(unsigned bits) {
  const float m = __uint_as_float(bits);
  if (!(m > 0.f) || !isfinite(m)) return 0;
  int e;
  frexpf(m, &e);  // m = f 2^e, f in [0.5, 1): |x| <= m < 2^e
  return e;
}

// v' = rint(x 2^(30 - e)) + 0x808080: byte i < 3 of v' is d_i + 128 for the
// balanced digit d_i in [-128, 127] (so XOR 0x80 gives d_i's two's-complement
// byte), byte 3 is the top digit d_3 itself (|d_3| <= 64):
//   v = sum_i d_i 256^i  =>  v + 128 (1 + 256 + 65536) = sum_i (d_i + 128) 256^i
// for the low three, the top untouched.
__device__ __forceinline__ unsigned gi_vbias(float x, int e) {
  return static_cast<unsigned>(static_cast<int>(rintf(ldexpf(x, 30 - e)))) + 0x808080u;
}

// 4 values (rows r..r+3) -> the 4 digit-plane dwords, top digit first
// (a 4 x 4 byte transpose in 8 v_perm_b32, then the bias flip)
__device__ __forceinline__ void gi_planes(unsigned v0, unsigned v1, unsigned v2, unsigned v3,
                                          unsigned (&w)[4]) {
  const unsigned p0 = __builtin_amdgcn_perm(v1, v0, 0x05010400u);  // v0.b0 v1.b0 v0.b1 v1.b1
  const unsigned p1 = __builtin_amdgcn_perm(v1, v0, 0x07030602u);  // v0.b2 v1.b2 v0.b3 v1.b3
  const unsigned q0 = __builtin_amdgcn_perm(v3, v2, 0x05010400u);
  const unsigned q1 = __builtin_amdgcn_perm(v3, v2, 0x07030602u);
  w[0] = __builtin_amdgcn_perm(q1, p1, 0x07060302u);                // byte 3: top digit
  w[1] = __builtin_amdgcn_perm(q1, p1, 0x05040100u) ^ 0x80808080u;  // byte 2
  w[2] = __builtin_amdgcn_perm(q0, p0, 0x07060302u) ^ 0x80808080u;  // byte 1
  w[3] = __builtin_amdgcn_perm(q0, p0, 0x05040100u) ^ 0x80808080u;  // byte 0
}

// ------------------------------------------------------------------ Gram i8, range level sums (r05)
// The same digits and the same 13 digit-pair products as gram_i8_kernel, but
// each of the five levels l = a + b is summed in its OWN int32 accumulator
// over the workgroup's whole row range, and the range's f64 partial is formed
// once at the end:  S = (((L0 2^8 + L1) 2^8 + L2) 2^8 + L3) 2^8 + L4 (exact in
// f64 up to the last step, which rounds once), G_part = S 2^(e_i + e_j - 44).
// gram_i8_kernel shifted and combined the levels into three words per 64-row
// k-step and added them to f64 accumulators: per tile and k-step 8 shifts,
// 12 conversions and 12 f64 FMAs beside the 13 MFMAs -- with the digit
// slicing, ~700 vector instructions per wave and chunk against 156 MFMAs, a
// kernel bound by vector issue (0.76 ms at 1M x 300), not by the matrix pipe
// (~0.3 ms of MFMA work).  Here the k-step loop issues the MFMAs, their
// operand reads and the slicing only.
// Exactness: per 64-row k-step |L0| <= 64 * 64 * 64 = 2^18, |L1| <= 2^20,
// |L2| <= 2^21, |L3|, |L4| <= 2^21.6, so int32 level sums are exact for 512
// k-steps: a range holds at most kGlMaxRows = 32768 rows (gram_i8l_plan).
// Registers: 5 levels x 4 words per 16x16 tile, so a workgroup holds fewer
// tiles than gram_i8_kernel's pairs: THREE workgroups per row range (on one
// XCD: the range's x is read from HBM once), each a contiguous run of the
// row-major triangle (<= 64 tiles, <= 8 per wave), split on the host so that
// the vector work -- a part slices only the features its tiles touch, from
// its first tile row on -- and the MFMA work balance (gram_i8l_split).
constexpr int kGlLev = 5;
constexpr int64_t kGlMaxRows = 512 * kGiRows;        // int32 level sums exact
constexpr int kGlMaxParts = 4;
constexpr int kGlMaxPartTiles = 64;

// One workgroup's share of a range's work: its tiles (ti | tj << 8, grouped
// by tile row for A reuse) and the features it slices, [f0, f0 + n0) and
// [f1, f1 + n1) -- every feature its tiles touch (gram_i8l_parts).
struct GlPart {
  int n, f0, n0, f1, n1;
  uint16_t tile[kGlMaxPartTiles];
};
struct GlParts {
  GlPart p[kGlMaxParts];
};

// Shape of a level-sum kernel: P workgroups per row range, NW waves each, at
// most MT tiles per wave (P * NW * MT >= 190 tiles at d = 300); IT slicing
// items (16 rows of one feature) per thread.
// SB: the mask of the scheduling barrier between tiles (0: nothing crosses;
// 0x100: LDS reads may move up into the previous tile); PF: the next tile's
// first B digit is read during the current tile's MFMAs (4 VGPRs).
// ST: staggered slicing -- waves 0 .. NW/2-1 slice each item BEFORE their
// run of tiles, waves NW/2 .. NW-1 (their SIMD partners) AFTER it, so one
// wave of a SIMD slices while the other issues MFMAs; each item's x for the
// chunk after next is loaded as soon as it is sliced.
template <int P, int NW, int MT, int IT, int SB = 0, bool PF = false, bool ST = false>
struct GlShape {
  static constexpr int kP = P, kNW = NW, kMT = MT, kNT = NW * kWave, kSB = SB;
  static constexpr bool kPF = PF, kST = ST;
  // staggered: the slice point of item u (before tile p; p = MT: after the last)
  static constexpr int slice_before(int u, bool second) { return ((u + (second ? 1 : 0)) * MT) / IT; }
  static constexpr int kPartMax = NW * MT < kGlMaxPartTiles ? NW * MT : kGlMaxPartTiles;
  static constexpr int kIt = IT;
  // item u is sliced after tile slice_at(u): spread over the tile loop
  static constexpr int slice_at(int u) { return (u * MT) / kIt + MT / kIt - 1; }
};

// DIAG (timing-only builds, wrong results; MMB_GRAM_DIAG with the level-sum
// kernel): bit 0 no MFMAs (operands kept live), bit 2 no slicing, bit 3 no x loads
template <int DIAG, class S>
__global__ __launch_bounds__(S::kNT) void gram_i8l_kernel(const float* __restrict__ x,
                                                         const unsigned* __restrict__ colmax,
                                                         int64_t N, int D, int nt, int64_t chunk,
                                                         int xcd_map, GlParts parts,
                                                         double* __restrict__ part) {
  constexpr int MT = S::kMT, NT = S::kNT, kIt = S::kIt;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dig[];  // [2][4][kGiF][64]
  int range, p;
  if (xcd_map) {  // the P parts of a range on one XCD (round-robin dispatch: b % 8)
    const int b = blockIdx.x, s = b >> 3;
    range = (b & 7) + 8 * (s / S::kP);
    p = s % S::kP;
  } else {
    range = blockIdx.x / S::kP;
    p = blockIdx.x % S::kP;
  }
  const GlPart& pt = parts.p[p];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int npt = pt.n;
  if (npt <= 0) return;  // an empty part (tiny d)
  const int per = (npt + S::kNW - 1) / S::kNW;
  const int q0 = wave * per;
  int ti[MT], tj[MT];
  int ntl = 0;
#pragma unroll
  for (int q = 0; q < MT; ++q) {
    ti[q] = tj[q] = 0;
    if (q < per && q0 + q < npt) {
      const int t = pt.tile[q0 + q];
      ti[q] = t & 255;
      tj[q] = t >> 8;
      ntl = q + 1;
    }
  }
  i32x4 lev[MT][kGlLev];
#pragma unroll
  for (int q = 0; q < MT; ++q)
#pragma unroll
    for (int l = 0; l < kGlLev; ++l) lev[q][l] = i32x4{0, 0, 0, 0};

  const int64_t r0 = range * chunk;
  const int64_t r1 = min(N, r0 + chunk);
  const int nchunks = static_cast<int>(r1 > r0 ? (r1 - r0 + kGiRows - 1) / kGiRows : 0);
  // the features this part slices: two ranges (every feature its tiles touch)
  const int f0 = pt.f0, n0 = pt.n0, f1 = pt.f1;
  const int nf = n0 + pt.n1;
  const int nitems = nf * 4;
  // item it = k + nf * kq: the k-th sliced feature f, rows 16 kq .. 16 kq + 15
  // of the chunk; packed (f | kq << 9 | (e + 256) << 11) with its row offset
  int it_pk[kIt], it_off[kIt];
#pragma unroll
  for (int u = 0; u < kIt; ++u) {
    const int it = tid + NT * u;
    const int k = it < nitems ? it % nf : 0;
    const int f = it < nitems ? (k < n0 ? f0 + k : f1 + k - n0) : 0;
    const int kq = it < nitems ? it / nf : 0;
    const int e = (it < nitems && f < D) ? gi_exp(colmax[f]) : 0;
    it_pk[u] = f | (kq << 9) | ((e + 256) << 11);
    // padding features / missing items read past the record count: 0
    it_off[u] = (it < nitems && f < D) ? (kq * 16 * D + f) * 4 : 0x7ffffff0;
  }
  const int nrec = __builtin_amdgcn_readfirstlane(static_cast<int>((r1 > r0 ? r1 - r0 : 0) * D * 4));
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x + r0 * D), 0, nrec, 0x00020000);
  float xv[kIt][16];
  auto load = [&](int c) {
    if constexpr ((DIAG & 8) != 0) {
#pragma unroll
      for (int u = 0; u < kIt; ++u)
#pragma unroll
        for (int j = 0; j < 16; ++j) asm volatile("" : "+v"(xv[u][j]));
      return;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int so = __builtin_amdgcn_readfirstlane((c * kGiRows + j) * D * 4);
#pragma unroll
      for (int u = 0; u < kIt; ++u)
        xv[u][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, it_off[u], so, 0));
    }
  };
  auto load_item = [&](int u, int c) {
    if constexpr ((DIAG & 8) != 0) {
#pragma unroll
      for (int j = 0; j < 16; ++j) asm volatile("" : "+v"(xv[u][j]));
      return;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int so = __builtin_amdgcn_readfirstlane((c * kGiRows + j) * D * 4);
      xv[u][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, it_off[u], so, 0));
    }
  };
  auto slice_item = [&](int u, unsigned char* buf) {
    if constexpr ((DIAG & 4) != 0) return;
    const int it = tid + NT * u;
    if (it < nitems) {
      const int f = it_pk[u] & 511, kq = (it_pk[u] >> 9) & 3, e = (it_pk[u] >> 11) - 256;
      unsigned w[4][kGiDig];
#pragma unroll
      for (int g = 0; g < 4; ++g)
        gi_planes(gi_vbias(xv[u][4 * g + 0], e), gi_vbias(xv[u][4 * g + 1], e),
                  gi_vbias(xv[u][4 * g + 2], e), gi_vbias(xv[u][4 * g + 3], e), w[g]);
      const int slot = kq ^ gi_swz(f);
#pragma unroll
      for (int a = 0; a < kGiDig; ++a)
        *reinterpret_cast<uint4*>(buf + ((a * kGiF + f) * 4 + slot) * 16) =
            make_uint4(w[0][a], w[1][a], w[2][a], w[3][a]);
    }
  };
  constexpr int kBuf = kGiDig * kGiF * kGiRows;

  // double-buffered digits, one barrier per 64-row chunk (as gram_i8_kernel)
  if (nchunks > 0) {
    load(0);
#pragma unroll
    for (int u = 0; u < kIt; ++u) slice_item(u, s_dig);
    if (nchunks > 1) load(1);
  }
  __syncthreads();
  const int lf = lane & 15, lsl = lane >> 4;
  for (int c = 0; c < nchunks; ++c) {
    const unsigned char* cur = s_dig + (c & 1) * kBuf;
    unsigned char* nxt = s_dig + ((c + 1) & 1) * kBuf;
    const bool more = c + 1 < nchunks;
    i32x4 A[kGiDig];
    auto ld_b = [&](const unsigned char* buf, int fb, int b) {
      return *reinterpret_cast<const i32x4*>(buf + ((b * kGiF + fb) * 4 + (lsl ^ gi_swz(fb))) * 16);
    };
    i32x4 Bn0 = {0, 0, 0, 0};
    if constexpr (S::kPF) {
      if (ntl > 0) Bn0 = ld_b(cur, tj[0] * 16 + lf, 0);
    }
    const bool second = wave >= S::kNW / 2;
    // staggered slicing: the items whose slice point is before tile p
    auto slice_point = [&](int p) {
      if constexpr (S::kST) {
#pragma unroll
        for (int u = 0; u < kIt; ++u) {
          if (S::slice_before(u, second) == p && more) {
            slice_item(u, nxt);
            if (c + 2 < nchunks) load_item(u, c + 2);
          }
        }
      }
    };
#pragma unroll
    for (int q = 0; q < MT; ++q) {
      slice_point(q);
      if (q < ntl) {
        if (q == 0 || ti[q] != ti[q - 1]) {  // the row block changes (wave-uniform)
          const int fa = ti[q] * 16 + lf;
#pragma unroll
          for (int a = 0; a < kGiDig; ++a)
            A[a] = *reinterpret_cast<const i32x4*>(cur + ((a * kGiF + fa) * 4 + (lsl ^ gi_swz(fa))) * 16);
        }
        const int fb = tj[q] * 16 + lf;
        i32x4 Bd[kGiDig];
#pragma unroll
        for (int b = 0; b < kGiDig; ++b)
          Bd[b] = (S::kPF && b == 0) ? Bn0 : ld_b(cur, fb, b);
        if constexpr (S::kPF) {
          if (q + 1 < ntl) Bn0 = ld_b(cur, tj[q + 1] * 16 + lf, 0);
        }
        // B digit by digit: digit b meets A digits a <= 4 - b (levels a + b <= 4)
#pragma unroll
        for (int b = 0; b < kGiDig; ++b) {
          const i32x4 B = Bd[b];
          if constexpr ((DIAG & 1) != 0) {
            asm volatile("" ::"v"(B));
          } else {
#pragma unroll
            for (int a = 0; a < kGiDig; ++a)
              if (a + b < kGlLev)
                lev[q][a + b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[a], B, lev[q][a + b], 0, 0, 0);
          }
        }
        if constexpr ((DIAG & 1) != 0) {
#pragma unroll
          for (int a = 0; a < kGiDig; ++a) asm volatile("" ::"v"(A[a]));
        }
      }
      // the next chunk's slicing spread between the tiles: VALU work beside
      // the MFMAs in flight
      if constexpr (!S::kST) {
#pragma unroll
        for (int u = 0; u < kIt; ++u)
          if (S::slice_at(u) == q && more) slice_item(u, nxt);
      }
      __builtin_amdgcn_sched_barrier(S::kSB);
    }
    slice_point(MT);
    if (!S::kST && c + 2 < nchunks) load(c + 2);
    __syncthreads();
  }
  // the range's partials: S exact to the last step, one rounding, then the
  // exact power-of-two scale; a non-finite bound gives NaN rows / columns
  const int T = nt * (nt + 1) / 2;
  double* pr = part + static_cast<int64_t>(range) * T * 256;
  const int lc = lane & 15, lr = 4 * (lane >> 4);
#pragma unroll
  for (int q = 0; q < MT; ++q) {
    if (q < ntl) {
      const int tau = ti[q] * nt - ti[q] * (ti[q] - 1) / 2 + (tj[q] - ti[q]);  // row-major triangle
      const int fj = tj[q] * 16 + lc;
      const int ej = fj < D ? gi_exp(colmax[fj]) : 0;
      const bool okj = fj >= D || isfinite(__uint_as_float(colmax[fj]));
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int fi = ti[q] * 16 + lr + e;
        const int ei = fi < D ? gi_exp(colmax[fi]) : 0;
        const bool bad = (fi < D && !isfinite(__uint_as_float(colmax[fi]))) || !okj;
        double sum = static_cast<double>(lev[q][0][e]);
#pragma unroll
        for (int l = 1; l < kGlLev; ++l) sum = fma(sum, 256.0, static_cast<double>(lev[q][l][e]));
        pr[static_cast<int64_t>(tau) * 256 + (lr + e) * 16 + lc] =
            bad ? __builtin_nan("") : ldexp(sum, ei + ej - 44);
      }
    }
  }
}

// product shape: three workgroups per range (80 ranges), 8 waves, <= 8 tiles
// per wave, each slicing two of three feature groups (<= 2 items per
// thread), staggered slicing between SIMD partners (r05, tools/gram_ab.py at
// 1M x 300: 0.62-0.63 ms vs 0.65-0.66 unstaggered, 0.77-0.80 for r04's
// kernel; 125k: 0.095 vs 0.099 / 0.122)
using GlProduct = GlShape<3, 8, 8, 2, 0, false, true>;

// colmax[j] = max_i |x[i, j]| as float bits (atomicMax on the bits of a
// non-negative float orders like the float); a NaN bound wins (non-finite x
// then reaches G through mmb_gram_i8).
__global__ void colmax_kernel(const float* __restrict__ x, int64_t N, int D, int64_t rows_per_block,
                              unsigned* __restrict__ colmax) {
  const int64_t r0 = blockIdx.x * rows_per_block;
  const int64_t r1 = min(N, r0 + rows_per_block);
  for (int j = threadIdx.x; j < D; j += blockDim.x) {
    unsigned m = 0u;  // bits of max |x|: NaN (0x7fc00000..) ranks above inf, so it propagates
    for (int64_t r = r0; r < r1; ++r) m = max(m, __float_as_uint(fabsf(x[r * D + j])));
    if (m > 0u) atomicMax(colmax + j, m);
  }
}

// Fixed-order sum of the R range partials of every upper-triangle tile
// element (consecutive threads read consecutive partial elements: coalesced;
// the former element-of-G order read the lower half transposed, 8x the bytes),
// written to G[p][q] and mirrored to G[q][p] for off-diagonal tiles (diagonal
// tiles hold both halves themselves).  Same sums in the same order as before.
// r03: 8 threads per element (thread group u sums the ranges r = u (mod 8) in
// increasing r, all of its <= 16 loads in flight at once; the 8 sums are
// combined in LDS) -- the same eight partial sums and the same combine order
// as the one-thread-per-element kernel, so G is bit-identical, but 8x the
// loads in flight: the reduction of 128 ranges (49.8 MB of partials at
// D = 300) was latency-bound at ~57 us.
constexpr int kRedEl = 32;      // elements per block
constexpr int kRedMaxPer = 16;  // ranges per thread (R <= 128)
__global__ __launch_bounds__(256) void gram_tri_reduce_kernel(const double* __restrict__ part, int D,
                                                              int nt, int R, int accumulate,
                                                              double* __restrict__ g) {
  __shared__ double s_p[8][kRedEl];
  const int T = nt * (nt + 1) / 2;
  const int64_t total = static_cast<int64_t>(T) * 256;
  const int el = threadIdx.x % kRedEl, u = threadIdx.x / kRedEl;
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kRedEl + el;
  double s = 0.0;
  if (e < total) {
    if (R >= 8) {  // thread group u sums ranges u, u + 8, .. (< R)
      double v[kRedMaxPer];
      const int per = (R + 7) / 8;
#pragma unroll
      for (int j = 0; j < kRedMaxPer; ++j)
        v[j] = (j < per && u + 8 * j < R) ? part[static_cast<int64_t>(u + 8 * j) * total + e] : 0.0;
#pragma unroll
      for (int j = 0; j < kRedMaxPer; ++j)
        if (j < per && u + 8 * j < R) s += v[j];
    } else if (u == 0) {
      for (int r = 0; r < R; ++r) s += part[static_cast<int64_t>(r) * total + e];
    }
  }
  s_p[u][el] = s;
  __syncthreads();
  if (u != 0 || e >= total) return;
  const int tau = static_cast<int>(e >> 8), w = static_cast<int>(e & 255);
  int bi, bj;
  tri_tile(tau, nt, bi, bj);
  const int p = 16 * bi + (w >> 4), q = 16 * bj + (w & 15);
  if (p >= D || q >= D) return;
  const double sum = ((s_p[0][el] + s_p[1][el]) + (s_p[2][el] + s_p[3][el])) +
                     ((s_p[4][el] + s_p[5][el]) + (s_p[6][el] + s_p[7][el]));
  const int64_t e1 = static_cast<int64_t>(p) * D + q;
  g[e1] = accumulate ? g[e1] + sum : sum;
  if (bi != bj) {
    const int64_t e2 = static_cast<int64_t>(q) * D + p;
    g[e2] = accumulate ? g[e2] + sum : sum;
  }
}

static int launch_tri_reduce(const double* part, int d, int nt, int R, int accumulate, double* g,
                             hipStream_t stream) {
  // the kernel sums ranges u + 8 j < R (at most kRedMaxPer per thread) for
  // R >= 8: a plan outside that would silently drop ranges
  MMB_REQUIRE(R >= 1 && R <= 8 * kRedMaxPer);
  const int64_t total = static_cast<int64_t>(nt) * (nt + 1) / 2 * 256;
  gram_tri_reduce_kernel<<<static_cast<int>(ceil_div(total, kRedEl)), 256, 0, stream>>>(
      part, d, nt, R, accumulate, g);
  return MMB_OK;
}

// Fixed-order sum over the S row chunks (deterministic), mirrored to both halves.
__global__ void gram_reduce_kernel(const double* __restrict__ part, int D, int nb, int npairs,
                                   int S, int accumulate, double* __restrict__ g) {
  const int64_t total = static_cast<int64_t>(D) * D;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int p = static_cast<int>(e / D), q = static_cast<int>(e % D);
    int bp = p / kGB, bq = q / kGB, i = p % kGB, j = q % kGB;
    if (bp > bq) {
      int t = bp; bp = bq; bq = t;
      t = i; i = j; j = t;
    }
    const int pair = gram_pair_index(bp, bq, nb);
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += part[(static_cast<int64_t>(s) * npairs + pair) * (kGB * kGB) + i * kGB + j];
    g[e] = accumulate ? g[e] + sum : sum;
  }
}

struct GramPlan {
  int nb, npairs, S, xcd;
  int64_t chunk;
};

static GramPlan gram_plan(int64_t n, int d) {
  GramPlan p;
  p.nb = static_cast<int>(ceil_div(d, kGB));
  p.npairs = p.nb * (p.nb + 1) / 2;
  int64_t S = n / 4096;
  if (S < 1) S = 1;
  if (S > 128) S = 128;
  if (S >= 8) S = S / 8 * 8;
  p.S = static_cast<int>(S);
  p.xcd = (p.S % 8 == 0) ? 1 : 0;
  p.chunk = ceil_div(ceil_div(n, p.S), 4) * 4;
  return p;
}

// The generic route (any d; f32 rows with their counts, or f64 rows): the
// 64x64-block partials, then their fixed-order sum into g.
template <typename TX>
static int launch_gram_generic(const TX* x, const float* cnt, int64_t n, int d, double* g,
                               int accumulate, double* part, hipStream_t stream) {
  const GramPlan p = gram_plan(n, d);
  gram_partial_kernel<TX><<<p.npairs * p.S, 256, 0, stream>>>(x, cnt, n, d, p.nb, p.npairs, p.S, p.chunk,
                                                              p.xcd, part);
  MMB_LAUNCH_CHECK();
  const int64_t total = static_cast<int64_t>(d) * d;
  gram_reduce_kernel<<<static_cast<int>(ceil_div(total, 256)), 256, 0, stream>>>(part, d, p.nb, p.npairs,
                                                                                 p.S, accumulate, g);
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

struct Gram2Plan {
  int nt, T, R, xcd;
  int64_t chunk;
};

// at most 128 row ranges = 256 workgroups, one per CU (measured on MI355X at
// 1M rows: 1.87 ms with 128, 1.95 with 256, 2.08 with 512, partial reduction
// included); fewer ranges also halve the partials the reduction reads
constexpr int kG2MaxR = 128;

static Gram2Plan gram2_plan(int64_t n, int d) {
  Gram2Plan p;
  p.nt = static_cast<int>(ceil_div(d, 16));
  p.T = p.nt * (p.nt + 1) / 2;
  // ranges of >= 512 rows -- but at least 16 ranges (32 workgroups) once
  // there are 64 rows per range: a dataset split (1284 rows) ran on 4
  // workgroups (0.15 ms)
  int64_t R = n / 512;
  if (R < 16) R = std::min<int64_t>(16, n / 64);
  if (R < 1) R = 1;
  if (R > kG2MaxR) R = kG2MaxR;
  if (R >= 8) R = R / 8 * 8;
  p.R = static_cast<int>(R);
  p.xcd = (p.R % 8 == 0) ? 1 : 0;
  p.chunk = ceil_div(n, p.R);
  return p;
}

// int8 Gram: ranges of >= 64 rows (one k-step) instead of gram2_plan's
// >= 512, so a 10k-row split (POM) fills every CU instead of 32 of them
static Gram2Plan gram_i8_plan(int64_t n, int d) {
  Gram2Plan q = gram2_plan(n, d);
  int64_t R = n / kGiRows;
  if (R < 1) R = 1;
  if (R > kG2MaxR) R = kG2MaxR;
  if (R >= 8) R = R / 8 * 8;
  q.R = static_cast<int>(R);
  q.xcd = (q.R % 8 == 0) ? 1 : 0;
  q.chunk = ceil_div(ceil_div(n, q.R), kGiRows) * kGiRows;
  return q;
}

static size_t gram2_lds() {
  const size_t lds = sizeof(double) * 2 * kG2Rows * kG2Stride;
  allow_dynamic_lds<&gram_tri_kernel>(lds);
  return lds;
}

static bool gram2_ok(const float* num, int d) {
  // 16-wave tile kernel: d <= 320 (20 tile rows, <= 8 tiles per wave per half)
  return d % 4 == 0 && d <= 320 && aligned16(num);
}



// ---- level-sum int8 Gram (gram_i8l_kernel): plan and parts
struct GramLPlan {
  int nt, T, R, xcd, P;
  GlParts parts;
  int64_t chunk;
};

static int tri_row_host(int tau, int nt) {
  int r = 0, rem = tau;
  while (rem >= nt - r) {
    rem -= nt - r;
    ++r;
  }
  return r;
}

static void gl_set_features(GlPart& g, int f0, int n0, int f1, int n1) {
  g.f0 = f0;
  g.n0 = n0;
  g.f1 = f1;
  g.n1 = n1;
}

// Three feature groups G0 | G1 | G2 of tile rows (nt split as evenly as it
// goes, the larger groups last) and three parts, one per pair of groups:
// {G0, G1}, {G0, G2}, {G1, G2}.  Each off-diagonal block Gi x Gj goes to part
// {Gi, Gj}; each diagonal block Gg x Gg is cut between the two parts holding
// Gg (row-major: the first x_g tiles to the first of them), the three cuts
// chosen to minimise the largest part (exhaustively: <= 29^3 cases, once per
// nt).  So every part slices two thirds of the features (the three together
// twice x, like a pair of workgroups) while holding a third of the tiles --
// where contiguous runs of the triangle made the first part slice every
// feature.
static GlParts gl_parts_groups3(int nt) {
  GlParts g{};
  const int c = nt / 3 + (nt % 3 > 1 ? 1 : 0), b = nt / 3 + (nt % 3 > 0 ? 1 : 0), a = nt - b - c;
  const int lo[3] = {0, a, a + b}, hi[3] = {a, a + b, nt};
  const int pg[3][2] = {{0, 1}, {0, 2}, {1, 2}};  // part -> its two groups
  const int dpart[3][2] = {{0, 1}, {0, 2}, {1, 2}};  // group -> the two parts holding it
  auto sz = [&](int k) { return hi[k] - lo[k]; };
  const int off[3] = {sz(0) * sz(1), sz(0) * sz(2), sz(1) * sz(2)};  // blocks 01, 02, 12
  int dg[3];
  for (int k = 0; k < 3; ++k) dg[k] = sz(k) * (sz(k) + 1) / 2;
  int bx[3] = {dg[0], dg[1], dg[2]}, best = 1 << 30;
  for (int x0 = 0; x0 <= dg[0]; ++x0)
    for (int x1 = 0; x1 <= dg[1]; ++x1)
      for (int x2 = 0; x2 <= dg[2]; ++x2) {
        int load[3] = {off[0], off[1], off[2]};
        const int xs[3] = {x0, x1, x2};
        for (int k = 0; k < 3; ++k) {
          load[dpart[k][0]] += xs[k];
          load[dpart[k][1]] += dg[k] - xs[k];
        }
        const int m = std::max(load[0], std::max(load[1], load[2]));
        if (m < best) {
          best = m;
          bx[0] = x0;
          bx[1] = x1;
          bx[2] = x2;
        }
      }
  auto group_of = [&](int r) { return r < hi[0] ? 0 : (r < hi[1] ? 1 : 2); };
  std::vector<std::pair<int, int>> lists[3];
  int seen[3] = {0, 0, 0};  // diagonal tiles handed out per group
  for (int ti = 0; ti < nt; ++ti) {
    for (int tj = ti; tj < nt; ++tj) {
      const int gi = group_of(ti), gj = group_of(tj);
      int q;
      if (gi != gj) {
        q = gi == 0 ? (gj == 1 ? 0 : 1) : 2;
      } else {
        q = seen[gi] < bx[gi] ? dpart[gi][0] : dpart[gi][1];
        ++seen[gi];
      }
      lists[q].push_back({ti, tj});
    }
  }
  for (int k = 0; k < 3; ++k) {
    std::sort(lists[k].begin(), lists[k].end());
    g.p[k].n = static_cast<int>(lists[k].size());
    for (int i = 0; i < g.p[k].n && i < kGlMaxPartTiles; ++i)
      g.p[k].tile[i] = static_cast<uint16_t>(lists[k][i].first | (lists[k][i].second << 8));
    const int g0 = pg[k][0], g1 = pg[k][1];
    gl_set_features(g.p[k], 16 * lo[g0], 16 * sz(g0), 16 * lo[g1], 16 * sz(g1));
  }
  return g;
}

// P contiguous runs of the row-major triangle, <= cap tiles each, minimising
// the largest part's modelled cost per 64-row chunk in SIMD cycles: the
// matrix pipe (13 MFMAs x 16 cycles per tile over 4 SIMDs) against vector
// issue (the MFMAs' 8 cycles each plus the slicing of every feature from the
// part's first tile row on: 64 values x ~6.75 vector instructions of 4
// cycles over 64 lanes and 4 SIMDs).  Dynamic program over the split points.
static GlParts gl_parts_runs(int nt, int P, int cap) {
  const int T = nt * (nt + 1) / 2;
  auto cost = [&](int t0, int t1) {
    const int n = t1 - t0;
    if (n <= 0) return 0.0;
    const int nf = 16 * (nt - tri_row_host(t0, nt));
    return std::max(52.0 * n, 26.0 * n + 6.75 * nf);
  };
  std::vector<std::vector<double>> best(P + 1, std::vector<double>(T + 1, 1e300));
  std::vector<std::vector<int>> arg(P + 1, std::vector<int>(T + 1, 0));
  best[0][0] = 0.0;
  for (int k = 1; k <= P; ++k)
    for (int t = 0; t <= T; ++t)
      for (int s = std::max(0, t - cap); s <= t; ++s) {
        const double c = std::max(best[k - 1][s], cost(s, t));
        if (c < best[k][t]) {
          best[k][t] = c;
          arg[k][t] = s;
        }
      }
  int bnd[kGlMaxParts + 1];
  bnd[P] = T;
  for (int k = P; k >= 1; --k) bnd[k - 1] = arg[k][bnd[k]];
  GlParts g{};
  for (int k = 0; k < P; ++k) {
    g.p[k].n = bnd[k + 1] - bnd[k];
    int r0 = nt;
    for (int t = bnd[k]; t < bnd[k + 1] && t - bnd[k] < kGlMaxPartTiles; ++t) {
      const int ti = tri_row_host(t, nt);
      int rem = t;
      for (int r = 0; r < ti; ++r) rem -= nt - r;
      g.p[k].tile[t - bnd[k]] = static_cast<uint16_t>(ti | ((ti + rem) << 8));
      r0 = std::min(r0, ti);
    }
    gl_set_features(g.p[k], 16 * r0, 16 * (nt - r0), 0, 0);
  }
  return g;
}

// R ranges of whole 64-row chunks: as many as keep all P R workgroups
// resident (P = 3: 80 ranges, 240 workgroups -- ten ranges' parts on each
// XCD's 32 CUs), at least one k-step each and at most kGlMaxRows rows each
// (the int32 level sums); a multiple of 8 (the XCD map and
// gram_tri_reduce_kernel) and <= 128 -- mmb_gram_i8 cuts larger calls into
// blocks of kGlBlockRows rows.  The parts depend on nt and the shape only:
// built once per (shape, nt) and cached (the dynamic program costs ~0.1 ms
// of host time, more than a small split's whole Gram).
constexpr int64_t kGlBlockRows = 128 * kGlMaxRows;

static int gram_i8l_ranges(int64_t n, int P) {
  const int64_t resident = 256 / P / 8 * 8;
  int64_t R = std::min<int64_t>(resident, std::max<int64_t>(1, n / kGiRows));
  R = std::max<int64_t>(R, ceil_div(n, kGlMaxRows));
  if (R >= 8) R = ceil_div(R, 8) * 8;
  return static_cast<int>(std::min<int64_t>(R, 128));
}

template <class S, bool GROUPS>
static GramLPlan gram_i8l_plan(int64_t n, int d) {
  GramLPlan q;
  q.nt = static_cast<int>(ceil_div(d, 16));
  q.T = q.nt * (q.nt + 1) / 2;
  q.P = S::kP;
  q.R = gram_i8l_ranges(n, S::kP);
#ifdef MMB_HOOK_GRAM_RANGES  // (tools/diag: MMB_GRAM_RANGES, A/B runs of the range count)
  MMB_HOOK_GRAM_RANGES(q.R);
#endif
  q.xcd = (q.R % 8 == 0) ? 1 : 0;
  q.chunk = ceil_div(ceil_div(std::max<int64_t>(n, 1), q.R), kGiRows) * kGiRows;
  static GlParts cache[kGiF / 16 + 1];
  static bool have[kGiF / 16 + 1] = {};
  if (!have[q.nt]) {
    cache[q.nt] = GROUPS ? gl_parts_groups3(q.nt) : gl_parts_runs(q.nt, S::kP, S::kPartMax);
    have[q.nt] = true;
  }
  q.parts = cache[q.nt];
  return q;
}

template <int DIAG, class S>
static size_t gram_i8l_lds() {
  const size_t lds = 2 * kGiDig * kGiF * kGiRows;  // 160 KB: double-buffered digits
  allow_dynamic_lds<&gram_i8l_kernel<DIAG, S>>(lds);
  return lds;
}

// One block of <= kGlBlockRows rows: the level-sum kernel, then the range
// reduction (writing or accumulating into g).
template <int DIAG, class S, bool GROUPS>
static int gram_i8l_block(const float* x, const uint32_t* colmax, int64_t n, int d, double* g,
                          int accumulate, double* part, hipStream_t stream) {
  const GramLPlan q = gram_i8l_plan<S, GROUPS>(n, d);
  int tiles = 0;
  for (int k = 0; k < q.P; ++k) {  // every tile once, within the shape's tiles and items
    MMB_REQUIRE(q.parts.p[k].n <= S::kPartMax);
    MMB_REQUIRE((q.parts.p[k].n0 + q.parts.p[k].n1) * 4 <= S::kIt * S::kNT);
    tiles += q.parts.p[k].n;
  }
  MMB_REQUIRE(tiles == q.T);
  // the buffer-descriptor record count and row offsets are 32-bit byte counts of one range
  MMB_REQUIRE(q.chunk * d * 4 < (int64_t{1} << 31));
  gram_i8l_kernel<DIAG, S><<<S::kP * q.R, S::kNT, gram_i8l_lds<DIAG, S>(), stream>>>(
      x, colmax, n, d, q.nt, q.chunk, q.xcd, q.parts, part);
  MMB_LAUNCH_CHECK();
  const int rc = launch_tri_reduce(part, d, q.nt, q.R, accumulate, g, stream);
  if (rc != MMB_OK) return rc;
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}


}  // namespace mmb

using namespace mmb;

extern "C" size_t mmb_gram_workspace_bytes(int64_t n, int d) {
  const GramPlan p = gram_plan(n, d);
  const size_t v1 = static_cast<size_t>(p.S) * p.npairs * kGB * kGB * sizeof(double);
  const Gram2Plan q = gram2_plan(n, d);
  const size_t v2 = static_cast<size_t>(q.R) * q.T * 256 * sizeof(double);
  const Gram2Plan qi = gram_i8_plan(n, d);
  const size_t v3 = static_cast<size_t>(qi.R) * qi.T * 256 * sizeof(double);
  // the level-sum kernel: at most 128 ranges per block (every shape)
  const int64_t ntl = ceil_div(d, 16);
  const size_t v4 = static_cast<size_t>(gram_i8l_ranges(std::min(n, kGlBlockRows), 2)) *
                    (ntl * (ntl + 1) / 2) * 256 * sizeof(double);  // every shape's ranges bound
  const size_t v23 = std::max(std::max(v2, v3), v4);
  return v1 > v23 ? v1 : v23;
}

extern "C" int mmb_gram(const float* num, const float* cnt, int64_t n, int d, double* g,
                        int accumulate, void* ws, hipStream_t stream) {
  MMB_REQUIRE(num && g && ws && n >= 0 && d > 0);
  double* part = static_cast<double*>(ws);
  if (n <= kGsMaxN && d <= 320) {  // small splits: tile-parallel, one launch, no partials
    const int nt = static_cast<int>(ceil_div(d, 16));
    // 12 k-steps a group from 512 rows on (24 and 16 spill at 1024
    // threads): MOSI's train split (1284 rows) in two round trips of loads
    // instead of three
    if (n > 512)
      gram_small_kernel<12><<<nt * (nt + 1) / 2, kGsNT, 0, stream>>>(num, cnt, n, d, nt, accumulate, g);
    else
      gram_small_kernel<8><<<nt * (nt + 1) / 2, kGsNT, 0, stream>>>(num, cnt, n, d, nt, accumulate, g);
    MMB_LAUNCH_CHECK();
    return MMB_OK;
  }
  if (gram2_ok(num, d)) {
    const Gram2Plan q = gram2_plan(n, d);
    const size_t lds = gram2_lds();
    gram_tri_kernel<<<2 * q.R, kG2NT, lds, stream>>>(num, cnt, n, d, q.nt, q.R, q.chunk, q.xcd, 0, part);
    MMB_LAUNCH_CHECK();
    {
      const int rc = launch_tri_reduce(part, d, q.nt, q.R, accumulate, g, stream);
      if (rc != MMB_OK) return rc;
    }
    MMB_LAUNCH_CHECK();
    return MMB_OK;
  }
  return launch_gram_generic(num, cnt, n, d, g, accumulate, part, stream);
}


extern "C" int mmb_colmax(const float* x, int64_t n, int d, uint32_t* colmax, int accumulate,
                          hipStream_t stream) {
  MMB_REQUIRE(x && colmax && n >= 0 && d > 0);
  MMB_REQUIRE(ceil_div(n, 256) <= kMaxGridX);  // a workgroup per 256 rows
  if (!accumulate) {
    const hipError_t e = static_cast<hipError_t>(zero_words_async(colmax, static_cast<int64_t>(sizeof(uint32_t) * d) / 4, stream));
    if (e != hipSuccess) return static_cast<int>(e);
  }
  if (n == 0) return MMB_OK;
  const int64_t rpb = 256;
  const int64_t blocks = ceil_div(n, rpb);
  colmax_kernel<<<static_cast<int>(blocks), d < 256 ? ((d + 63) / 64) * 64 : 256, 0, stream>>>(
      x, n, d, rpb, colmax);
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

extern "C" int mmb_gram_i8(const float* x, const uint32_t* colmax, int64_t n, int d, double* g,
                           int accumulate, void* ws, hipStream_t stream) {
  MMB_REQUIRE(x && colmax && g && ws && n >= 0 && d > 0 && d <= 304 && d % 4 == 0);
  double* part = static_cast<double*>(ws);
#ifndef MMB_HOOK_GRAM_I8  // (tools/diag: MMB_GRAM_I8_V1, the r04 kernel)
#define MMB_HOOK_GRAM_I8(rc) false
#endif
  {
    int rc_ = MMB_OK;
    if (MMB_HOOK_GRAM_I8(rc_)) return rc_;
  }
  // blocks of <= kGlBlockRows rows (<= 128 ranges of <= 32768 rows: int32
  // level sums, at most 128 range partials per reduction); the first block
  // writes (or accumulates into) g, later ones accumulate
  int64_t b0 = 0;
  do {
    const int64_t nb = std::min(n - b0, kGlBlockRows);
    const float* xb = x + b0 * d;
    const int acc = accumulate || b0 > 0;
#ifndef MMB_HOOK_GRAM_I8_BLOCK  // (tools/diag: MMB_GRAM_I8_SHAPE / MMB_GRAM_DIAG)
#define MMB_HOOK_GRAM_I8_BLOCK gram_i8l_block<0, GlProduct, true>
#endif
    const int rc = MMB_HOOK_GRAM_I8_BLOCK(xb, colmax, nb, d, g, acc, part, stream);
    if (rc != MMB_OK) return rc;
    b0 += nb;
  } while (b0 < n);
  return MMB_OK;
}

extern "C" int mmb_gram_part(const float* num, const float* cnt, int64_t n, int64_t n_plan, int d,
                             int accumulate, void* ws, hipStream_t stream) {
  MMB_REQUIRE(num && ws && n >= 0 && n <= n_plan && d > 0 && gram2_ok(num, d));
  const Gram2Plan q = gram2_plan(n_plan, d);
  gram_tri_kernel<<<2 * q.R, kG2NT, gram2_lds(), stream>>>(num, cnt, n, d, q.nt, q.R, q.chunk, q.xcd,
                                                           accumulate ? 1 : 0,
                                                           static_cast<double*>(ws));
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

extern "C" int mmb_gram_finish(int64_t n_plan, int d, double* g, int accumulate, const void* ws,
                               hipStream_t stream) {
  MMB_REQUIRE(g && ws && n_plan >= 0 && d > 0 && d % 4 == 0 && d <= 320);
  const Gram2Plan q = gram2_plan(n_plan, d);
  {
    const int rc = launch_tri_reduce(static_cast<const double*>(ws), d, q.nt, q.R, accumulate, g, stream);
    if (rc != MMB_OK) return rc;
  }
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

// float64 X: the numpy drop-ins (compute_pc / remove_pc) take any X; the
// reference runs randomized SVD and the removal on it in f64
// (sif_functions.py:58-81).  X that is not f32-representable takes the generic
// route on its f64 rows instead of being rounded (as mmb_xt_omega_f64 and
// mmb_pc_remove_f64 do for X^T Omega and the removal).
extern "C" int mmb_gram_f64(const double* x, int64_t n, int d, double* g, int accumulate, void* ws,
                            hipStream_t stream) {
  MMB_REQUIRE(x && g && ws && n >= 0 && d > 0);
  return launch_gram_generic(x, nullptr, n, d, g, accumulate, static_cast<double*>(ws), stream);
}

// the tools build's variant kernels, launches, knobs and entry points
// (tools/diag/); the product library includes an empty header here
#ifndef MMB_TOOLS_TAIL_GRAM
#define MMB_TOOLS_TAIL_GRAM "mmb_no_tools.h"
#endif
#include MMB_TOOLS_TAIL_GRAM
