// The stream kernels proper as templates -- utt_stream_kernel (a workgroup
// per utterance) and utt_wave_kernel (a wave per utterance) -- with their
// launchers and the route selection of the MMB2 stream entry points.  Three
// sources instantiate them, one per word-table element type TE:
// sif_kernels.hip every f32-table kernel (mmb_sif_wavg, mmb_mm2_stream,
// mmb_mm2_stream_ft), sif_tab_f16_kernels.hip and sif_tab_bf16_kernels.hip
// the kernels of a 16-bit table (mmb_sif_wavg_tt, mmb_mm2_stream_tt).  A
// kernel is in exactly one code object: an instantiation's TE names its
// source.  Included by those three only.
#pragma once
#include "mmb_stream.h"

namespace mmb {

#pragma GCC visibility push(hidden)
// (sif_kernels.hip: the f32 wave kernel's narrow-frame route, and the pass
// that makes the workgroup kernel's fp32 sums fp16 hi | lo -- a kernel that
// is not a template, launched from its own source)
bool narrow_ok(const StreamArgs& a);
int narrow_variant();
int launch_narrow(const StreamArgs& a, hipStream_t stream, int* parts);
int split_rows(const StreamArgs& s, hipStream_t stream);
#pragma GCC visibility pop

// FU: frame rows (and TU: text rows) per thread in flight -- 4 / 4 when the
// grid fills the chip (occupancy hides the latency); for a few hundred long
// rows (dataset splits: one workgroup per CU at most, so one workgroup's
// loads in flight set the time; POM's 100-row valid split spent 0.18 ms in 68
// rounds of 4 frame loads per thread) NT = 1024 threads with 8 / 4.  NT
// changes the f32 order of the row sums (RT = NT / CT row slots).
// FE: the frame element type (float, f16_t or bf16_t).
// TE: the word table's element type (float, f16_t or bf16_t; a 16-bit table
// is gathered text: a.ids is set).
template <bool MM2, int VT, int VA, int VV, int FU = 4, int TU = 4, int NT = kNT, class FE = float,
          class TE = float>
__global__ __launch_bounds__(NT) void utt_stream_kernel(StreamArgs a) {
  constexpr int kRF = NT * 4;  // one accumulator image: R*F <= NT*VEC
  constexpr int kSI = (kTokChunk + NT - 1) / NT;
  __shared__ int64_t s_off[kTokChunk];
  __shared__ float s_w[kTokChunk];
  __shared__ float s_red[(MM2 ? 4 : 1) * kRF];
  __shared__ float s_cnt[NT / kWave], s_sw[NT / kWave];
  __shared__ float s_c0[NT / kWave], s_w0[NT / kWave];
  __shared__ int s_keep[kSI][NT / kWave];

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  // text lane map: CT column units of VT floats, RT row slots
  const int CT = a.D / VT;
  const int RT = NT / CT;
  const int rT = tid / CT, cT = tid - (tid / CT) * CT;
  const bool actT = rT < RT;
  // audio / visual lane maps
  const int CA = MM2 ? a.A / VA : 1, RA = NT / CA;
  const int rA = tid / CA, cA = tid - rA * CA;
  const int CV = MM2 ? a.Vd / VV : 1, RV = NT / CV;
  const int rV = tid / CV, cV = tid - rV * CV;
  // (the rows of a 16-bit table: StreamArgs::table read as elements of TE)
  const TE* tsrc = reinterpret_cast<const TE*>(a.ids ? a.table : a.text_dense);
  const TE* esrc = reinterpret_cast<const TE*>(a.ids ? a.table : a.emb_dense);
  const bool split_emb = MM2 && (esrc != tsrc);

  const bool gather = a.ids != nullptr;
  float cmx0 = 0.f, cmx1 = 0.f;  // running max |x| of columns tid, tid + NT (MMB2)
  for (int64_t i = blockIdx.x; i < a.N; i += gridDim.x) {
    float num[VT], sx[VT], sxx[VT];
#pragma unroll
    for (int e = 0; e < VT; ++e) num[e] = sx[e] = sxx[e] = 0.f;
    float cntp = 0.f, swp = 0.f, c0p = 0.f, w0p = 0.f;

    for (int t0 = 0; t0 < a.L; t0 += kTokChunk) {
      const int tl = min(kTokChunk, a.L - t0);
      int64_t off_k[kSI];
      float w_k[kSI];
      int rank_k[kSI];
      bool keep_k[kSI];
#pragma unroll
      for (int k = 0; k < kSI; ++k) {
        const int t = tid + k * NT;
        int64_t off = -1;
        float w = 0.f;
        if (t < tl) {
          stage_token(a, i, t0 + t, off, w);
          cntp += (w != 0.f) ? 1.f : 0.f;
          swp += w;
          if (gather && off == 0) {
            c0p += 1.f;
            w0p += w;
          }
        }
        const bool keep = t < tl && (gather ? off > 0 : true);
        const unsigned long long bal = __ballot(keep);
        rank_k[k] = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_keep[k][wave] = __popcll(bal);
        off_k[k] = off;
        w_k[k] = w;
        keep_k[k] = keep;
      }
      __syncthreads();
      int nkeep = 0;
#pragma unroll
      for (int k = 0; k < kSI; ++k) {
        for (int v = 0; v < NT / kWave; ++v) {
          if (keep_k[k] && v == wave) s_off[nkeep + rank_k[k]] = off_k[k];
          if (keep_k[k] && v == wave) s_w[nkeep + rank_k[k]] = w_k[k];
          nkeep += s_keep[k][v];
        }
      }
      __syncthreads();
      if (actT) {
        // branch-free: a negative offset (negative or flagged id) loads row
        // 0 and contributes nothing, so the unrolled iterations keep their
        // loads in flight together (a `continue` per token would wait on
        // each load right after its branch)
        if constexpr (!std::is_same_v<TE, float>)  // a table's rows: never a second dense tensor
          text_rows<MM2, false, VT, TU, TE>(tsrc, esrc, s_off, s_w, nkeep, rT, RT, cT, num, sx, sxx);
        else if (split_emb)
          text_rows<MM2, true, VT, TU>(tsrc, esrc, s_off, s_w, nkeep, rT, RT, cT, num, sx, sxx);
        else
          text_rows<MM2, false, VT, TU>(tsrc, esrc, s_off, s_w, nkeep, rT, RT, cT, num, sx, sxx);
      }
      __syncthreads();
    }

    // audio / visual frame sums (MMB2 only): sum_t x and sum_t x^2 per feature
    float sa[VA], saa[VA], sv[VV], svv[VV];
#pragma unroll
    for (int e = 0; e < VA; ++e) sa[e] = saa[e] = 0.f;
#pragma unroll
    for (int e = 0; e < VV; ++e) sv[e] = svv[e] = 0.f;
    if constexpr (MM2) {
      if (rA < RA) {
        const FE* base = frames<FE>(a.audio) + (i * a.L) * a.A + cA * VA;
#pragma unroll FU
        for (int t = rA; t < a.L; t += RA) {
          float v[VA];
          ldv_nt<VA>(base + static_cast<int64_t>(t) * a.A, v);
#pragma unroll
          for (int e = 0; e < VA; ++e) {
            sa[e] += v[e];
            saa[e] = fmaf(v[e], v[e], saa[e]);
          }
        }
      }
      if (rV < RV) {
        const FE* base = frames<FE>(a.visual) + (i * a.L) * a.Vd + cV * VV;
#pragma unroll FU
        for (int t = rV; t < a.L; t += RV) {
          float v[VV];
          ldv_nt<VV>(base + static_cast<int64_t>(t) * a.Vd, v);
#pragma unroll
          for (int e = 0; e < VV; ++e) {
            sv[e] += v[e];
            svv[e] = fmaf(v[e], v[e], svv[e]);
          }
        }
      }
    }

    // count_nonzero(w) and sum(w) (and the row-0 token count / weight sum):
    // wave shuffle then fixed-order wave sum
    cntp = wave_sum(cntp);
    swp = wave_sum(swp);
    c0p = wave_sum(c0p);
    w0p = wave_sum(w0p);
    if (lane == 0) {
      s_cnt[wave] = cntp;
      s_sw[wave] = swp;
      s_c0[wave] = c0p;
      s_w0[wave] = w0p;
    }
    // round 1: text accumulators
    if (actT) {
#pragma unroll
      for (int e = 0; e < VT; ++e) {
        const int f = rT * a.D + cT * VT + e;
        s_red[f] = num[e];
        if constexpr (MM2) {
          s_red[kRF + f] = sx[e];
          s_red[2 * kRF + f] = sxx[e];
        }
      }
    }
    __syncthreads();
    float cnt = 0.f, sw = 0.f, c0 = 0.f, w0 = 0.f;
#pragma unroll
    for (int w = 0; w < NT / kWave; ++w) {
      cnt += s_cnt[w];
      sw += s_sw[w];
      c0 += s_c0[w];
      w0 += s_w0[w];
    }
    float smax = 0.f;  // max |sum| of this thread's part of the row (MMB2)
    for (int f = tid; f < a.D; f += NT) {
      float n_ = 0.f;
      for (int r = 0; r < RT; ++r) n_ += s_red[r * a.D + f];
      // row 0 once for its c0 tokens (gather mode; c0 = 0 otherwise)
      const float e0 = (c0 > 0.f) ? table_f32<TE>(a.table, f) : 0.f;
      n_ = fmaf(w0, e0, n_);
      if constexpr (MM2) {
        float x1 = 0.f, x2 = 0.f;
        for (int r = 0; r < RT; ++r) {
          x1 += s_red[kRF + r * a.D + f];
          x2 += s_red[2 * kRF + r * a.D + f];
        }
        x1 = fmaf(c0, e0, x1);
        x2 = fmaf(c0 * e0, e0, x2);
        const float xf = n_ / cnt;
        a.num_out[i * a.D + f] = xf;  // x = the a2 row (sif_functions.py:55)
        if (f < NT) cmx0 = bmax(cmx0, fabsf(xf)); else cmx1 = bmax(cmx1, fabsf(xf));
        a.s_out[i * a.Kp + f] = x1;
        a.s_out[i * a.Kp + a.D + f] = x2;
        smax = fmaxf(smax, fmaxf(fabsf(x1), fabsf(x2)));
      } else {
        if (a.num_out) a.num_out[i * a.D + f] = n_;
        if (a.x_out) a.x_out[i * a.D + f] = n_ / cnt;
      }
    }
    if (tid == 0) {
      if (cnt == 0.f && a.flag) atomicOr(a.flag, MMB_FLAG_ZERO_WEIGHTS);
      if constexpr (MM2) {
        a.aux_out[i] = cnt;         // planar [3][N]: row 0 doubles as the SIF count
        a.aux_out[a.N + i] = sw;
      } else {
        if (a.cnt_out) a.cnt_out[i] = cnt;
      }
    }
    if constexpr (MM2) {
      __syncthreads();
      // round 2: audio and visual accumulators
      if (rA < RA) {
#pragma unroll
        for (int e = 0; e < VA; ++e) {
          const int f = rA * a.A + cA * VA + e;
          s_red[f] = sa[e];
          s_red[kRF + f] = saa[e];
        }
      }
      if (rV < RV) {
#pragma unroll
        for (int e = 0; e < VV; ++e) {
          const int f = rV * a.Vd + cV * VV + e;
          s_red[2 * kRF + f] = sv[e];
          s_red[3 * kRF + f] = svv[e];
        }
      }
      __syncthreads();
      float* srow = a.s_out + i * a.Kp + 2 * a.D;
      for (int f = tid; f < a.A; f += NT) {
        float x1 = 0.f, x2 = 0.f;
        for (int r = 0; r < RA; ++r) {
          x1 += s_red[r * a.A + f];
          x2 += s_red[kRF + r * a.A + f];
        }
        srow[f] = x1;
        srow[a.A + f] = x2;
        smax = fmaxf(smax, fmaxf(fabsf(x1), fabsf(x2)));
      }
      for (int f = tid; f < a.Vd; f += NT) {
        float x1 = 0.f, x2 = 0.f;
        for (int r = 0; r < RV; ++r) {
          x1 += s_red[2 * kRF + r * a.Vd + f];
          x2 += s_red[3 * kRF + r * a.Vd + f];
        }
        srow[2 * a.A + f] = x1;
        srow[2 * a.A + a.Vd + f] = x2;
        smax = fmaxf(smax, fmaxf(fabsf(x1), fabsf(x2)));
      }
      const int k = 2 * (a.D + a.A + a.Vd);
      for (int f = k + tid; f < a.Kp; f += NT) a.s_out[i * a.Kp + f] = 0.f;
      smax = wave_max(smax);
      if (lane == 0) s_cnt[wave] = smax;
      __syncthreads();
      if (tid == 0) {
        float m = 0.f;
        for (int w = 0; w < NT / kWave; ++w) m = fmaxf(m, s_cnt[w]);
        a.aux_out[2 * a.N + i] = row_scale(m);
      }
    }
    __syncthreads();
  }
  if (MM2 && a.cmax_part) {  // this workgroup's column bounds (mmb_gram_i8)
    float* pr = a.cmax_part + static_cast<int64_t>(blockIdx.x) * a.D;
    if (tid < a.D) pr[tid] = cmx0;
    if (tid + NT < a.D) pr[tid + NT] = cmx1;
  }
}

// ---------------------------------------------------------------------------
// Wave-per-utterance variant (tokens/frames <= 64, widths % 4 == 0, <= 512):
// the fast path for MOSI / synthetic shapes.  One wave owns one utterance:
// lane t stages token t (id, weight) in registers and the loop broadcasts it
// with v_readlane, lane l owns float4 columns l and l+64 of every row for the
// whole utterance, so there is no LDS, no barrier and no cross-lane reduction
// of the sums — only independent 16-B loads (3 rows per frame in MMB2 mode)
// that the compiler keeps in flight across unrolled frames.

// Per-utterance sums of the wave-per-utterance kernels (utt_wave_kernel,
// utt_fused_kernel): lane t stages token t, the frame loop broadcasts it with
// v_readlane, lane l owns float4 columns l + 64 c of every row.
template <int CT, int CA, int CV>
struct UttSums {
  float4 num[CT], sx[CT], sxx[CT], sa[CA], saa[CA], sv[CV], svv[CV];
  float cnt, sw;
};

// A loaded frame column unit (4 values) as the load group holds it until its
// frame is summed: the float4 itself, or for a 16-bit frame type the 8 bytes
// still packed (half the registers of a group in flight), widened in accum.
template <class FE>
struct FrameUnit {
  using type = u2;
  template <bool NT>
  static __device__ __forceinline__ u2 load(const FE* p) {
    if constexpr (NT) {
      return __builtin_nontemporal_load(reinterpret_cast<const u2*>(p));
    } else {
      return *reinterpret_cast<const u2*>(p);
    }
  }
  static __device__ __forceinline__ float4 f32(u2 q) { return frame_f32x4<FE>(q); }
};
template <>
struct FrameUnit<float> {
  using type = float4;
  template <bool NT>
  static __device__ __forceinline__ float4 load(const float* p) { return ldnt4<NT>(p); }
  static __device__ __forceinline__ float4 f32(float4 q) { return q; }
};

// The same for a loaded text column unit: of a 16-bit word table the 8 bytes
// still packed, from a plain load (cached: the table rows are the reused data).
template <class TE>
struct TextUnit {
  using type = u2;
  static __device__ __forceinline__ u2 load(const TE* p) { return *reinterpret_cast<const u2*>(p); }
  static __device__ __forceinline__ float4 f32(u2 q) { return frame_f32x4<TE>(q); }
};
template <>
struct TextUnit<float> {
  using type = float4;
  static __device__ __forceinline__ float4 load(const float* p) { return ld4(p); }
  static __device__ __forceinline__ float4 f32(float4 q) { return q; }
};

// FE: the frame element type (float, f16_t or bf16_t).
// TE: the word table's element type (float, f16_t or bf16_t): a text column
// unit of a 16-bit table is one 8-byte load, kept packed by its load group as
// a 16-bit frame unit is.
template <bool MM2, int CT, int CA, int CV, int UNR, bool NT, bool SPLIT, class FE = float,
          class TE = float>
__device__ __forceinline__ void utt_sums(const StreamArgs& a, int64_t i, int lane,
                                         UttSums<CT, CA, CV>& u) {
  using FU = FrameUnit<FE>;
  using fu_t = typename FU::type;
  using TX = TextUnit<TE>;
  using tx_t = typename TX::type;
  static_assert(std::is_same_v<TE, float> || !SPLIT, "a 16-bit table is gathered text");
  const int UT = a.D >> 2, UA = a.A >> 2, UV = a.Vd >> 2;
  // (the rows of a 16-bit table: StreamArgs::table read as elements of TE)
  const TE* tsrc = reinterpret_cast<const TE*>(a.ids ? a.table : a.text_dense);
  const float* esrc = a.ids ? a.table : a.emb_dense;
  constexpr bool split_emb = MM2 && SPLIT;  // weighted sum over a different dense tensor
  const bool gather = a.ids != nullptr;
  // stage: lane t <- token t (row id or -1, weight)
  int rid = -1;
  float w = 0.f;
  if (lane < a.L) {
    int64_t off;
    stage_token(a, i, lane, off, w);
    rid = off < 0 ? -1 : (gather ? static_cast<int>(off / a.D) : lane);
  }
  u.cnt = wave_sum((w != 0.f) ? 1.f : 0.f);
  u.sw = wave_sum(w);
  // every weight 0: x is 0/0 = NaN (numpy's answer); the reference's
  // TruncatedSVD then rejects the split -- report it through the flag word
  if (lane == 0 && u.cnt == 0.f && a.flag) atomicOr(a.flag, MMB_FLAG_ZERO_WEIGHTS);

  float4 (&num)[CT] = u.num;
  float4 (&sx)[CT] = u.sx;
  float4 (&sxx)[CT] = u.sxx;
  float4 (&sa)[CA] = u.sa;
  float4 (&saa)[CA] = u.saa;
  float4 (&sv)[CV] = u.sv;
  float4 (&svv)[CV] = u.svv;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int c = 0; c < CT; ++c) num[c] = sx[c] = sxx[c] = z4;
#pragma unroll
  for (int c = 0; c < CA; ++c) sa[c] = saa[c] = z4;
#pragma unroll
  for (int c = 0; c < CV; ++c) sv[c] = svv[c] = z4;
  const FE* abase = frames<FE>(a.audio) + i * a.L * a.A;
  const FE* vbase = frames<FE>(a.visual) + i * a.L * a.Vd;
  const int64_t dbase = i * a.L;
  // Column offsets clamped into the row so every lane loads unconditionally:
  // lanes past a row's width read a valid duplicate and never store it.  A
  // group of UNR frames issues ALL its loads before any accumulation — no
  // branch separates them, so UNR frames x (CT+CA+CV) 16-B loads per lane
  // are in flight together (a guarded load per lane would be waited on
  // right after its branch: one load in flight per wave).
  int ct[CT], ca[CA], cv[CV];
#pragma unroll
  for (int c = 0; c < CT; ++c) ct[c] = 4 * min(lane + kWave * c, UT - 1);
#pragma unroll
  for (int c = 0; c < CA; ++c) ca[c] = 4 * min(lane + kWave * c, MM2 ? UA - 1 : 0);
#pragma unroll
  for (int c = 0; c < CV; ++c) cv[c] = 4 * min(lane + kWave * c, MM2 ? UV - 1 : 0);
  auto frame = [&](int t, tx_t (&vt)[CT], float4 (&ve)[CT], fu_t (&va)[CA],
                   fu_t (&vv)[CV], float& wt, bool& ok) {
    const int r = __builtin_amdgcn_readlane(rid, t);
    wt = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), t));
    ok = r >= 0;  // an out-of-range id (flagged) contributes a zero row
    const int64_t o = (gather ? static_cast<int64_t>(ok ? r : 0) : dbase + t) * a.D;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      vt[c] = TX::load(tsrc + o + ct[c]);
      if (split_emb) ve[c] = ld4(esrc + o + ct[c]);
    }
    if constexpr (MM2) {
#pragma unroll
      for (int c = 0; c < CA; ++c) va[c] = FU::template load<NT>(abase + static_cast<int64_t>(t) * a.A + ca[c]);
#pragma unroll
      for (int c = 0; c < CV; ++c) vv[c] = FU::template load<NT>(vbase + static_cast<int64_t>(t) * a.Vd + cv[c]);
    }
  };
  auto accum = [&](tx_t (&vt)[CT], float4 (&ve)[CT], fu_t (&va)[CA], fu_t (&vv)[CV],
                   float wt, bool ok) {
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const float4 v = ok ? TX::f32(vt[c]) : z4;
      fma4(num[c], wt, split_emb ? (ok ? ve[c] : z4) : v);
      if constexpr (MM2) {
        add4(sx[c], v);
        sq4(sxx[c], v);
      }
    }
    if constexpr (MM2) {
#pragma unroll
      for (int c = 0; c < CA; ++c) {
        const float4 x = FU::f32(va[c]);
        add4(sa[c], x);
        sq4(saa[c], x);
      }
#pragma unroll
      for (int c = 0; c < CV; ++c) {
        const float4 x = FU::f32(vv[c]);
        add4(sv[c], x);
        sq4(svv[c], x);
      }
    }
  };
  int t = 0;
  for (; t + UNR <= a.L; t += UNR) {
    tx_t vt[UNR][CT];
    float4 ve[UNR][CT];
    fu_t va[UNR][CA], vv[UNR][CV];
    float wt[UNR];
    bool ok[UNR];
#pragma unroll
    for (int q = 0; q < UNR; ++q) frame(t + q, vt[q], ve[q], va[q], vv[q], wt[q], ok[q]);
#pragma unroll
    for (int q = 0; q < UNR; ++q) accum(vt[q], ve[q], va[q], vv[q], wt[q], ok[q]);
  }
  for (; t < a.L; ++t) {
    tx_t vt[CT];
    float4 ve[CT];
    fu_t va[CA], vv[CV];
    float wt;
    bool ok;
    frame(t, vt, ve, va, vv, wt, ok);
    accum(vt, ve, va, vv, wt, ok);
  }
}

template <bool MM2, int CT, int CA, int CV, int UNR = 2, bool NT = false, bool SPLIT = false,
          bool NTS = false, int OCC = 1, class FE = float, class TE = float>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(OCC, 8))) void utt_wave_kernel(
    StreamArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wid = static_cast<int64_t>(blockIdx.x) * (blockDim.x / kWave) + threadIdx.x / kWave;
  const int64_t nw = static_cast<int64_t>(gridDim.x) * (blockDim.x / kWave);
  const int UT = a.D >> 2, UA = a.A >> 2, UV = a.Vd >> 2;

  float4 cmx[CT];  // running max |x| of this lane's columns (MMB2, mmb_gram_i8)
#pragma unroll
  for (int c = 0; c < CT; ++c) cmx[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t i = wid; i < a.N; i += nw) {
    UttSums<CT, CA, CV> u;
    utt_sums<MM2, CT, CA, CV, UNR, NT, SPLIT, FE, TE>(a, i, lane, u);
    const float cnt = u.cnt, sw = u.sw;
    float4 (&num)[CT] = u.num;
    float4 (&sx)[CT] = u.sx;
    float4 (&sxx)[CT] = u.sxx;
    float4 (&sa)[CA] = u.sa;
    float4 (&saa)[CA] = u.saa;
    float4 (&sv)[CV] = u.sv;
    float4 (&svv)[CV] = u.svv;

    if constexpr (MM2) {
      float m = 0.f;
#pragma unroll
      for (int c = 0; c < CT; ++c) m = fmaxf(m, fmaxf(amax4(sx[c]), amax4(sxx[c])));
#pragma unroll
      for (int c = 0; c < CA; ++c) m = fmaxf(m, fmaxf(amax4(sa[c]), amax4(saa[c])));
#pragma unroll
      for (int c = 0; c < CV; ++c) m = fmaxf(m, fmaxf(amax4(sv[c]), amax4(svv[c])));
      const float rs = row_scale(wave_max(m));
      // one sums row: fp32, or fp16 hi | lo planes of the row-scaled sums (the
      // projection GEMM's A operand, ready for direct global->LDS staging)
      float* srow = a.s_out + i * a.Kp;
      _Float16* hrow = reinterpret_cast<_Float16*>(a.s_out) + i * 2 * a.Kp;
      auto put = [&](int f, float4 v) {
        if (a.s_half) {
          split_store4<NTS>(hrow + f, hrow + a.Kp + f, v, rs);
        } else {
          stnt4<NTS>(srow + f, v);
        }
      };
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        const int u = lane + kWave * c;
        if (u < UT) {
          const float4 xr = div4(num[c], cnt);
          stnt4<NTS>(a.num_out + i * a.D + 4 * u, xr);  // x = the a2 row
          cmx[c] = bmax4(cmx[c], xr);
          put(4 * u, sx[c]);
          put(a.D + 4 * u, sxx[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < CA; ++c) {
        const int u = lane + kWave * c;
        if (u < UA) {
          put(2 * a.D + 4 * u, sa[c]);
          put(2 * a.D + a.A + 4 * u, saa[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < CV; ++c) {
        const int u = lane + kWave * c;
        if (u < UV) {
          put(2 * (a.D + a.A) + 4 * u, sv[c]);
          put(2 * (a.D + a.A) + a.Vd + 4 * u, svv[c]);
        }
      }
      const int k = 2 * (a.D + a.A + a.Vd);
      for (int f = k + lane; f < a.Kp; f += kWave) {
        if (a.s_half) {
          hrow[f] = hrow[a.Kp + f] = static_cast<_Float16>(0.f);
        } else {
          srow[f] = 0.f;
        }
      }
      if (lane == 0) {
        a.aux_out[i] = cnt;  // planar [3][N]: count | sum w | fp16 row scale
        a.aux_out[a.N + i] = sw;
        a.aux_out[2 * a.N + i] = rs;
      }
    } else {
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        const int u = lane + kWave * c;
        if (u < UT) {
          if (a.num_out) st4(a.num_out + i * a.D + 4 * u, num[c]);
          if (a.x_out) st4(a.x_out + i * a.D + 4 * u, div4(num[c], cnt));
        }
      }
      if (lane == 0 && a.cnt_out) a.cnt_out[i] = cnt;
    }
  }
  if (MM2 && a.cmax_part) {  // this wave's column bounds (mmb_gram_i8)
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const int u = lane + kWave * c;
      if (u < UT) st4(a.cmax_part + wid * a.D + 4 * u, cmx[c]);
    }
  }
}

// Load/store policy of the MMB2 wave kernel: bit 0 = frame loads
// non-temporal, bit 1 = output stores non-temporal, bit 2 = 4 frames per load
// group instead of 2.  Default 5 (4-frame groups, non-temporal frame loads):
// measured on MI355X at 1M x 40 x 3 x 300-d, Zipf ids (tools/policy_sweep.sh):
// policy 0/1/2/3/4/5/6/7 = 20.65/20.62/21.00/19.94/20.54/19.80/20.57/20.09 ms;
// uniform ids 26.87 (0) -> 24.23 (5).  MMB_STREAM_POLICY overrides it (read
// once) for such sweeps.
// Read per launch (in-process A/B sweeps flip it).  Bit 3 (policy 13):
// the default variant compiled for two waves per SIMD (amdgpu_waves_per_eu).
// The sweep knobs (this one, MMB_STREAM_GRID_MULT, the fused kernel's
// MMB_FUSED_*, the projection's MMB_PROJ_*, MMB_GRAM_DIAG, MMB_PC_REMOVE_R)
// exist only in the tools build (libmmb_diag.so, tools/diag/): at each
// MMB_HOOK_* point below the product library compiles its default and reads
// no environment variable.

template <bool MM2, int CT, int CA, int CV, int UNR, bool NT, bool NTS, int OCC = 1>
static void launch_wave_v(const StreamArgs& a, int grid, hipStream_t stream) {
  if (MM2 && a.ids == nullptr && a.emb_dense != a.text_dense) {
    utt_wave_kernel<MM2, CT, CA, CV, UNR, NT, true, NTS, OCC><<<grid, 256, 0, stream>>>(a);
  } else {
    utt_wave_kernel<MM2, CT, CA, CV, UNR, NT, false, NTS, OCC><<<grid, 256, 0, stream>>>(a);
  }
}

// Workgroups per CU of the grid-stride wave kernel: 2 = exactly the resident
// waves at its occupancy (2 waves / SIMD), one even share of utterances per
// wave.  Measured (tools/grid_sweep.sh, MI355X): 2/4/8/16/32 = 20.88/20.94/
// 21.04/21.01/21.18 ms.  MMB_STREAM_GRID_MULT overrides it (tools build).
#ifndef MMB_HOOK_STREAM_GRID_MULT
#define MMB_HOOK_STREAM_GRID_MULT 2
#endif
static int stream_grid_mult() { return MMB_HOOK_STREAM_GRID_MULT; }


// The wave kernels' grid: workgroups of 4 waves, a wave per utterance at a
// time -- ceil(N / 4) of them, at most per_cu per CU of the stream (the
// resident ones: the rest of the rows by grid stride) and, where the column
// bounds are taken, at most kCmaxRows / 4 (a partial row per wave: *parts).
static int wave_grid(const StreamArgs& a, int per_cu, hipStream_t stream, int* parts) {
  const int64_t blocks = ceil_div(a.N, 4);
  int grid_cap = per_cu * stream_cu_count(stream);
  if (a.cmax_part && grid_cap > kCmaxRows / 4) grid_cap = kCmaxRows / 4;
  const int grid = static_cast<int>(blocks < grid_cap ? blocks : grid_cap);
  if (parts) *parts = grid * 4;
  return grid;
}

template <bool MM2, int CT, int CA, int CV, class FE = float, class TE = float>
static int launch_wave(const StreamArgs& a, hipStream_t stream, int* parts = nullptr) {
  if constexpr (!std::is_same_v<TE, float>) {
    // a 16-bit word table (mmb_sif_wavg_tt, mmb_mm2_stream_tt), frames of any
    // type: the policy of the f32-table kernel of its mode (MMB2: 4-frame
    // groups, non-temporal frame loads; SIF: 2-token groups), the table rows
    // in plain cached loads, and never the narrow-frame kernel
    const int grid = wave_grid(a, stream_grid_mult(), stream, parts);
    utt_wave_kernel<MM2, CT, CA, CV, MM2 ? 4 : 2, MM2, false, false, 1, FE, TE><<<grid, 256, 0, stream>>>(a);
    MMB_LAUNCH_CHECK();
    return MMB_OK;
  } else if constexpr (!std::is_same_v<FE, float>) {
    // 16-bit frames (mmb_mm2_stream_ft): the MMB2 policy below (4-frame
    // groups, non-temporal frame loads), and never the narrow-frame kernel,
    // whose packed frame loads are f32 only
    static_assert(MM2, "16-bit frames are an MMB2 input");
    const int grid = wave_grid(a, stream_grid_mult(), stream, parts);
#ifndef MMB_HOOK_WAVE16_LAUNCH  // (tools/diag: the frame-group depth, MMB_FRAMES16_UNR)
#define MMB_HOOK_WAVE16_LAUNCH false
#endif
    if (!(MMB_HOOK_WAVE16_LAUNCH)) {
      utt_wave_kernel<true, CT, CA, CV, 4, true, false, false, 1, FE><<<grid, 256, 0, stream>>>(a);
    }
    MMB_LAUNCH_CHECK();
    return MMB_OK;
  } else {
    if (MM2 && narrow_ok(a) && narrow_variant() > 0) return launch_narrow(a, stream, parts);
    const int grid = wave_grid(a, stream_grid_mult(), stream, parts);
#ifndef MMB_HOOK_WAVE_LAUNCH  // (tools/diag: the stream-policy sweep)
#define MMB_HOOK_WAVE_LAUNCH false
#endif
    if (!(MMB_HOOK_WAVE_LAUNCH)) {
      if constexpr (MM2) {  // policy 5: 4-frame groups, non-temporal frame loads
        launch_wave_v<MM2, CT, CA, CV, 4, true, false>(a, grid, stream);
      } else {
        launch_wave_v<MM2, CT, CA, CV, 2, false, false>(a, grid, stream);
      }
    }
    MMB_LAUNCH_CHECK();
    return MMB_OK;
  }
}

template <bool MM2, int VT, int VA, int VV, class FE = float, class TE = float>
static int launch_stream(const StreamArgs& a, hipStream_t stream, int* parts = nullptr) {
  int grid = stream_grid(a.N, 6, stream);
  if (a.cmax_part && grid > kCmaxRows) grid = kCmaxRows;
  if (parts) *parts = grid;
  if (MM2 && a.N <= stream_cu_count(stream)) {
    // a few long rows (POM's splits: 100 / 203 rows of 1089 / 1357 tokens):
    // 16 frame / 8 text rows in flight per group instead of 4 / 4 (r05
    // tools/splits_ab.py, gpurun_out r05m: stream 0.180 -> 0.148 ms and
    // 0.217 -> 0.188 ms, the same sums bit for bit; 1024 threads x 4 / 4:
    // 0.157 / 0.193 ms)
#ifndef MMB_HOOK_STREAM_SMALL  // (tools/diag: MMB_STREAM_SMALL)
#define MMB_HOOK_STREAM_SMALL false
#endif
    bool swept = false;  // (f32 frames and table only)
    if constexpr (std::is_same_v<FE, float> && std::is_same_v<TE, float>) swept = MMB_HOOK_STREAM_SMALL;
    if (!swept) {
      utt_stream_kernel<MM2, VT, VA, VV, 16, 8, kNT, FE, TE><<<grid, kNT, 0, stream>>>(a);
    }
  } else
    utt_stream_kernel<MM2, VT, VA, VV, 4, 4, kNT, FE, TE><<<grid, kNT, 0, stream>>>(a);
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

// The routes of mmb_mm2_stream, mmb_mm2_stream_ft and mmb_mm2_stream_tt on
// frames of type FE and a word table of type TE, after the entry point's
// checks: the wave kernel where every modality and both outputs take vector
// rows (a unit is 4 values: 16 bytes of f32, 8 of a 16-bit type), else the
// workgroup kernel (and the pass that makes its fp32 sums fp16 hi | lo); then
// the column bounds.
template <class FE, class TE = float>
static int stream_route(StreamArgs& s, uint32_t* colmax, hipStream_t stream) {
  int parts = 0;
  const int s_half = s.s_half;
  const StreamVec vec = stream_vec(s, sizeof(FE), sizeof(TE));
  // the wave kernel: vector rows of every modality and of both outputs, at
  // most 64 tokens and 512 columns; anything else is not rejected but falls
  // through to the workgroup kernel
  if (vec.t && vec.a && vec.v && s.L <= kWave && s.D <= 512 && s.A <= 512 && s.Vd <= 512 &&
      aligned16(s.num_out) && aligned16(s.s_out)) {
    const int rc = dispatch3(s.D > 256, s.A > 256, s.Vd > 256, [&](auto ct, auto ca, auto cv) {
      return launch_wave<true, ct.value ? 2 : 1, ca.value ? 2 : 1, cv.value ? 2 : 1, FE, TE>(s, stream, &parts);
    });
    return reduce_colmax(rc, s, parts, colmax, stream);
  }
  MMB_REQUIRE(units_fit(s, vec));
  MMB_REQUIRE(!s_half || s.N <= kMaxGridX);  // split_rows: a workgroup per row
  s.s_half = 0;  // fp32 sums; split_rows makes them fp16 hi | lo afterwards
  int rc = dispatch3(vec.t, vec.a, vec.v, [&](auto vt, auto va, auto vv) {
    return launch_stream<true, vt.value ? 4 : 1, va.value ? 4 : 1, vv.value ? 4 : 1, FE, TE>(s, stream, &parts);
  });
  rc = reduce_colmax(rc, s, parts, colmax, stream);
  if (rc != MMB_OK || !s_half) return rc;
  return split_rows(s, stream);
}

// mmb_sif_wavg's launch on a table of type TE, after its checks: the wave
// kernel (`wave`: at most 64 tokens and 512 columns in 4-value units `v4`,
// 16-byte aligned outputs), else the workgroup kernel.
template <class TE>
static int sif_route(const StreamArgs& a, bool v4, bool wave, hipStream_t stream) {
  if (wave) {
    return a.D <= 256 ? launch_wave<false, 1, 1, 1, float, TE>(a, stream)
                      : launch_wave<false, 2, 1, 1, float, TE>(a, stream);
  }
  return v4 ? launch_stream<false, 4, 1, 1, float, TE>(a, stream)
            : launch_stream<false, 1, 1, 1, float, TE>(a, stream);
}

#pragma GCC visibility push(hidden)
// the routes on a 16-bit table, each instantiated in its own source
// (sif_tab_f16_kernels.hip, sif_tab_bf16_kernels.hip); frame_type is validated
// by the caller
int sif_route_f16(const StreamArgs& a, bool v4, bool wave, hipStream_t stream);
int sif_route_bf16(const StreamArgs& a, bool v4, bool wave, hipStream_t stream);
int stream_route_f16(StreamArgs& s, int frame_type, uint32_t* colmax, hipStream_t stream);
int stream_route_bf16(StreamArgs& s, int frame_type, uint32_t* colmax, hipStream_t stream);
#pragma GCC visibility pop

// stream_route on a table of type TE for frames of storage type frame_type
template <class TE>
static int stream_route_frames(StreamArgs& s, int frame_type, uint32_t* colmax, hipStream_t stream) {
  return frame_type == MMB_FRAMES_F32   ? stream_route<float, TE>(s, colmax, stream)
         : frame_type == MMB_FRAMES_F16 ? stream_route<f16_t, TE>(s, colmax, stream)
                                        : stream_route<bf16_t, TE>(s, colmax, stream);
}

}  // namespace mmb
