// The split stream for a few long rows as templates -- utt_split_part_kernel
// and utt_split_finish_kernel -- with their plan and their launcher.  Three
// sources instantiate them, one per word-table element type TE:
// sif_kernels.hip every f32-table kernel (mmb_mm2_stream_split,
// mmb_mm2_stream_split_ft), split_tab_f16_kernels.hip and
// split_tab_bf16_kernels.hip the kernels of a 16-bit table
// (mmb_mm2_stream_split_tt).  A kernel is in exactly one code object: an
// instantiation's TE names its source.  Included by those three only.
#pragma once
#include "mmb_stream.h"

namespace mmb {

// ---------------------------------------------------------------------------
// Few long rows split over workgroups (r06; POM's splits: 100 / 203
// transcripts of 1089 / 1357 aligned tokens).  One workgroup per utterance
// (utt_stream_kernel) puts 100 / 203 workgroups on 256 CUs, each a
// 1,089-1,357-frame chain: 0.21 / 0.42 of 8 TB/s.  Here every utterance is
// cut into P ranges of Lc tokens / frames and each range has a text and a
// frame workgroup, in ONE launch: the text workgroups (blocks [0, N Pt):
// token staging, the kept rows' gather, the counts) first, then the frame
// workgroups (one modality each, audio then visual: pure streams, no
// staging, no barrier before their reduction), each writing PARTIAL sums; utt_split_finish_kernel adds
// an utterance's partials in fixed part order and finishes the row as
// utt_stream_kernel does (x = num / count, the s row, aux, the row scale,
// the column bounds) -- writing the fp16 hi / lo planes directly, so the
// s_half path needs no split_rows pass.  Deterministic; against the
// one-workgroup kernel only the f32 order of the token and frame sums
// differs (with one range it is the same order: bit-identical).
//
// Workspace (floats): text partials [N][Pt][Wt] = [num (D) | Sx_e (D) |
// Sxx_e (D) | count_nonzero(w), sum w, row-0 tokens, their weight sum] (row
// 0 excluded from the sums, as utt_stream_kernel), then frame partials
// [N][Pf][Wf] = [Sx_a (A) | Sxx_a (A) | Sx_v (Vd) | Sxx_v (Vd)].
//
// The frame workgroups read frames of type FE (mmb_mm2_stream_split_ft): a
// 16-bit unit of 4 values is one 8-byte load, a scalar one a 2-byte load,
// widened to f32 in registers (ldv_nt) and summed by the same statements in
// the same order -- the partials, f32 in either case, are bit for bit those
// of the upcast frames, and the text workgroups and the finish kernel do not
// know the frame type.
//
// The text workgroups read table rows of type TE (mmb_mm2_stream_split_tt;
// a 16-bit table is gathered text: a.ids is set, and the dense-`emb` variant
// of text_rows is never instantiated for it): a 16-bit unit of 4 values is
// one 8-byte plain cached load, a scalar one a 2-byte load (ldv16), widened
// to f32 in registers and summed by the same statements in the same order;
// the finish kernel reads row 0 for its shortcut through table_f32<TE>.  The
// partials are f32 and bit for bit those of the upcast table, and the frame
// workgroups do not know the table type.
struct SplitPlan {
  int Pt, Lt, Pf, Lf;  // text / frame parts per utterance and their lengths
  int Wt, Wf;          // partial row strides (floats, multiples of 4)
};
// Text ranges per frame range of the automatic plan (an explicit part count
// keeps them equal) and text / frame rows unrolled per thread group (the
// sums' order does not depend on them).  Settled on POM's real splits
// ("Settled kernel constants").
constexpr int kSplitTextX = 1;
constexpr int kSplitTU = 8;
constexpr int kSplitFU = 8;
// the same for 16-bit frames: a frame row is half the bytes, so 16 rows keep
// in flight what 8 f32 rows do (tools/split_ab.py --frames16, graph-timed,
// bf16, 8 / 16 rows: valid 47.7 / 39.9 us, test 93.7 / 77.9 us; the same
// sums bit for bit)
constexpr int kSplitFU16 = 16;
inline SplitPlan split_plan_of(int t, int d, int a, int vd, int Pf, int text_x = 1) {
  SplitPlan q;
  q.Lf = (t + Pf - 1) / Pf;
  q.Pf = (t + q.Lf - 1) / q.Lf;  // no empty part
  // the text ranges are the frame ranges (over kTokChunk tokens they are
  // staged chunk by chunk): with one range the sums run in the one-workgroup
  // kernel's order.  One LDS chunk per text workgroup instead measured no
  // faster (POM valid 57.5 vs 55.3 us, r06 tools/split_ab.py)
  q.Lt = (t + q.Pf * text_x - 1) / (q.Pf * text_x);
  q.Pt = (t + q.Lt - 1) / q.Lt;
  q.Wt = (3 * d + 4 + 3) / 4 * 4;
  q.Wf = (2 * a + 2 * vd + 3) / 4 * 4;
  return q;
}

template <int VT, int VA, int VV, int FU = 16, int TU = 8, class FE = float, class TE = float>
__global__ __launch_bounds__(kNT) void utt_split_part_kernel(StreamArgs a, SplitPlan q,
                                                             float* __restrict__ part) {
  constexpr int NT = kNT;
  constexpr int kRF = NT * 4;
  constexpr int kSI = (kTokChunk + NT - 1) / NT;
  __shared__ int64_t s_off[kTokChunk];
  __shared__ float s_w[kTokChunk];
  __shared__ float s_red[4 * kRF];
  __shared__ float s_sc[4][NT / kWave];
  __shared__ int s_keep[kSI][NT / kWave];

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t ntext = a.N * q.Pt;
  if (static_cast<int64_t>(blockIdx.x) < ntext) {
    // ---- a token range: staging, the kept rows, the counts
    const int64_t i = blockIdx.x / q.Pt;
    const int p = static_cast<int>(blockIdx.x - i * q.Pt);
    const int tb = p * q.Lt, te = min(a.L, tb + q.Lt);
    const int CT = a.D / VT, RT = NT / CT;
    const int rT = tid / CT, cT = tid - rT * CT;
    const bool actT = rT < RT;
    const float* tsrc = a.ids ? a.table : a.text_dense;
    const float* esrc = a.ids ? a.table : a.emb_dense;
    const bool gather = a.ids != nullptr;
    float num[VT], sx[VT], sxx[VT];
#pragma unroll
    for (int e = 0; e < VT; ++e) num[e] = sx[e] = sxx[e] = 0.f;
    float cntp = 0.f, swp = 0.f, c0p = 0.f, w0p = 0.f;
    for (int t0 = tb; t0 < te; t0 += kTokChunk) {  // the range in LDS chunks
      const int tl = min(kTokChunk, te - t0);
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
          if (keep_k[k] && v == wave) {
            s_off[nkeep + rank_k[k]] = off_k[k];
            s_w[nkeep + rank_k[k]] = w_k[k];
          }
          nkeep += s_keep[k][v];
        }
      }
      __syncthreads();
      if (actT) {
        if constexpr (!std::is_same_v<TE, float>) {
          // (the rows of a 16-bit table: StreamArgs::table read as elements of TE)
          const TE* trow = reinterpret_cast<const TE*>(a.table);
          text_rows<true, false, VT, TU, TE>(trow, trow, s_off, s_w, nkeep, rT, RT, cT, num, sx, sxx);
        } else if (esrc != tsrc)
          text_rows<true, true, VT, TU>(tsrc, esrc, s_off, s_w, nkeep, rT, RT, cT, num, sx, sxx);
        else
          text_rows<true, false, VT, TU>(tsrc, esrc, s_off, s_w, nkeep, rT, RT, cT, num, sx, sxx);
      }
      __syncthreads();
    }
    cntp = wave_sum(cntp);
    swp = wave_sum(swp);
    c0p = wave_sum(c0p);
    w0p = wave_sum(w0p);
    if (lane == 0) {
      s_sc[0][wave] = cntp;
      s_sc[1][wave] = swp;
      s_sc[2][wave] = c0p;
      s_sc[3][wave] = w0p;
    }
    if (actT) {
#pragma unroll
      for (int e = 0; e < VT; ++e) {
        const int f = rT * a.D + cT * VT + e;
        s_red[f] = num[e];
        s_red[kRF + f] = sx[e];
        s_red[2 * kRF + f] = sxx[e];
      }
    }
    __syncthreads();
    float* prow = part + (i * q.Pt + p) * static_cast<int64_t>(q.Wt);
    for (int f = tid; f < a.D; f += NT) {  // the row slots summed in order
      float n_ = 0.f, x1 = 0.f, x2 = 0.f;
      for (int r = 0; r < RT; ++r) {
        n_ += s_red[r * a.D + f];
        x1 += s_red[kRF + r * a.D + f];
        x2 += s_red[2 * kRF + r * a.D + f];
      }
      prow[f] = n_;
      prow[a.D + f] = x1;
      prow[2 * a.D + f] = x2;
    }
    if (tid < 4) {
      float sc = 0.f;
#pragma unroll
      for (int w = 0; w < NT / kWave; ++w) sc += s_sc[tid][w];
      prow[3 * a.D + tid] = sc;
    }
    return;
  }
  // ---- a frame range of ONE modality (audio workgroups, then visual)
  const int64_t b = blockIdx.x - ntext;
  const bool vis = b >= a.N * q.Pf;
  const int64_t bm = vis ? b - a.N * q.Pf : b;
  const int64_t i = bm / q.Pf;
  const int p = static_cast<int>(bm - i * q.Pf);
  const int tb = p * q.Lf, te = min(a.L, tb + q.Lf);
  float* prow = part + ntext * q.Wt + (i * q.Pf + p) * static_cast<int64_t>(q.Wf);
  auto stream = [&](const FE* src, int F, float* out, auto vec) {
    constexpr int VF = decltype(vec)::value;
    const int CF = F / VF, RF = NT / CF;
    const int rF = tid / CF, cF = tid - rF * CF;
    float sm[VF], sq[VF];
#pragma unroll
    for (int e = 0; e < VF; ++e) sm[e] = sq[e] = 0.f;
    if (rF < RF) {
      const FE* base = src + (i * a.L) * F + cF * VF;
#pragma unroll FU
      for (int t = tb + rF; t < te; t += RF) {
        float v[VF];
        ldv_nt<VF, FE>(base + static_cast<int64_t>(t) * F, v);
#pragma unroll
        for (int e = 0; e < VF; ++e) {
          sm[e] += v[e];
          sq[e] = fmaf(v[e], v[e], sq[e]);
        }
      }
#pragma unroll
      for (int e = 0; e < VF; ++e) {
        const int f = rF * F + cF * VF + e;
        s_red[f] = sm[e];
        s_red[kRF + f] = sq[e];
      }
    }
    __syncthreads();
    for (int f = tid; f < F; f += NT) {  // the row slots summed in order
      float x1 = 0.f, x2 = 0.f;
      for (int r = 0; r < RF; ++r) {
        x1 += s_red[r * F + f];
        x2 += s_red[kRF + r * F + f];
      }
      out[f] = x1;
      out[F + f] = x2;
    }
  };
  if (vis)
    stream(frames<FE>(a.visual), a.Vd, prow + 2 * a.A, std::integral_constant<int, VV>{});
  else
    stream(frames<FE>(a.audio), a.A, prow, std::integral_constant<int, VA>{});
}

// The partials of utterance i (blockIdx.x) in part order, then the row's
// epilogue of utt_stream_kernel: row 0 once for its tokens, x, the s row
// (fp32, or the fp16 hi / lo planes of s * rs), aux, the column bounds of
// this workgroup (grid = N <= kCmaxRows rows of cmax_part).  Thread tid owns
// columns f = tid + NT j (j < kSplitJ) of [num | Sx_e | Sxx_e | frame sums]
// and walks each kind's parts in order, all kSplitJ loads of a part issued
// together (a loop over the parts per column was a chain of P dependent L2
// round trips per column).
// TE: the word table's element type (row 0 of the shortcut, table_f32<TE>).
constexpr int kSplitJ = 7;  // ceil((3 * 320 + 4 * 320) / kNT): every partial column
template <class TE = float>
__global__ __launch_bounds__(kNT) void utt_split_finish_kernel(StreamArgs a, SplitPlan q,
                                                               const float* __restrict__ part) {
  constexpr int NT = kNT;
  extern __shared__ float s_row[];  // s_half: the fp32 row before the split
  __shared__ float s_m[NT / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t i = blockIdx.x;
  const int K = 2 * (a.D + a.A + a.Vd);
  const int D3 = 3 * a.D, W = a.D + K;  // text columns; all partial columns
  const float* pt = part + i * q.Pt * static_cast<int64_t>(q.Wt);
  const float* pf = part + a.N * q.Pt * static_cast<int64_t>(q.Wt) + i * q.Pf * static_cast<int64_t>(q.Wf);
  float acc[kSplitJ], sc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < kSplitJ; ++j) acc[j] = 0.f;
#pragma unroll 2
  for (int p = 0; p < q.Pt; ++p) {
    const float* pr = pt + static_cast<int64_t>(p) * q.Wt;
    float v[kSplitJ], u[4];
#pragma unroll
    for (int j = 0; j < kSplitJ; ++j) {
      const int f = tid + NT * j;
      v[j] = f < D3 ? pr[f] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) u[c] = pr[D3 + c];  // (a broadcast: every lane the same word)
#pragma unroll
    for (int j = 0; j < kSplitJ; ++j) acc[j] += v[j];
#pragma unroll
    for (int c = 0; c < 4; ++c) sc[c] += u[c];
  }
#pragma unroll 2
  for (int p = 0; p < q.Pf; ++p) {
    const float* pr = pf + static_cast<int64_t>(p) * q.Wf - D3;
    float v[kSplitJ];
#pragma unroll
    for (int j = 0; j < kSplitJ; ++j) {
      const int f = tid + NT * j;
      v[j] = (f >= D3 && f < W) ? pr[f] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < kSplitJ; ++j) acc[j] += v[j];
  }
  const float cnt = sc[0], sw = sc[1], c0 = sc[2], w0 = sc[3];
  float cmx0 = 0.f, cmx1 = 0.f, smax = 0.f;
#pragma unroll
  for (int j = 0; j < kSplitJ; ++j) {
    const int f = tid + NT * j;
    if (f >= W) continue;
    float v = acc[j];
    if (f < a.D) {  // the weighted text sum: row 0 once for its c0 tokens (gather mode)
      const float e0 = (c0 > 0.f) ? table_f32<TE>(a.table, f) : 0.f;
      v = fmaf(w0, e0, v);
      const float xf = v / cnt;
      a.num_out[i * a.D + f] = xf;
      if (f < NT) cmx0 = bmax(cmx0, fabsf(xf)); else cmx1 = bmax(cmx1, fabsf(xf));
      continue;
    }
    const int g = f - a.D;  // s column
    if (g < 2 * a.D) {
      const float e0 = (c0 > 0.f) ? table_f32<TE>(a.table, g < a.D ? g : g - a.D) : 0.f;
      v = g < a.D ? fmaf(c0, e0, v) : fmaf(c0 * e0, e0, v);
    }
    smax = fmaxf(smax, fabsf(v));
    if (a.s_half) s_row[g] = v; else a.s_out[i * a.Kp + g] = v;
  }
  smax = wave_max(smax);
  if (lane == 0) s_m[wave] = smax;
  __syncthreads();
  float m = 0.f;
#pragma unroll
  for (int w = 0; w < NT / kWave; ++w) m = fmaxf(m, s_m[w]);
  const float rs = row_scale(m);
  if (a.s_half) {
    _Float16* hi = reinterpret_cast<_Float16*>(a.s_out) + i * 2 * static_cast<int64_t>(a.Kp);
    for (int f = tid; f < a.Kp; f += NT) {
      const float x = f < K ? s_row[f] * rs : 0.f;
      const _Float16 h = static_cast<_Float16>(x);
      hi[f] = h;
      hi[a.Kp + f] = static_cast<_Float16>(x - static_cast<float>(h));
    }
  } else {
    for (int f = K + tid; f < a.Kp; f += NT) a.s_out[i * a.Kp + f] = 0.f;
  }
  if (tid == 0) {
    if (cnt == 0.f && a.flag) atomicOr(a.flag, MMB_FLAG_ZERO_WEIGHTS);
    a.aux_out[i] = cnt;
    a.aux_out[a.N + i] = sw;
    a.aux_out[2 * a.N + i] = rs;
  }
  if (a.cmax_part) {
    float* pr = a.cmax_part + i * a.D;
    if (tid < a.D) pr[tid] = cmx0;
    if (tid + NT < a.D) pr[tid + NT] = cmx1;
  }
}

template <int VT, int VA, int VV, class FE = float, class TE = float>
static int launch_split(const StreamArgs& a, const SplitPlan& q, float* part, hipStream_t stream) {
  const int64_t grid = a.N * (q.Pt + 2 * q.Pf);
  if constexpr (std::is_same_v<FE, float>) {
    utt_split_part_kernel<VT, VA, VV, kSplitFU, kSplitTU, float, TE>
        <<<static_cast<unsigned>(grid), kNT, 0, stream>>>(a, q, part);
  } else {
    // 16-bit frames (mmb_mm2_stream_split_ft): the frame branch alone reads
    // FE; the partials are f32, so the finish kernel below does not know FE
#ifndef MMB_HOOK_SPLIT16_LAUNCH  // (tools/diag: the 16-bit frame unroll, MMB_SPLIT16_UNR)
#define MMB_HOOK_SPLIT16_LAUNCH false
#endif
    bool swept = false;  // (f32 table only)
    if constexpr (std::is_same_v<TE, float>) swept = MMB_HOOK_SPLIT16_LAUNCH;
    if (!swept) {
      utt_split_part_kernel<VT, VA, VV, kSplitFU16, kSplitTU, FE, TE>
          <<<static_cast<unsigned>(grid), kNT, 0, stream>>>(a, q, part);
    }
  }
  MMB_LAUNCH_CHECK();
  const size_t lds = a.s_half ? static_cast<size_t>(2 * (a.D + a.A + a.Vd)) * sizeof(float) : 0;
  utt_split_finish_kernel<TE><<<static_cast<unsigned>(a.N), kNT, lds, stream>>>(a, q, part);
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

// launch_split on a table of type TE for frames of storage type frame_type
// (validated by the caller), a bit of `vec` per modality: 4-value units or
// scalar loads
template <class TE>
static int split_route(const StreamArgs& s, const SplitPlan& q, const StreamVec& vec, int frame_type,
                       float* part, hipStream_t stream) {
  return dispatch3(vec.t, vec.a, vec.v, [&](auto vt, auto va, auto vv) {
    constexpr int VT = vt.value ? 4 : 1, VA = va.value ? 4 : 1, VV = vv.value ? 4 : 1;
    return frame_type == MMB_FRAMES_F32   ? launch_split<VT, VA, VV, float, TE>(s, q, part, stream)
           : frame_type == MMB_FRAMES_F16 ? launch_split<VT, VA, VV, f16_t, TE>(s, q, part, stream)
                                          : launch_split<VT, VA, VV, bf16_t, TE>(s, q, part, stream);
  });
}

#pragma GCC visibility push(hidden)
// the route on a 16-bit table, each instantiated in its own source
// (split_tab_f16_kernels.hip, split_tab_bf16_kernels.hip)
int split_route_f16(const StreamArgs& s, const SplitPlan& q, const StreamVec& vec, int frame_type, float* part,
                    hipStream_t stream);
int split_route_bf16(const StreamArgs& s, const SplitPlan& q, const StreamVec& vec, int frame_type, float* part,
                     hipStream_t stream);
#pragma GCC visibility pop

}  // namespace mmb
