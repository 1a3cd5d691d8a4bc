// The MMB2 stream and its projection in one kernel at narrow frame widths:
// utt_narrow_fused_kernel (f32, fp16 and bf16 frames), mmb_mm2_stream_project_narrow,
// mmb_mm2_stream_project_narrow_ft and mmb_mm2_stream_project_narrow_tt (a
// 16-bit word table: the same kernels, whose text comes from the cache).
#include "mmb_stream.h"

namespace mmb {

// ------------------------------------------------------------------ narrow fused (r04)
// SIF + closed-form MMB2 at narrow frame widths (MOSI: COVAREP A = 76, FACET
// Vd = 48, V = 3016) in ONE kernel: the two-kernel step wrote the frame sums
// s (fp16 hi | lo of 2 (D + A + Vd) = 848 sums, 3.4 KB per utterance) to HBM
// and read them back in a K = 864 projection.  Here the text sums never
// form: the text rows of Wm are applied per vocabulary row (the text cache,
// mmb_mm2_text_cache: P[v] = E_v Wm_t1 + E_v^2 Wm_t2, column D the total
// weight), so an utterance's text term is sum_t P[id_t], gathered beside its
// table rows, and only the audio / visual sums [Sa | Saa | Sv | Svv] (K =
// kq(A) + kq(Vd) <= 256) go through the f16 x3 MFMA -- in the same launch.
//
// One persistent 512-thread workgroup per CU, batches of 32 utterances:
//   stream phase: every wave runs 4 utterances as utt_narrow_kernel does
//     (packed frame instructions issued first, ids one utterance ahead,
//     buffer-descriptor loads), its text rows from LDS for the 32 words of
//     smallest weight (the most frequent; ~58 % of Zipf(1.1) tokens at
//     V = 3016) and from L2 otherwise; it writes x (the a2 row, bit-identical
//     to the narrow kernel's: the same f32 operations in the same order),
//     aux, its column bounds, and into LDS the row's text term T (x-sum + sum
//     of P) and its audio / visual sums as fp16 hi | lo (power-of-2 row scale);
//   MFMA phase (after a barrier): [32 x K] x [K x 320] as fp16 x3 products
//     (v_mfma_f32_16x16x32_f16, the fused kernel's projector arithmetic; B =
//     the audio / visual chunks of the piece-ordered weight image, from L2);
//   epilogue: y = acc * scales + T + c0 into the T rows (LDS), then per row
//     the division by the total weight (column D) and the L2 norm, the MMB2
//     row written with 16-byte stores.
// LDS: hot E rows 38.4 KB + hot P rows 38.9 KB + T 38.9 KB + A 32 KB.
constexpr int kNFUnr = 2;  // cold words per load group
constexpr int kNFHU = 1;   // hot words per LDS group
constexpr int kNFGA = 7;   // audio / visual frame loads issued with the text loads
constexpr int kNFGV = 4;
constexpr int kNFWaves = 8;  // 2 per SIMD, 32-row batches
constexpr int kNFThreads = kNFWaves * kWave;
constexpr int kNFRpw = 4;                   // utterances per wave and batch (at most)
constexpr int kNFRows = kNFWaves * kNFRpw;     // rows of a batch (at most)
constexpr int kNFRT = (kNFRows + 15) / 16;     // MFMA row tiles
constexpr int kNFHot = kTextHot;            // the text cache's layout (mmb_common.h)
constexpr int kNFLdp = kTextLdp;            // T row stride, floats: y columns and the total
constexpr int kNFLdq = kTextLdq;            // text cache row: E | P, floats
constexpr int kNFHotRow = 604;              // a hot word's E | P row in LDS (151 float4 units)
constexpr int kNFK = 256;                   // K of the audio / visual GEMM (max)
constexpr int kNFLdw = 320;                 // projection columns
constexpr int kNFCT = kNFLdp / 16;          // 16-column tiles of y and the total (19)
constexpr size_t kNFLdsRows = sizeof(float) * (kNFHot * kNFHotRow + kNFRows * kNFLdp) +
                              sizeof(_Float16) * kNFRows * 2 * kNFK + sizeof(float) * 3 * kNFRows;
static_assert(kNFLdsRows % 16 == 0, "the frame-slot scratch is float4-aligned");
// + 1 KB per wave for the frame-slot sums
constexpr size_t kNFLds = kNFLdsRows + 16 * kWave * kNFWaves + 16;  // + team counters

struct NarrowFusedArgs {
  StreamArgs s;        // ids, table, V, wtab, audio, visual, N, L, D, A, Vd, num_out, aux_out, flag, cmax_part
  const float* ptab;   // [V][kNFLdq]: E | P rows
  const int32_t* hot_slot1;  // [V]
  const int32_t* hot_ids;    // [n_hot]
  int n_hot;
  const _Float16* img;       // piece-ordered weight image (mmb_mm2_split_pieces)
  const float* col_inv;
  const float* c0;
  float* out;                // MMB2 rows [N][D]
  int cb_av;                 // first audio chunk of the image (kq(D) / 32)
  int kq_a, kq_v;            // K rows of the audio / visual pieces (multiples of 32)
  int rpw;                   // utterances per wave and batch (4; 1 or 2 for small N)
  int64_t nb;                // batches of 8 rpw rows (teams: of 4 rpw rows)
  int team_lag;              // teams: team 1 starts after team 0's first stream phase
};

// TM (teams): the workgroup's two halves (waves 0-3 and 4-7, one wave of
// each per SIMD) run batches of 4 rpw rows on their own LDS halves with
// their own (LDS counter) barriers, so that one team's batch GEMM and
// epilogue can run beside the other team's stream phase.
// FE: the audio / visual frames' element type (mmb_stream.h).  On 16-bit rows
// a frame instruction keeps its lane mapping (lane = f U + c: row f of the
// group, column unit c of 4 values) and loads the unit as 8 bytes instead of
// 16, every byte quantity scaled by sizeof(FE); the units stay packed until
// the frame is summed, and are widened (exactly) in front of the f32
// instantiation's add4 / sq4.  Nothing else depends on FE.
template <int UNR, int HU, int GA_MAX, int GV_MAX, bool TM = false, class FE = float>
__global__ __launch_bounds__(kNFThreads) __attribute__((amdgpu_waves_per_eu(kNFWaves / 4, kNFWaves / 4))) void utt_narrow_fused_kernel(
    NarrowFusedArgs f) {
  static_assert(kNFWaves == 8, "teams of 4 waves: 8-wave workgroups");
  extern __shared__ __attribute__((aligned(16))) float nf_lds[];
  float* hotEP = nf_lds;                                  // [kNFHot][kNFHotRow]: E | P
  float* sT = hotEP + kNFHot * kNFHotRow;                 // [rows][kNFLdp]
  _Float16* sA = reinterpret_cast<_Float16*>(sT + kNFRows * kNFLdp);  // [rows][2][kNFK] swizzled
  float* s_irs = reinterpret_cast<float*>(sA + kNFRows * 2 * kNFK);   // [rows] 1 / row scale
  float* s_cnt = s_irs + kNFRows;                         // [rows]
  float* s_ok = s_cnt + kNFRows;                          // [rows] 1 = a row of this batch
  float4* s_scr = reinterpret_cast<float4*>(s_ok + kNFRows);  // [waves][64] frame-slot sums
  unsigned* s_team = reinterpret_cast<unsigned*>(s_scr + kWave * kNFWaves);  // [2]

  const StreamArgs& a = f.s;
  // (holding these pointers in VGPRs instead -- fewer SGPR spills -- measured
  // slower: 4.21 vs 4.08 ms)
  float* const num_out = a.num_out;
  float* const aux_out = a.aux_out;
  float* const mmb_out = f.out;
  const int32_t* const ids_v = a.ids;
  int32_t* const flag_v = a.flag;
  const int V = static_cast<int>(a.V);  // <= 16384 (the text cache)
  constexpr int CT = 2;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int64_t wid = static_cast<int64_t>(blockIdx.x) * kNFWaves + wave;
  constexpr int kTW = TM ? 4 : kNFWaves;       // waves of a team (the workgroup: one team)
  constexpr int kTRT = TM ? 1 : kNFRT;         // MFMA row tiles of a team's batch
  const int team = TM ? wave >> 2 : 0;
  const int wt = TM ? wave & 3 : wave;          // wave in its team
  const int r0 = TM ? 16 * team : 0;            // the team's first LDS row
  const int L = a.L, D = a.D;
  const int UT = D >> 2, UA = a.A >> 2, UV = a.Vd >> 2;
  const int PA = kWave / UA, PV = kWave / UV;
  const int GA = (L + PA - 1) / PA, GV = (L + PV - 1) / PV;

  // the hot words' E | P rows into LDS
  const int NU = 2 * (D >> 2) + 1;  // float4 units of a cache row: E (D / 4) then P (D / 4 + 1)
  for (int e = tid; e < f.n_hot * NU; e += kNFThreads) {
    const int k = e / NU, u = e - k * NU;
    *reinterpret_cast<float4*>(hotEP + k * kNFHotRow + 4 * u) =
        ld4(f.ptab + static_cast<int64_t>(f.hot_ids[k]) * kNFLdq + 4 * u);
  }

  // one descriptor over the whole text cache: E | P rows | hot slots | hot
  // ids | the weights (mm2_kernels.hip); offset `cbytes` is past its end and
  // reads 0
  const int hbase = V * kNFLdq * 4;              // hot_slot1
  const int wbase = hbase + V * 4 + 4 * kNFHot;  // the weight copy
  const int cbytes = wbase + V * 4;
  const auto prsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(f.ptab), 0, cbytes, 0x00020000);
  // a token's E | P row: unit u = lane + 64 c of slot c (E units [0, UT),
  // P units [UT, NU)); slot 0 is all E, slot 1 E on lanes 64 + lane < UT and
  // P above, slot 2 P or nothing
  constexpr int CQ = 3;
  int vu[CQ], hu[CQ];
#pragma unroll
  for (int c = 0; c < CQ; ++c) {
    const int u = lane + kWave * c;
    vu[c] = u < NU ? 16 * u : cbytes;  // past the cache: reads 0
    hu[c] = 4 * min(u, NU - 1);
  }
  const bool e1 = kWave + lane < UT;  // slot 1 holds an E unit on this lane
  constexpr int kFB = static_cast<int>(sizeof(FE));  // bytes of a frame value
  const int voa = ((lane / UA) * a.A + 4 * (lane % UA)) * kFB;
  const int vov = ((lane / UV) * a.Vd + 4 * (lane % UV)) * kFB;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 cmx[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) cmx[c] = z4;

  // utterance u of this wave in batch j: row 8 rpw (blockIdx.x + gridDim.x j) + rpw wave + u
  // (teams: 4 rpw (tg + ntg j) + rpw wt + u, team tg = 2 blockIdx.x + team of ntg)
  const int rpw = f.rpw;
  const int nbr = kTW * rpw;  // rows of a batch
  const int nrt = (nbr + 15) / 16;  // MFMA row tiles holding them
  // 32-bit rows and batches (N < 2^31: the launcher checks), 64-bit offsets
  const int N = static_cast<int>(a.N), nb = static_cast<int>(f.nb);
  const int tg = TM ? 2 * static_cast<int>(blockIdx.x) + team : static_cast<int>(blockIdx.x);
  const int ntg = TM ? 2 * static_cast<int>(gridDim.x) : static_cast<int>(gridDim.x);
  auto row_of = [&](int j, int u) -> int { return nbr * (tg + ntg * j) + rpw * wt + u; };
  // the batch barrier: the workgroup's, or the team's 4 waves' (an LDS
  // arrival counter; every wave of a team runs the same batches)
  unsigned bar_target = 0;
  auto bar_batch = [&]() {
    if constexpr (!TM) {
      __syncthreads();
    } else {
      bar_target += kTW;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      if (lane == 0) {
        __hip_atomic_fetch_add(&s_team[team], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        while (__hip_atomic_load(&s_team[team], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < bar_target)
          __builtin_amdgcn_s_sleep(1);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
  };
  auto ld_id = [&](int i) -> int {
    return (i < N && lane < L) ? ids_v[static_cast<int64_t>(i) * L + lane] : -1;
  };
  auto resolve = [&](int raw, int& rid, float& w, int& hs) {
    rid = -1;
    w = 0.f;
    hs = 0;
    if (lane < L) {
      int id = raw;
      const bool in = id >= 0 && id < V;
      w = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(prsrc, in ? wbase + id * 4 : cbytes, 0, 0));
      if (id < 0) id += V;
      if (id < 0 || id >= V) {
        if (flag_v) atomicOr(flag_v, MMB_FLAG_ID_RANGE);
      } else {
        rid = id;
        hs = __builtin_amdgcn_raw_buffer_load_b32(prsrc, hbase + rid * 4, 0, 0);
      }
    }
  };

  // MFMA phase: this wave's column tiles wave, wave + 8, wave + 16 (< 20);
  // lane (q, g) holds row / column q, K group g of a 16 x 32 fragment
  const int q = lane & 15, g = lane >> 4;
  constexpr int CH = 2 * kNFLdw * 32, PL = kNFLdw * 32;  // image chunk / plane (halves)
  constexpr int kMaxT = (kNFCT + kTW - 1) / kTW;  // 3 (8 waves), 2 (12) or 5 (teams)
  const int nch = (f.kq_a + f.kq_v) / 32;
  const auto brsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(f.img), 0,
                                                       (f.cb_av + nch) * CH * 2, 0x00020000);
  int boff[kMaxT];
#pragma unroll
  for (int tt = 0; tt < kMaxT; ++tt) {
    const int col = 16 * min(wt + kTW * tt, kNFCT - 1) + q;
    boff[tt] = col * 32 + ((g ^ x3_swz(col)) << 3);
  }
  static_assert(kMaxT == 2 || kMaxT == 3 || kMaxT == 5, "column tiles per wave");
  const int ntt = wt + kTW * (kMaxT - 1) < kNFCT ? kMaxT : kMaxT - 1;  // this wave's column tiles
  float cinv[kMaxT], cc0[kMaxT];  // the tiles' column scales and c0
#pragma unroll
  for (int tt = 0; tt < kMaxT; ++tt) {
    const int col = 16 * min(wt + kTW * tt, kNFCT - 1) + q;
    const bool held = tt < ntt && col < kNFLdp;
    cinv[tt] = held ? f.col_inv[col] : 0.f;
    cc0[tt] = held ? f.c0[col] : 0.f;
  }
  auto ld_b = [&](int c, half8 (&bh)[kMaxT], half8 (&bl)[kMaxT]) {
    const int so = (f.cb_av + c) * CH * 2;
#pragma unroll
    for (int tt = 0; tt < kMaxT; ++tt) {
      if (tt < ntt) {
        bh[tt] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(brsrc, boff[tt] * 2, so, 0));
        bl[tt] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(brsrc, (boff[tt] + PL) * 2, so, 0));
      }
    }
  };

  auto frame_rsrc = [&](int i, const void* base, int W) {
    const bool live = i < N;
    const int64_t ic = live ? i : 0;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<FE*>(frames<FE>(base) + ic * L * W), 0,
                                             live ? L * W * kFB : 0, 0x00020000);
  };
  auto take = [](uint64_t& m) -> int {  // next token of a (uniform) mask, -1 = none
    const int t = m ? __builtin_ctzll(m) : -1;
    m &= m - 1;
    return t;
  };

  // the A rows' pads (K past each piece) stay zero: zeroed once here
  for (int e = tid; e < kNFRows * 2 * kNFK / 8; e += kNFThreads)
    reinterpret_cast<float4*>(sA)[e] = z4;
  if (TM && tid < 2) s_team[tid] = 0u;
  int rid_n, hs_n, raw = -1;  // the next utterance's ids, weights, hot slots
  float w_n;
  resolve(ld_id(row_of(0, 0)), rid_n, w_n, hs_n);
  __syncthreads();  // hot rows in LDS
  if (TM && team == 1 && f.team_lag && tg < nb) {
    // team 1 starts once team 0 (which has a batch if team 1 has) is past its
    // first stream phase: the teams' phases start out of step
    if (lane == 0)
      while (__hip_atomic_load(&s_team[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < static_cast<unsigned>(kTW))
        __builtin_amdgcn_s_sleep(2);
    __builtin_amdgcn_wave_barrier();
  }
  for (int j = 0; j < nb; j += 1) {
    if (tg + ntg * j >= nb) break;
    // ------------------------------------------------------------ stream phase
    for (int u = 0; u < rpw; ++u) {
      const int i = row_of(j, u);
      const int r = r0 + rpw * wt + u;  // LDS row
      const bool live = i < N;
      const int rid = rid_n, hs = hs_n;
      const float w = w_n;
      raw = ld_id(u + 1 < rpw ? row_of(j, u + 1) : row_of(j + 1, 0));
      const auto arsrc = frame_rsrc(i, a.audio, a.A);
      const auto vrsrc = frame_rsrc(i, a.visual, a.Vd);
      float4 sa = z4, saa = z4, sv = z4, svv = z4;
      auto frames = [&](auto gmax, auto rsrc, int vo, int W, int U, int P, int g0, float4& s1, float4& s2) {
        constexpr int GM = decltype(gmax)::value;
        // a group's units as loaded: a float4, or four 16-bit values packed in 8 bytes
        std::conditional_t<kFB == 4, float4, u2> v[GM > 0 ? GM : 1];
#pragma unroll
        for (int g = 0; g < GM; ++g) {
          if constexpr (kFB == 4)
            v[g] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, vo, (g0 + g) * P * W * 4, 2));
          else
            v[g] = __builtin_bit_cast(u2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, vo, (g0 + g) * P * W * kFB, 2));
        }
        const bool mine = lane < P * U;
        return [=, &s1, &s2]() {
#pragma unroll
          for (int g = 0; g < GM; ++g) {
            if (mine) {
              if constexpr (kFB == 4) {
                add4(s1, v[g]);
                sq4(s2, v[g]);
              } else {
                const float4 x = frame_f32x4<FE>(v[g]);
                add4(s1, x);
                sq4(s2, x);
              }
            }
          }
        };
      };
      using GAc = std::integral_constant<int, GA_MAX>;
      using GVc = std::integral_constant<int, GV_MAX>;
      auto acc_a = frames(GAc{}, arsrc, voa, a.A, UA, PA, 0, sa, saa);
      auto acc_v = frames(GVc{}, vrsrc, vov, a.Vd, UV, PV, 0, sv, svv);

      // text: the x sums (w E) and the P rows of the text term over the
      // utterance's valid tokens -- hot words (LDS) while the first group of
      // cold words (global loads) is in flight, then the cold groups.  The
      // order (hot tokens, then cold, each by position) is not
      // utt_narrow_kernel's: x agrees with it to f32 rounding.
      float4 ac[CQ];  // slot sums: w E units, then P units (e1: slot 1 mixes them)
#pragma unroll
      for (int c = 0; c < CQ; ++c) ac[c] = z4;
      const bool tok = lane < L && rid >= 0;
      uint64_t cold = __builtin_amdgcn_ballot_w64(tok && hs == 0);
      uint64_t hot = __builtin_amdgcn_ballot_w64(tok && hs > 0);
      auto cold_row = [&](int t, float4 (&v)[CQ]) {
        const int rr = t >= 0 ? __builtin_amdgcn_readlane(rid, t) : -1;
        const int so = rr >= 0 ? rr * kNFLdq * 4 : cbytes;  // none: out of range, reads 0
#pragma unroll
        for (int c = 0; c < CQ; ++c)
          v[c] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(prsrc, vu[c], so, 0));
      };
      auto accum = [&](int t, const float4 (&v)[CQ]) {
        const float wt = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), t));
        fma4(ac[0], wt, v[0]);
        fma4(ac[1], e1 ? wt : 1.f, v[1]);  // 1 * p + s == p + s exactly
        add4(ac[2], v[2]);
      };
      {
        float4 vc[UNR][CQ];
        int tq[UNR];
#pragma unroll
        for (int q = 0; q < UNR; ++q) {
          tq[q] = take(cold);
          cold_row(tq[q], vc[q]);
        }
        while (hot) {
          float4 vh[HU][CQ];
          int th[HU];
#pragma unroll
          for (int q = 0; q < HU; ++q) {
            th[q] = take(hot);
            const int hh = th[q] >= 0 ? __builtin_amdgcn_readlane(hs, th[q]) - 1 : 0;
            const float* pr = hotEP + hh * kNFHotRow;
#pragma unroll
            for (int c = 0; c < CQ; ++c) vh[q][c] = *reinterpret_cast<const float4*>(pr + hu[c]);
          }
#pragma unroll
          for (int q = 0; q < HU; ++q)
            if (th[q] >= 0) accum(th[q], vh[q]);
        }
        acc_a();
        acc_v();
        for (;;) {
#pragma unroll
          for (int q = 0; q < UNR; ++q)
            if (tq[q] >= 0) accum(tq[q], vc[q]);
          if (!cold) break;
#pragma unroll
          for (int q = 0; q < UNR; ++q) {
            tq[q] = take(cold);
            cold_row(tq[q], vc[q]);
          }
        }
      }
      const float cnt = static_cast<float>(__builtin_popcountll(__builtin_amdgcn_ballot_w64(w != 0.f)));
      const float sw = wave_sum_dpp_f32(w);  // (DPP row sums: another order than wave_sum's)
      if (live && lane == 0 && cnt == 0.f && flag_v) atomicOr(flag_v, MMB_FLAG_ZERO_WEIGHTS);
      for (int g0 = GA_MAX; g0 < GA; g0 += GA_MAX) frames(GAc{}, arsrc, voa, a.A, UA, PA, g0, sa, saa)();
      for (int g0 = GV_MAX; g0 < GV; g0 += GV_MAX) frames(GVc{}, vrsrc, vov, a.Vd, UV, PV, g0, sv, svv)();
      // The A row [Sa | Saa | 0 | Sv | Svv] (K = 4 lane .. 4 lane + 3 on lane
      // `lane`): each frame sum's P row slots added up through this wave's 1
      // KB of LDS (one write, P reads by the lanes holding that piece; slot 0
      // first, as the shuffle reduction of utt_narrow_kernel); pads 0
      float4* scr = s_scr + wave * kWave;
      float4 av = z4;
      auto gather = [&](const float4& acc, int U, int P, int u0) {
        __builtin_amdgcn_wave_barrier();  // the previous piece's reads are issued
        scr[lane] = acc;
        __builtin_amdgcn_wave_barrier();
        const int l = lane - u0;
        if (l >= 0 && l < U) {
          av = scr[l];
          for (int q = 1; q < P; ++q) add4(av, scr[l + q * U]);
        }
      };
      gather(sa, UA, PA, 0);
      gather(saa, UA, PA, UA);
      gather(sv, UV, PV, f.kq_a >> 2);
      gather(svv, UV, PV, (f.kq_a >> 2) + UV);
      __builtin_amdgcn_wave_barrier();  // (12 waves: the T row is written below)
      const float rsc = row_scale(wave_max_dpp_f32(amax4(av)));
      resolve(raw, rid_n, w_n, hs_n);  // the next utterance's
      // x (the a2 row), column bounds, aux; the text term T into LDS
      const float rc = 1.f / cnt;
      float* trow = sT + r * kNFLdp;
      // T = sum w E + sum P: the P units into the T row first (unit UT, the
      // total weight column, plus the weight sum; pads 0), then each E unit's
      // lane adds its sum there
#pragma unroll
      for (int c = 1; c < CQ; ++c) {
        const int p = lane + kWave * c - UT;  // P unit of this slot
        if (p >= 0 && p <= UT) {
          float4 tv = ac[c];
          if (p == UT) tv.x += sw;
          *reinterpret_cast<float4*>(trow + 4 * p) = tv;
        }
      }
      if (lane > UT && lane < kNFLdp / 4) *reinterpret_cast<float4*>(trow + 4 * lane) = z4;
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int uu = lane + kWave * c;
        if (uu < UT) {
          const float4 xr = make_float4(ac[c].x * rc, ac[c].y * rc, ac[c].z * rc, ac[c].w * rc);
          if (live) {
            st4(num_out + static_cast<int64_t>(i) * D + 4 * uu, xr);
            cmx[c] = bmax4(cmx[c], xr);
          }
          float4 tv = *reinterpret_cast<const float4*>(trow + 4 * uu);
          add4(tv, ac[c]);
          *reinterpret_cast<float4*>(trow + 4 * uu) = tv;
        }
      }
      // the A row as fp16 hi | lo, row-scaled, swizzled per row
      {
        _Float16* arow = sA + r * 2 * kNFK;
        const int q = r & 15;
        auto put = [&](int k, float4 v) {  // 4 consecutive K at k (k % 4 == 0)
          const int grp = k >> 3, o = ((grp ^ q) << 3) + (k & 7);
          split_store4(arow + o, arow + kNFK + o, v, rsc);
        };
        put(4 * lane, av);  // the whole row, pads included
      }
      if (lane == 0) {
        s_irs[r] = 1.f / rsc;
        s_cnt[r] = cnt;
        s_ok[r] = live ? 1.f : 0.f;
        if (live) {
          aux_out[i] = cnt;
          aux_out[static_cast<int64_t>(N) + i] = sw;
          aux_out[2 * static_cast<int64_t>(N) + i] = rsc;
        }
      }
    }
    // the first image chunk's B fragments load across the barrier
    half8 bh[kMaxT], bl[kMaxT];
    ld_b(0, bh, bl);
    bar_batch();
    // ------------------------------------------------------------ MFMA phase
    {
      f32x4 acc[kTRT][kMaxT];
#pragma unroll
      for (int rt = 0; rt < kTRT; ++rt)
#pragma unroll
        for (int tt = 0; tt < kMaxT; ++tt) acc[rt][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int c = 0; c < nch; ++c) {
        half8 nh[kMaxT], nl[kMaxT];  // chunk c + 1, in flight during chunk c
        if (c + 1 < nch) ld_b(c + 1, nh, nl);
#pragma unroll
        for (int rt = 0; rt < kTRT; ++rt) {
          if (rt < nrt) {
            // (36-row batches: rows past the last are clamped, their results unused)
            const int rr = r0 + (kNFRows % 16 == 0 ? 16 * rt + q : min(16 * rt + q, kNFRows - 1));
            const int o = (((4 * c + g) ^ q) << 3);
            const half8 ah = *reinterpret_cast<const half8*>(sA + rr * 2 * kNFK + o);
            const half8 al = *reinterpret_cast<const half8*>(sA + rr * 2 * kNFK + kNFK + o);
#pragma unroll
            for (int tt = 0; tt < kMaxT; ++tt) {
              if (tt < ntt) {
                acc[rt][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[tt], acc[rt][tt], 0, 0, 0);
                acc[rt][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[tt], acc[rt][tt], 0, 0, 0);
                acc[rt][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[tt], acc[rt][tt], 0, 0, 0);
              }
            }
          }
        }
#pragma unroll
        for (int tt = 0; tt < kMaxT; ++tt) {
          bh[tt] = nh[tt];
          bl[tt] = nl[tt];
        }
      }
      // y = acc * (col scale * row scale) + T + c0, in place in the T rows
      // (lane value (rt, tt, jj): row 16 rt + 4 g + jj, column 16 ct + q).
      // Every T value and row scale is read before any update is written: in
      // place, each read-modify-write waited for the previous one's store
      // (the compiler cannot tell the rows apart)
      static_assert(kNFCT * 16 <= kNFLdp, "the column tiles lie inside the T rows");
      float irs[kTRT][4], tv[kMaxT][kTRT][4];
#pragma unroll
      for (int rt = 0; rt < kTRT; ++rt)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) irs[rt][jj] = s_irs[r0 + min(16 * rt + 4 * g + jj, kNFRows - 1)];
#pragma unroll
      for (int tt = 0; tt < kMaxT; ++tt) {
        const int col = 16 * min(wt + kTW * tt, kNFCT - 1) + q;
#pragma unroll
        for (int rt = 0; rt < kTRT; ++rt)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)
            tv[tt][rt][jj] = sT[(r0 + min(16 * rt + 4 * g + jj, kNFRows - 1)) * kNFLdp + col];
      }
#pragma unroll
      for (int tt = 0; tt < kMaxT; ++tt) {
        if (tt < ntt) {
          const int col = 16 * (wt + kTW * tt) + q;
          const float ci = cinv[tt], cc = cc0[tt];
#pragma unroll
          for (int rt = 0; rt < kTRT; ++rt)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
              const int rr = 16 * rt + 4 * g + jj;
              if (kNFRows % 16 == 0 ? rt < nrt : rr < nbr)
                sT[(r0 + rr) * kNFLdp + col] = acc[rt][tt][jj] * (ci * irs[rt][jj]) + tv[tt][rt][jj] + cc;
            }
        }
      }
    }
    bar_batch();
    // ------------------------------------------------------------ epilogue
    // wave w finishes rows rpw w .. rpw w + rpw - 1: / total (column D), L2 norm, store
    for (int u = 0; u < rpw; ++u) {
      const int r = r0 + rpw * wt + u;
      const int i = row_of(j, u);
      const float* trow = sT + r * kNFLdp;
      const float rt = __builtin_amdgcn_rcpf(trow[D]);  // v_rcp_f32 (1 ulp): the MMB2 bar is 2e-6
      float4 y[CT];
      float ss = 0.f;
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        const int uu = lane + kWave * c;
        y[c] = *reinterpret_cast<const float4*>(trow + 4 * min(uu, UT - 1));
        y[c] = make_float4(y[c].x * rt, y[c].y * rt, y[c].z * rt, y[c].w * rt);
        if (uu < UT) ss += y[c].x * y[c].x + y[c].y * y[c].y + y[c].z * y[c].z + y[c].w * y[c].w;
      }
      const float inv = __builtin_amdgcn_rsqf(wave_sum_dpp_f32(ss));  // v_rsq_f32 (1 ulp)
      if (s_ok[r] != 0.f) {
#pragma unroll
        for (int c = 0; c < CT; ++c) {
          const int uu = lane + kWave * c;
          if (uu < UT) st4(mmb_out + static_cast<int64_t>(i) * D + 4 * uu, make_float4(y[c].x * inv, y[c].y * inv, y[c].z * inv, y[c].w * inv));
        }
      }
    }
    bar_batch();  // the T / A rows are rewritten by the next batch
  }
  if (a.cmax_part) {
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const int uu = lane + kWave * c;
      if (uu < UT) st4(a.cmax_part + wid * D + 4 * uu, cmx[c]);
    }
  }
}

// the product launch on 16-bit frames of type FE (mmb_mm2_stream_project_narrow_ft)
template <class FE>
static void launch_narrow_fused16(const NarrowFusedArgs& f, int64_t grid, hipStream_t stream) {
  allow_dynamic_lds<&utt_narrow_fused_kernel<kNFUnr, kNFHU, kNFGA, kNFGV, false, FE>>(kNFLds);
  utt_narrow_fused_kernel<kNFUnr, kNFHU, kNFGA, kNFGV, false, FE>
      <<<static_cast<unsigned>(grid), kNFThreads, kNFLds, stream>>>(f);
}

// the narrow fused kernel's shapes: gathered ids, a weight table, 256 < d <
// 304 (d % 4), frame rows of 4..128 floats (two or more per instruction,
// A % 4 == Vd % 4 == 0), kq(A) + kq(Vd) <= 256, t <= 64, V <= 16384 (the
// text cache)
}  // namespace mmb

using namespace mmb;

extern "C" int mmb_mm2_stream_project_narrow_supported(int t, int d, int a_, int vd, int64_t v) {
  const int kq = piece_k(a_) + piece_k(vd);
  return t > 0 && t <= kWave && d > 256 && d < kNFLdp && d % 4 == 0 && a_ >= 4 && vd >= 4 &&
         a_ <= 128 && vd <= 128 && a_ % 4 == 0 && vd % 4 == 0 && kq <= kNFK && v > 0 && v <= 16384 &&
         v * (kNFLdq + 2) * 4 + 4 * kNFHot < (int64_t{1} << 31) && static_cast<int64_t>(t) * (a_ > vd ? a_ : vd) * 4 < (int64_t{1} << 31);
}

// mmb_mm2_stream_project_narrow for a word table of storage type table_type
// and frames of storage type frame_type (MMB_TABLE_* / MMB_FRAMES_*, validated
// by the caller): the checks, the text cache, the rows per wave, the grid and
// the column bounds are the same for all.  The kernel takes its text from the
// cache (ptab: the E | P rows, f32 whatever the table's type) and never reads
// `table`, so the table's type picks no instantiation: it only sets what the
// pointer is held to.
static int narrow_project(int table_type, int frame_type, const int32_t* ids, const void* table_, int64_t v,
                          const float* wtab32, const void* text_cache, const void* audio,
                          const void* visual, int64_t n, int t, int d, int a_, int vd, const void* wpieces,
                          const float* c0, float* num_out, float* aux_out, float* mmb2_out, int32_t* flag,
                          uint32_t* colmax, void* colmax_ws, hipStream_t stream) {
  NarrowFusedArgs f{};
  const float* table = static_cast<const float*>(table_);
  // gathered text with the weight table only; the sums stay on chip
  MMB_REQUIRE(ids && wtab32);
  if (const int rc = stream_args(&f.s, ids, table, v, wtab32, nullptr, nullptr, nullptr, audio, visual, n, t, d,
                                 a_, vd, num_out, nullptr, 1, aux_out, flag, colmax, colmax_ws))
    return rc;
  MMB_REQUIRE(n < (int64_t{1} << 31) - kNFRows && mmb_mm2_stream_project_narrow_supported(t, d, a_, vd, v));
  MMB_REQUIRE(text_cache && mmb2_out && wpieces && c0);
  // (stream_vec's width % 4 asks nothing new: the predicate above has it)
  StreamVec vec = stream_vec(f.s, frame_bytes(frame_type));
  // a 16-bit table (not read by the launch) is held to its element's alignment
  if (table_type != MMB_TABLE_F32) vec.t = (reinterpret_cast<uintptr_t>(table) & 1) == 0;
  MMB_REQUIRE(vec.t && vec.a && vec.v && aligned16(text_cache) && aligned16(num_out) && aligned16(mmb2_out) &&
              aligned16(wpieces));
  if (n == 0) return empty_call(colmax, d, stream);
  f.ptab = static_cast<const float*>(text_cache);
  f.hot_slot1 = reinterpret_cast<const int32_t*>(f.ptab + static_cast<size_t>(v) * kNFLdq);
  f.hot_ids = f.hot_slot1 + v;
  f.n_hot = static_cast<int>(v < kNFHot ? v : kNFHot);
  const int kq_t = piece_k(d);
  f.kq_a = piece_k(a_);
  f.kq_v = piece_k(vd);
  f.cb_av = kq_t / 32;
  f.img = static_cast<const _Float16*>(wpieces);
  f.col_inv = reinterpret_cast<const float*>(f.img + 2 * static_cast<size_t>(kNFLdw) * (kq_t + f.kq_a + f.kq_v));
  f.c0 = c0;
  f.out = mmb2_out;
  // 4 utterances per wave (32-row batches) once that fills every CU; small N
  // (dataset splits) fewer per wave: more workgroups, a shorter chain each
  const int64_t cus = stream_cu_count(stream);
  f.rpw = kNFRpw;
  while (f.rpw > 1 && ceil_div(n, static_cast<int64_t>(kNFWaves) * f.rpw) < cus) --f.rpw;
#ifndef MMB_HOOK_NF_TEAMS  // (tools/diag: MMB_NF_TEAMS)
#define MMB_HOOK_NF_TEAMS 0
#endif
  // 1: two teams of 4 waves per workgroup, 2: the same, team 1 starting a phase later (f32 frames)
  int teams = frame_type == MMB_FRAMES_F32 ? MMB_HOOK_NF_TEAMS : 0;
  f.team_lag = teams == 2 ? 1 : 0;
  // batches: of 8 rpw rows, or of 4 rpw rows per team (two per workgroup)
  f.nb = ceil_div(n, static_cast<int64_t>(teams ? kNFWaves / 2 : kNFWaves) * f.rpw);
  if (frame_type == MMB_FRAMES_F32) {
    allow_dynamic_lds<&utt_narrow_fused_kernel<kNFUnr, kNFHU, kNFGA, kNFGV>>(kNFLds);
#ifdef MMB_HOOK_NF_TEAMS_ATTR
    MMB_HOOK_NF_TEAMS_ATTR;
#endif
  }
  // one workgroup per CU; the bounds: a partial row per wave
  int64_t grid = cus;
  if (colmax && grid > kCmaxRows / kNFWaves) grid = kCmaxRows / kNFWaves;
  if (grid > (teams ? ceil_div(f.nb, int64_t{2}) : f.nb)) grid = teams ? ceil_div(f.nb, int64_t{2}) : f.nb;
#ifndef MMB_HOOK_NF_TEAMS_LAUNCH
#define MMB_HOOK_NF_TEAMS_LAUNCH false
#endif
  if (frame_type == MMB_FRAMES_F16) {
    launch_narrow_fused16<f16_t>(f, grid, stream);
  } else if (frame_type == MMB_FRAMES_BF16) {
    launch_narrow_fused16<bf16_t>(f, grid, stream);
  } else if (!(MMB_HOOK_NF_TEAMS_LAUNCH)) {
    utt_narrow_fused_kernel<kNFUnr, kNFHU, kNFGA, kNFGV><<<static_cast<unsigned>(grid), kNFThreads, kNFLds, stream>>>(f);
  }
  MMB_LAUNCH_CHECK();
  return reduce_colmax(MMB_OK, f.s, static_cast<int>(grid) * kNFWaves, colmax, stream);
}

extern "C" int mmb_mm2_stream_project_narrow(const int32_t* ids, const float* table, int64_t v,
                                             const float* wtab32, const void* text_cache,
                                             const float* audio, const float* visual, int64_t n,
                                             int t, int d, int a_, int vd, const void* wpieces,
                                             const float* c0, float* num_out, float* aux_out,
                                             float* mmb2_out, int32_t* flag, uint32_t* colmax,
                                             void* colmax_ws, hipStream_t stream) {
  return narrow_project(MMB_TABLE_F32, MMB_FRAMES_F32, ids, table, v, wtab32, text_cache, audio, visual, n, t, d, a_,
                        vd, wpieces, c0, num_out, aux_out, mmb2_out, flag, colmax, colmax_ws, stream);
}

extern "C" int mmb_mm2_stream_project_narrow_ft(const int32_t* ids, const float* table, int64_t v,
                                                const float* wtab32, const void* text_cache,
                                                const void* audio, const void* visual, int frame_type,
                                                int64_t n, int t, int d, int a_, int vd, const void* wpieces,
                                                const float* c0, float* num_out, float* aux_out,
                                                float* mmb2_out, int32_t* flag, uint32_t* colmax,
                                                void* colmax_ws, hipStream_t stream) {
  MMB_REQUIRE(frame_bytes(frame_type) != 0);
  return narrow_project(MMB_TABLE_F32, frame_type, ids, table, v, wtab32, text_cache, audio, visual, n, t, d, a_, vd,
                        wpieces, c0, num_out, aux_out, mmb2_out, flag, colmax, colmax_ws, stream);
}

extern "C" int mmb_mm2_stream_project_narrow_tt(const int32_t* ids, const void* table, int table_type, int64_t v,
                                                const float* wtab32, const void* text_cache,
                                                const void* audio, const void* visual, int frame_type,
                                                int64_t n, int t, int d, int a_, int vd, const void* wpieces,
                                                const float* c0, float* num_out, float* aux_out,
                                                float* mmb2_out, int32_t* flag, uint32_t* colmax,
                                                void* colmax_ws, hipStream_t stream) {
  MMB_REQUIRE(table_bytes(table_type) != 0 && frame_bytes(frame_type) != 0);
  return narrow_project(table_type, frame_type, ids, table, v, wtab32, text_cache, audio, visual, n, t, d, a_, vd,
                        wpieces, c0, num_out, aux_out, mmb2_out, flag, colmax, colmax_ws, stream);
}

// the tools build's two-team variant (tools/diag/); the product library
// includes an empty header here
#ifndef MMB_TOOLS_TAIL_NARROW_FUSED
#define MMB_TOOLS_TAIL_NARROW_FUSED "mmb_no_tools.h"
#endif
#include MMB_TOOLS_TAIL_NARROW_FUSED
