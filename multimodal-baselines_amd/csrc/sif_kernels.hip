// SIF word-weight gather (a1), weighted gather-reduce (a2) and the fused
// text+audio+visual per-utterance sums of the closed-form MMB2 (a6/a7/a8 stream).
//
// Design (MI355X): one workgroup of 320 threads (5 waves) owns one utterance at
// a time (grid-stride over utterances).  A 300-wide f32 row is 75 float4 column
// units; 4 row slots x 75 units = 300 active lanes, so every wave-instruction
// issues 16 B/lane loads that cover contiguous 1 KiB runs of a frame row or a
// gathered table row.  The utterance's token ids and weights are staged in LDS
// (broadcast reads), the per-slot partial sums are combined through one LDS
// image per accumulator in a fixed order (deterministic), and only the
// reductions leave the chip: the [N,L,300] gathered text tensor the reference
// materialises (simplesif.py:319-340, :871) never exists.
//
// The stream kernels proper: every f32-table instantiation of utt_stream_kernel
// and utt_wave_kernel (the templates, their launchers and the route selection
// are in mmb_stream_kernels.h; the instantiations for a 16-bit word table in
// sif_tab_f16_kernels.hip and sif_tab_bf16_kernels.hip) and utt_narrow_kernel,
// every f32-table instantiation of the split stream (utt_split_part_kernel,
// utt_split_finish_kernel: few long rows split over workgroups; the templates
// and their launcher are in mmb_split_kernels.h, the instantiations for a
// 16-bit word table in split_tab_f16_kernels.hip and
// split_tab_bf16_kernels.hip), the entry points of all of them, and the
// host-side front end that all stream entry points share (mmb_stream.h).  The
// fused families have a source each: fused_kernels.hip (stream + projection in
// one kernel), narrow_fused_kernels.hip (the same at narrow frame widths).
// The f32-table split stream stays in this translation unit on purpose: it
// shares text_rows<.., TU = 8> with utt_stream_kernel's few-long-rows
// instantiations (FU = 16, TU = 8), and compiled without it in the module
// those 24 kernels come out with other code (other sizes and register
// counts).  For the same reason nothing else is instantiated here: a kernel
// for another table type goes into a source of its own.
#include "mmb_stream_kernels.h"
#include "mmb_split_kernels.h"

namespace mmb {


// ------------------------------------------------------ narrow-frame stream
// MMB2 stream kernel for narrow frame rows (MOSI: COVAREP A = 76, FACET
// Vd = 48 -- 19 and 12 float4 units).  utt_wave_kernel gives every frame row
// its own wave-instruction, so at these widths 19 / 12 of the 64 lanes load
// (304 / 192 B per instruction) and a wave moves ~2 KB per HBM round trip:
// latency-bound at ~2.9 TB/s.  Here a wave-instruction covers P = 64 / U
// consecutive frame rows (lane -> frame slot f = lane / U, unit c = lane % U:
// 3 rows = 912 contiguous bytes of audio, 5 rows = 960 B of visual; lanes past
// P U load a duplicate), and ALL of an utterance's frame instructions (7 + 4
// at T = 20) are issued together, before its text groups: one HBM round trip
// per utterance for ~10 KB.  The token ids of the next utterance are loaded
// one utterance ahead and its weights gathered before the loop turns, so a
// text group waits for nothing but the (L2-resident at MOSI's V = 3016) table
// rows.  (The last iteration resolves its own ids a second time: an
// out-of-range id sets the same flag bit again.)
// Sums: the text sums (and so x, aux's count and weight sum, the column
// bounds) are utt_wave_kernel's operations in its order: bit-identical.  The
// frame sums (FR = 1, the product) are per-lane partials over the rows of one
// slot (f, f + P, f + 2P, ...) added slot 0 + 1 + ... at the end -- another
// f32 summation order than the wave kernel's t = 0, 1, ... (within f32
// rounding of it; the reference's torch sum over T fixes no order either).
// FR = 0 gathers every frame across the packed lanes (ds_bpermute) in t order
// instead: bit-identical to the wave kernel, 0.5 ms slower at MOSI (r03z).
// GA / GV: frame instructions per modality issued at once (7 + 4 = all of a
// T = 20 MOSI utterance; longer utterances take further groups after the text)
// ABL (tools build, timing-only ablations with wrong outputs): bit 0 skips the
// text rows, bit 1 the frames, bit 2 the row stores (kept live behind a test
// no value passes)
// FR: 0 = frames gathered frame by frame (ds_bpermute, the wave kernel's
// order), 1 = per-lane slot partials combined slot 0 + 1 + ... at the end.
// ORD: 0 = utterances round robin over the waves, 1 = a contiguous range per
// wave (neighbouring x / s / aux rows written by one wave: whole lines).
template <int CT, int UNR, int GA_MAX, int GV_MAX, int OCC = 2, int ABL = 0, int FR = 0, int ORD = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(OCC, 8))) void utt_narrow_kernel(StreamArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  // the wave index made visibly wave-uniform: utterance bases stay in SGPRs
  const int64_t wid = static_cast<int64_t>(blockIdx.x) * (blockDim.x / kWave) +
                      __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int64_t nw = static_cast<int64_t>(gridDim.x) * (blockDim.x / kWave);
  const int L = a.L, D = a.D;
  const int UT = D >> 2, UA = a.A >> 2, UV = a.Vd >> 2;
  const int PA = kWave / UA, PV = kWave / UV;  // frame rows per instruction (>= 2)
  const int GA = (L + PA - 1) / PA, GV = (L + PV - 1) / PV;
  // Loads go through buffer descriptors: a scalar offset per row / per packed
  // instruction and a fixed per-lane column offset -- no 64-bit address
  // arithmetic in VGPRs.  A row id < 0 (out of range, flagged) reads past the
  // table's record count, which returns zeros (a zero row, as the wave
  // kernel's select).  Text column offsets clamped into the row (lanes past
  // unit 74 read a duplicate the L1 coalesces and never store it).
  int vt[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) vt[c] = 16 * min(lane + kWave * c, UT - 1);
  const int tbytes = static_cast<int>(a.V * D * 4);
  const auto trsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.table), 0, tbytes, 0x00020000);
  // lane f U + c of a packed frame instruction: frame row f, unit c
  const int voa = ((lane / UA) * a.A + 4 * (lane % UA)) * 4;
  const int vov = ((lane / UV) * a.Vd + 4 * (lane % UV)) * 4;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 cmx[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) cmx[c] = z4;

  // token t of utterance i on lane t: the raw id (prefetched one utterance
  // ahead), then stage_token's semantics
  auto ld_id = [&](int64_t i) -> int { return (i < a.N && lane < L) ? a.ids[i * L + lane] : -1; };
  // (the weight gather is issued here and first waited for by the text loop,
  // behind the frame loads: the wave sums of the weights come after the text;
  // an id outside [0, V) -- a negative one wraps for its ROW only -- reads
  // past the weight table's record count: weight 0 with no select)
  const auto wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wtab), 0,
                                                       static_cast<int>(a.V * 4), 0x00020000);
  auto resolve = [&](int raw, int& rid, float& w) {
    rid = -1;
    w = 0.f;
    if (lane < L) {
      int64_t id = raw;
      const bool in = id >= 0 && id < a.V;
      w = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                        wrsrc, in ? static_cast<int>(id) * 4 : static_cast<int>(a.V * 4), 0, 0));
      if (id < 0) id += a.V;
      if (id < 0 || id >= a.V) {
        if (a.flag) atomicOr(a.flag, MMB_FLAG_ID_RANGE);
      } else {
        rid = static_cast<int>(id);
      }
    }
  };
  const int64_t chunk = (a.N + nw - 1) / nw;
  const int64_t i_beg = ORD ? wid * chunk : wid;
  const int64_t i_end = ORD ? min(a.N, i_beg + chunk) : a.N;
  const int64_t i_step = ORD ? 1 : nw;
  // The next utterance's ids are loaded at the top of an iteration and
  // resolved (row ids, weight gather issued) at its end BEFORE its row stores:
  // with loads and stores both pending, gfx9's one vmcnt counter makes any
  // wait a wait for everything (s_waitcnt vmcnt(0)), so an iteration that
  // began by waiting for its ids waited for the previous row's stores too.
  int rid_n, raw = -1;
  float w_n;
  resolve(i_beg < i_end ? ld_id(i_beg) : -1, rid_n, w_n);
  for (int64_t i = i_beg; i < i_end; i += i_step) {
    const int rid = rid_n;
    float w = w_n;
    if (i + i_step < i_end) raw = ld_id(i + i_step);  // in flight through this utterance

    // frames: the first GA_MAX / GV_MAX packed instructions per modality
    // issued before the text loop (rows past L read zeros past the record count)
    const auto arsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(frames<float>(a.audio) + i * L * a.A), 0,
                                                         L * a.A * 4, 0x00020000);
    const auto vrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(frames<float>(a.visual) + i * L * a.Vd), 0,
                                                         L * a.Vd * 4, 0x00020000);
    float4 sa = z4, saa = z4, sv = z4, svv = z4;
    auto frames = [&](auto gmax, auto rsrc, int vo, int W, int U, int P, int g0, float4& s1, float4& s2) {
      constexpr int GM = decltype(gmax)::value;
      float4 v[GM > 0 ? GM : 1];
#pragma unroll
      for (int g = 0; g < GM; ++g)  // non-temporal: read-once streams
        v[g] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, vo, (g0 + g) * P * W * 4, 2));
      // frame t = g P + q of unit c sits on lane q U + c: lane c < U adds the
      // frames in order t = 0, 1, ... (ds_bpermute), the order of
      // utt_wave_kernel / the fused kernel's frame_piece -- bit-identical sums
      const int c = lane % U;
      const bool mine = lane < P * U;
      return [=, &s1, &s2]() {
#pragma unroll
        for (int g = 0; g < GM; ++g) {
          if constexpr (FR == 1) {  // rows past L read zeros
            if (mine) {
              add4(s1, v[g]);
              sq4(s2, v[g]);
            }
            continue;
          }
          for (int q = 0; q < P; ++q) {
            if ((g0 + g) * P + q >= L) break;
            const int src = min(q * U + c, kWave - 1);
            float4 x;
            x.x = __shfl(v[g].x, src, kWave);
            x.y = __shfl(v[g].y, src, kWave);
            x.z = __shfl(v[g].z, src, kWave);
            x.w = __shfl(v[g].w, src, kWave);
            add4(s1, x);
            sq4(s2, x);
          }
        }
      };
    };
    using GAc = std::integral_constant<int, GA_MAX>;
    using GVc = std::integral_constant<int, GV_MAX>;
    using G0 = std::integral_constant<int, 0>;
    auto acc_a = frames(std::conditional_t<(ABL & 2) != 0, G0, GAc>{}, arsrc, voa, a.A, UA, PA, 0, sa, saa);
    auto acc_v = frames(std::conditional_t<(ABL & 2) != 0, G0, GVc>{}, vrsrc, vov, a.Vd, UV, PV, 0, sv, svv);

    // text: utt_sums' text half, the same operations in the same order
    float4 num[CT], sx[CT], sxx[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) num[c] = sx[c] = sxx[c] = z4;
    auto row = [&](int t, float4 (&v)[CT]) {
      const int r = __builtin_amdgcn_readlane(rid, t);
      const int so = r >= 0 ? r * D * 4 : tbytes;  // out of range: a zero row
#pragma unroll
      for (int c = 0; c < CT; ++c)
        v[c] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(trsrc, vt[c], so, 0));
    };
    // (the weight is read at accumulation: its gather is waited for there)
    auto accum = [&](int t, const float4 (&v)[CT]) {
      const float wt = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), t));
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        fma4(num[c], wt, v[c]);
        add4(sx[c], v[c]);
        sq4(sxx[c], v[c]);
      }
    };
    int t = (ABL & 1) ? L : 0;
    for (; t + UNR <= L; t += UNR) {
      float4 v[UNR][CT];
#pragma unroll
      for (int u = 0; u < UNR; ++u) row(t + u, v[u]);
#pragma unroll
      for (int u = 0; u < UNR; ++u) accum(t + u, v[u]);
    }
    for (; t < L; ++t) {
      float4 v[CT];
      row(t, v);
      accum(t, v);
    }
    acc_a();
    acc_v();
    const float cnt = wave_sum((w != 0.f) ? 1.f : 0.f);
    const float sw = wave_sum(w);
    if (lane == 0 && cnt == 0.f && a.flag) atomicOr(a.flag, MMB_FLAG_ZERO_WEIGHTS);
    if constexpr ((ABL & 2) == 0)
    for (int g0 = GA_MAX; g0 < GA; g0 += GA_MAX) frames(GAc{}, arsrc, voa, a.A, UA, PA, g0, sa, saa)();
    if constexpr ((ABL & 2) == 0)
    for (int g0 = GV_MAX; g0 < GV; g0 += GV_MAX) frames(GVc{}, vrsrc, vov, a.Vd, UV, PV, g0, sv, svv)();
    if constexpr (FR == 1) {  // slot partials -> unit totals on lanes < U, slot 0 + 1 + ...
      auto slots = [&](float4& acc, int U, int P) {
        float4 r = acc;
        for (int f = 1; f < P; ++f) {
          const int src = min(lane + f * U, kWave - 1);
          float4 o;
          o.x = __shfl(acc.x, src, kWave);
          o.y = __shfl(acc.y, src, kWave);
          o.z = __shfl(acc.z, src, kWave);
          o.w = __shfl(acc.w, src, kWave);
          add4(r, o);
        }
        acc = r;
      };
      slots(sa, UA, PA);
      slots(saa, UA, PA);
      slots(sv, UV, PV);
      slots(svv, UV, PV);
    }
    // lanes past a modality's units summed duplicates: keep them out of the row max
    if (lane >= UA) sa = saa = z4;
    if (lane >= UV) sv = svv = z4;

    float m = fmaxf(fmaxf(amax4(sa), amax4(saa)), fmaxf(amax4(sv), amax4(svv)));
#pragma unroll
    for (int c = 0; c < CT; ++c) m = fmaxf(m, fmaxf(amax4(sx[c]), amax4(sxx[c])));
    const float rs = row_scale(wave_max(m));
    resolve(raw, rid_n, w_n);  // the next utterance's (see above)
    if ((ABL & 4) != 0 && rs != 3.f) continue;  // (never 3: a power of two)
    _Float16* hrow = reinterpret_cast<_Float16*>(a.s_out) + i * 2 * a.Kp;
    auto put = [&](int f, float4 v) { split_store4<false>(hrow + f, hrow + a.Kp + f, v, rs); };
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const int u = lane + kWave * c;
      if (u < UT) {
        const float4 xr = div4(num[c], cnt);
        st4(a.num_out + i * D + 4 * u, xr);  // x = the a2 row
        cmx[c] = bmax4(cmx[c], xr);
        put(4 * u, sx[c]);
        put(D + 4 * u, sxx[c]);
      }
    }
    if (lane < UA) {
      put(2 * D + 4 * lane, sa);
      put(2 * D + a.A + 4 * lane, saa);
    }
    if (lane < UV) {
      put(2 * (D + a.A) + 4 * lane, sv);
      put(2 * (D + a.A) + a.Vd + 4 * lane, svv);
    }
    for (int f = 2 * (D + a.A + a.Vd) + lane; f < a.Kp; f += kWave)
      hrow[f] = hrow[a.Kp + f] = static_cast<_Float16>(0.f);
    if (lane == 0) {
      a.aux_out[i] = cnt;  // planar [3][N]: count | sum w | fp16 row scale
      a.aux_out[a.N + i] = sw;
      a.aux_out[2 * a.N + i] = rs;
    }
  }
  if (a.cmax_part) {  // this wave's column bounds (mmb_gram_i8)
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const int u = lane + kWave * c;
      if (u < UT) st4(a.cmax_part + wid * D + 4 * u, cmx[c]);
    }
  }
}

// the narrow kernel's shapes: gathered ids with the weight table, fp16 s,
// text rows of 65-128 float4 units (CT = 2; the MOSI / bench D = 300), frame
// rows of at most 32 units (two or more rows per instruction), T <= 64
bool narrow_ok(const StreamArgs& a) {
  return a.ids && a.wtab && !a.w_dense && a.s_half && a.D > 256 && a.D <= 512 &&
         a.A <= 128 && a.Vd <= 128 && a.L <= kWave && a.V * a.D * 4 < (int64_t{1} << 31);
}

// colmax[f] = max over the P partial rows (float bits; non-negative floats
// order like their bits), fixed order.  16 row groups per column, LDS reduce.
__global__ __launch_bounds__(1024) void colmax_reduce_kernel(const float* __restrict__ part, int P,
                                                            int D, unsigned* __restrict__ colmax) {
  __shared__ float s_m[16][64];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int f = blockIdx.x * 64 + c;
  float m = 0.f;
  if (f < D) {
    // 8 independent loads in flight per thread (a single chain is latency-bound)
    float mm[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int r = g;
    for (; r + 7 * 16 < P; r += 8 * 16) {
#pragma unroll
      for (int u = 0; u < 8; ++u) mm[u] = bmax(mm[u], part[static_cast<int64_t>(r + 16 * u) * D + f]);
    }
    for (; r < P; r += 16) mm[0] = bmax(mm[0], part[static_cast<int64_t>(r) * D + f]);
#pragma unroll
    for (int u = 0; u < 8; ++u) m = bmax(m, mm[u]);
  }
  s_m[g][c] = m;
  __syncthreads();
  if (g == 0 && f < D) {
    for (int k = 1; k < 16; ++k) m = bmax(m, s_m[k][c]);
    colmax[f] = __float_as_uint(m);
  }
}


// Narrow-frame kernel variant (MMB_STREAM_NARROW, tools build; the product
// runs 10).  Measured (r03z, MOSI 1M x 20, A = 76, Vd = 48, V = 3016, same
// process, stream kernel ms): utt_wave_kernel (0) 5.04; frames gathered frame
// by frame, 4 / 5 text rows per load group (2 / 3) 4.41 / 4.34; 10 rows at
// occupancy 2 (4) 4.74; 5 rows forced to 4 waves per SIMD (5, spills) 5.15;
// slot-partial frame sums (10) 3.81; contiguous utterance ranges per wave (11
// = 3, 12 = 10 with it) no change; 8-row groups (13, occupancy 2) 4.41;
// not kept (removed after measuring): the text rows' last column load on
// its 11 live lanes only 3.87 vs 3.87; the last 11 units of 5 text rows in
// ONE packed instruction (16 instead of 40 text loads per utterance) 3.89 vs
// 3.85 with 5-row groups, 4.44 with 10; the next utterance's ids resolved
// before the row stores (kept: no iteration starts by waiting for the
// previous row's stores) 3.87 vs 3.81; slot partials with 7 / 10 text rows
// per group (occupancy 2) 4.31 / 3.90, 7 rows forced to occupancy 3 (7 VGPRs
// spilled) 4.09 vs 3.84.
// Timing-only ablations of 3 (wrong rows): no text 3.14 (6), no frames 2.32
// (7), no row stores 3.61 (8), neither text nor frames 1.41 (9).
#ifndef MMB_HOOK_NARROW_VARIANT
#define MMB_HOOK_NARROW_VARIANT 10
#endif
int narrow_variant() { return MMB_HOOK_NARROW_VARIANT; }

int launch_narrow(const StreamArgs& a, hipStream_t stream, int* parts) {
  const int var = narrow_variant();
  // resident workgroups of 4 waves per CU at each variant's occupancy
  const int per_cu = (var == 4 || var == 13) ? 2 : var == 5 ? 4 : 3;
  const int grid = wave_grid(a, per_cu, stream, parts);
#ifndef MMB_HOOK_NARROW_LAUNCH  // (tools/diag: the variant sweep)
#define MMB_HOOK_NARROW_LAUNCH false
#endif
  if (!(MMB_HOOK_NARROW_LAUNCH)) utt_narrow_kernel<2, 5, 7, 4, 2, 0, 1, 0><<<grid, 256, 0, stream>>>(a);
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}


__global__ void seq2weight_kernel(const int32_t* __restrict__ seq, const uint8_t* __restrict__ sel,
                                  int64_t total, const double* __restrict__ wtab, int64_t V,
                                  float* __restrict__ w, int32_t* flag) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < total;
       k += (int64_t)gridDim.x * blockDim.x) {
    const int32_t id = seq[k];
    float out = 0.f;
    if ((sel == nullptr || sel[k]) && id >= 0) {
      if (id < V) {
        out = static_cast<float>(wtab[id]);  // f64 -> f32, round to nearest (sif_functions.py:13)
      } else if (flag) {
        atomicOr(flag, MMB_FLAG_ID_RANGE);
      }
    }
    w[k] = out;
  }
}

__global__ void calc_weights_kernel(const float* __restrict__ x, int64_t total, int F,
                                    const float* __restrict__ bm, const float* __restrict__ bl,
                                    float* __restrict__ qm, float* __restrict__ qs) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < total;
       k += (int64_t)gridDim.x * blockDim.x) {
    const int f = static_cast<int>(k % F);
    const float d = x[k] - bm[f];
    const float e = expf(2.f * bl[f]);
    qm[k] = d / e;
    qs[k] = d * d / e - 1.f;
  }
}

int stream_cu_count(hipStream_t stream) {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    return 256;
  }
  if (stream == nullptr) return n;
  uint32_t mask[32] = {};
  if (hipExtStreamGetCUMask(stream, 32, mask) != hipSuccess) {
    (void)hipGetLastError();  // a query failure is not a launch error
    return n;
  }
  int c = 0;
  for (int b = 0; b < n && b < 32 * 32; ++b) c += (mask[b >> 5] >> (b & 31)) & 1;
  return (c > 0 && c < n) ? c : n;
}


// ------------------------------------------------ the entry points' front end
// What mmb_sif_wavg and the MMB2 stream entry points do alike, once:
// their shared checks and the StreamArgs they hand to a kernel, the empty
// call, the vector eligibility of the three modalities, and the column-bound
// reduction that ends every path.  An entry point keeps what is particular to
// it: its own limits, its kernel choice and its grid.

// The text source: gathered (ids into table, weights from wtab32 or given
// per token) or dense (text_dense frames, emb_dense rows, given weights).
bool set_text_source(StreamArgs* s, const int32_t* ids, const float* table, int64_t v,
                     const float* wtab32, const float* text_dense, const float* emb_dense,
                     const float* w_dense) {
  if (ids ? !(table && v > 0 && (wtab32 || w_dense)) : !(text_dense && emb_dense && w_dense)) return false;
  s->ids = ids; s->table = table; s->V = v; s->wtab = wtab32; s->w_dense = w_dense;
  s->text_dense = text_dense; s->emb_dense = emb_dense;
  return true;
}

// The StreamArgs of an MMB2 stream call (s_out is null for the fused kernels,
// which keep the sums on chip), after the checks every such call gets:
// positive shapes, the text source, the outputs, bounds only with a workspace.
int stream_args(StreamArgs* s, const int32_t* ids, const float* table, int64_t v, const float* wtab32,
                const float* text_dense, const float* emb_dense, const float* w_dense, const void* audio,
                const void* visual, int64_t n, int t, int d, int a_, int vd, float* num_out, void* s_out,
                int s_half, float* aux_out, int32_t* flag, const uint32_t* colmax, void* colmax_ws) {
  MMB_REQUIRE(n >= 0 && t > 0 && d > 0 && a_ > 0 && vd > 0);
  MMB_REQUIRE(audio && visual && num_out && aux_out && (s_half == 0 || s_half == 1));
  MMB_REQUIRE(colmax == nullptr || colmax_ws != nullptr);
  *s = StreamArgs{};
  MMB_REQUIRE(set_text_source(s, ids, table, v, wtab32, text_dense, emb_dense, w_dense));
  s->audio = audio; s->visual = visual;
  s->N = n; s->L = t; s->D = d; s->A = a_; s->Vd = vd; s->Kp = mmb_mm2_k(d, a_, vd);
  s->num_out = num_out; s->s_out = static_cast<float*>(s_out); s->aux_out = aux_out; s->flag = flag;
  s->s_half = s_half;
  s->cmax_part = colmax ? static_cast<float*>(colmax_ws) : nullptr;
  return MMB_OK;
}

// The empty call: no rows, so every column bound is 0 (cleared by a kernel:
// no memset node, see zero_words_async).
int empty_call(uint32_t* colmax, int d, hipStream_t stream) {
  return colmax ? zero_words_async(colmax, d, stream) : MMB_OK;
}

// The end of every path: the column bounds as the max over the `parts`
// per-wave / per-workgroup rows the stream launch (rc) left in the workspace.
int reduce_colmax(int rc, const StreamArgs& s, int parts, uint32_t* colmax, hipStream_t stream) {
  if (rc != MMB_OK || !colmax) return rc;
  colmax_reduce_kernel<<<static_cast<unsigned>(ceil_div(s.D, 64)), 1024, 0, stream>>>(s.cmax_part, parts,
                                                                                      s.D, colmax);
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

// Vector eligibility of the three modalities (StreamVec): rows of whole
// column units of 4 values from a base aligned to one unit.  A text unit is a
// float4 -- of a 16-bit word table 4 * tbytes = 8 bytes (table_bytes); a
// frame unit is 4 * fbytes bytes (frame_bytes: 16 of f32, one b128 load, 8 of
// a 16-bit type, one b64 load).
StreamVec stream_vec(const StreamArgs& s, int fbytes, int tbytes) {
  auto unit = [&](int w, const void* p, int bytes) {
    return w % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & (4 * bytes - 1)) == 0;
  };
  return {s.ids ? unit(s.D, s.table, tbytes) : (s.D % 4 == 0 && aligned16(s.text_dense) && aligned16(s.emb_dense)),
          unit(s.A, s.audio, fbytes), unit(s.Vd, s.visual, fbytes)};
}
// the workgroup kernels' limit: a thread per column unit (float4 or scalar)
bool units_fit(const StreamArgs& s, const StreamVec& vec) {
  return s.D / (vec.t ? 4 : 1) <= kNT && s.A / (vec.a ? 4 : 1) <= kNT && s.Vd / (vec.v ? 4 : 1) <= kNT;
}

}  // namespace mmb

using namespace mmb;

extern "C" int mmb_version(void) { return 100; }

extern "C" int mmb_cu_count(int device, int* out) {
  MMB_REQUIRE(out);
  const hipError_t e = hipDeviceGetAttribute(out, hipDeviceAttributeMultiprocessorCount, device);
  return e == hipSuccess ? MMB_OK : static_cast<int>(e);
}

extern "C" int mmb_stream_create_cu_mask(const uint32_t* cu_mask, int mask_words,
                                         hipStream_t* out) {
  MMB_REQUIRE(cu_mask && mask_words > 0 && out);
  const hipError_t e =
      hipExtStreamCreateWithCUMask(out, static_cast<uint32_t>(mask_words), cu_mask);
  return e == hipSuccess ? MMB_OK : static_cast<int>(e);
}

extern "C" int mmb_stream_destroy(hipStream_t stream) {
  MMB_REQUIRE(stream);
  const hipError_t e = hipStreamDestroy(stream);
  return e == hipSuccess ? MMB_OK : static_cast<int>(e);
}

extern "C" int mmb_seq2weight(const int32_t* seq, const uint8_t* sel, int64_t n, int64_t l,
                              const double* wtab64, int64_t v, float* w_out, int32_t* flag,
                              hipStream_t stream) {
  MMB_REQUIRE(n >= 0 && l >= 0 && v > 0 && seq && wtab64 && w_out);
  const int64_t total = n * l;
  if (total == 0) return MMB_OK;
  const int grid = static_cast<int>(std::min<int64_t>(ceil_div(total, 256), 256 * 16));
  seq2weight_kernel<<<grid, 256, 0, stream>>>(seq, sel, total, wtab64, v, w_out, flag);
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

// mmb_sif_wavg and mmb_sif_wavg_tt on a table of storage type table_type
// (validated by the caller): the checks, the route, the launch of the kernel
// instantiated for the table type.
static int sif_wavg(int table_type, const void* table, int64_t v, int d, const int32_t* ids, int64_t n, int l,
                    const float* w, const float* wtab32, float* x_out, float* num_out, float* cnt_out,
                    int32_t* flag, hipStream_t stream) {
  const int tb = table_bytes(table_type);
  MMB_REQUIRE(ids && d > 0 && n >= 0 && l >= 0);
  MMB_REQUIRE(x_out || num_out || cnt_out);
  StreamArgs a{};
  MMB_REQUIRE(set_text_source(&a, ids, static_cast<const float*>(table), v, wtab32, nullptr, nullptr, w));
  // a 16-bit value is never read from an odd address, scalar rows included
  MMB_REQUIRE(tb == 4 || (reinterpret_cast<uintptr_t>(table) & 1) == 0);
  if (n == 0) return MMB_OK;
  a.N = n; a.L = l; a.D = d;
  a.x_out = x_out; a.num_out = num_out; a.cnt_out = cnt_out; a.flag = flag;
  // a text column unit: 4 values, 16 bytes of f32 or 8 of a 16-bit type
  const bool v4 = (d % 4 == 0) && (reinterpret_cast<uintptr_t>(table) & (4 * tb - 1)) == 0;
  const bool wave = v4 && l <= kWave && d <= 512 && (x_out == nullptr || aligned16(x_out)) &&
                    (num_out == nullptr || aligned16(num_out));
  if (!wave) MMB_REQUIRE(d / (v4 ? 4 : 1) <= kNT && d <= kRedFloats);
  return table_type == MMB_TABLE_F32   ? sif_route<float>(a, v4, wave, stream)
         : table_type == MMB_TABLE_F16 ? sif_route_f16(a, v4, wave, stream)
                                       : sif_route_bf16(a, v4, wave, stream);
}

extern "C" int mmb_sif_wavg(const float* table, int64_t v, int d, const int32_t* ids, int64_t n,
                            int l, const float* w, const float* wtab32, float* x_out,
                            float* num_out, float* cnt_out, int32_t* flag, hipStream_t stream) {
  return sif_wavg(MMB_TABLE_F32, table, v, d, ids, n, l, w, wtab32, x_out, num_out, cnt_out, flag, stream);
}

extern "C" int mmb_sif_wavg_tt(const void* table, int table_type, int64_t v, int d, const int32_t* ids,
                               int64_t n, int l, const float* w, const float* wtab32, float* x_out,
                               float* num_out, float* cnt_out, int32_t* flag, hipStream_t stream) {
  MMB_REQUIRE(table_bytes(table_type) != 0);
  return sif_wavg(table_type, table, v, d, ids, n, l, w, wtab32, x_out, num_out, cnt_out, flag, stream);
}

extern "C" int mmb_calc_weights(const float* x, int64_t rows, int f, const float* b_mean,
                                const float* b_log_sigma, float* q_mean, float* q_sigma,
                                hipStream_t stream) {
  MMB_REQUIRE(x && b_mean && b_log_sigma && q_mean && q_sigma && rows >= 0 && f > 0);
  const int64_t total = rows * f;
  if (total == 0) return MMB_OK;
  const int grid = static_cast<int>(std::min<int64_t>(ceil_div(total, 256), 256 * 16));
  calc_weights_kernel<<<grid, 256, 0, stream>>>(x, total, f, b_mean, b_log_sigma, q_mean, q_sigma);
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

extern "C" int mmb_mm2_k(int d, int a, int vd) {
  const int k = 2 * (d + a + vd);
  return (k + 31) / 32 * 32;
}

// The workgroup stream kernel writes fp32 sums; for the fp16 hi/lo format a
// second pass splits each row in place (one workgroup per row, the row staged
// in LDS).  Only the fallback shapes (tokens > 64, widths not % 4) take it.
__global__ __launch_bounds__(256) void split_rows_kernel(float* __restrict__ s,
                                                         const float* __restrict__ rscale,
                                                         int Kp) {
  extern __shared__ float srow[];
  const int64_t i = blockIdx.x;
  float* row = s + i * Kp;
  for (int f = threadIdx.x; f < Kp; f += blockDim.x) srow[f] = row[f];
  __syncthreads();
  const float rs = rscale[i];
  _Float16* hi = reinterpret_cast<_Float16*>(row);
  for (int f = threadIdx.x; f < Kp; f += blockDim.x) {
    const float x = srow[f] * rs;
    const _Float16 h = static_cast<_Float16>(x);
    hi[f] = h;
    hi[Kp + f] = static_cast<_Float16>(x - static_cast<float>(h));
  }
}

int mmb::split_rows(const StreamArgs& s, hipStream_t stream) {
  split_rows_kernel<<<static_cast<unsigned>(s.N), 256, s.Kp * sizeof(float), stream>>>(
      s.s_out, s.aux_out + 2 * s.N, s.Kp);
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

// the column-bound partials [kCmaxRows][d], then (mmb_mm2_stream_project)
// the fused kernel's batch counter (16 bytes)
extern "C" size_t mmb_mm2_colmax_ws_bytes(int d) {
  return static_cast<size_t>(kCmaxRows) * (d > 0 ? d : 0) * sizeof(float) + 16;
}


extern "C" int mmb_mm2_stream(const int32_t* ids, const float* table, int64_t v,
                              const float* wtab32, const float* text_dense,
                              const float* emb_dense, const float* w_dense, const float* audio,
                              const float* visual, int64_t n, int t, int d, int a_, int vd,
                              float* num_out, void* s_out, int s_half, float* aux_out,
                              int32_t* flag, uint32_t* colmax, void* colmax_ws,
                              hipStream_t stream) {
  StreamArgs s;
  if (const int rc = stream_args(&s, ids, table, v, wtab32, text_dense, emb_dense, w_dense, audio, visual, n,
                                 t, d, a_, vd, num_out, s_out, s_half, aux_out, flag, colmax, colmax_ws))
    return rc;
  MMB_REQUIRE(s_out && (colmax == nullptr || d <= 2 * kNT));
  if (n == 0) return empty_call(colmax, d, stream);
  return stream_route<float>(s, colmax, stream);
}

// mmb_mm2_stream_ft and mmb_mm2_stream_tt on a table of storage type
// table_type and frames of storage type frame_type (both validated by the
// caller): the checks, then the routes of the kernels instantiated for the pair.
static int stream_gathered(int table_type, int frame_type, const int32_t* ids, const void* table, int64_t v,
                           const float* wtab32, const float* w_dense, const void* audio, const void* visual,
                           int64_t n, int t, int d, int a_, int vd, float* num_out, void* s_out, int s_half,
                           float* aux_out, int32_t* flag, uint32_t* colmax, void* colmax_ws,
                           hipStream_t stream) {
  const int fb = frame_bytes(frame_type), tb = table_bytes(table_type);
  MMB_REQUIRE(ids);  // gathered text only
  StreamArgs s;
  if (const int rc = stream_args(&s, ids, static_cast<const float*>(table), v, wtab32, nullptr, nullptr, w_dense,
                                 audio, visual, n, t, d, a_, vd, num_out, s_out, s_half, aux_out, flag, colmax,
                                 colmax_ws))
    return rc;
  MMB_REQUIRE(s_out && (colmax == nullptr || d <= 2 * kNT));
  // a 16-bit value is never read from an odd address, scalar rows included
  MMB_REQUIRE(fb == 4 || ((reinterpret_cast<uintptr_t>(audio) | reinterpret_cast<uintptr_t>(visual)) & 1) == 0);
  MMB_REQUIRE(tb == 4 || (reinterpret_cast<uintptr_t>(table) & 1) == 0);
  if (n == 0) return empty_call(colmax, d, stream);
  return table_type == MMB_TABLE_F32   ? stream_route_frames<float>(s, frame_type, colmax, stream)
         : table_type == MMB_TABLE_F16 ? stream_route_f16(s, frame_type, colmax, stream)
                                       : stream_route_bf16(s, frame_type, colmax, stream);
}

extern "C" int mmb_mm2_stream_ft(const int32_t* ids, const float* table, int64_t v, const float* wtab32,
                                 const float* w_dense, const void* audio, const void* visual, int frame_type,
                                 int64_t n, int t, int d, int a_, int vd, float* num_out, void* s_out,
                                 int s_half, float* aux_out, int32_t* flag, uint32_t* colmax,
                                 void* colmax_ws, hipStream_t stream) {
  MMB_REQUIRE(frame_bytes(frame_type) != 0);
  return stream_gathered(MMB_TABLE_F32, frame_type, ids, table, v, wtab32, w_dense, audio, visual, n, t, d, a_, vd,
                         num_out, s_out, s_half, aux_out, flag, colmax, colmax_ws, stream);
}

extern "C" int mmb_mm2_stream_tt(const int32_t* ids, const void* table, int table_type, int64_t v,
                                 const float* wtab32, const float* w_dense, const void* audio,
                                 const void* visual, int frame_type, int64_t n, int t, int d, int a_, int vd,
                                 float* num_out, void* s_out, int s_half, float* aux_out, int32_t* flag,
                                 uint32_t* colmax, void* colmax_ws, hipStream_t stream) {
  MMB_REQUIRE(table_bytes(table_type) != 0 && frame_bytes(frame_type) != 0);
  return stream_gathered(table_type, frame_type, ids, table, v, wtab32, w_dense, audio, visual, n, t, d, a_, vd,
                         num_out, s_out, s_half, aux_out, flag, colmax, colmax_ws, stream);
}

// Ranges per utterance of the few-long-rows path: about one workgroup per
// CU in all (3 per range: text, audio, visual), no range under
// kSplitMinTok frames.  r06 sweep (tools/split_ab.py, graph-timed, POM's
// real splits): fewer, longer streams win -- valid (100 x 1089) 55.3 / 62.9
// / 64.8 / 64.8 us at 1 / 2 / 3 / 4 ranges, test (203 x 1357) 126 / 135 /
// 125 / 145 us; the one-workgroup kernel 89.7 / 134 us; a plain read of the
// same frame bytes (probe, 512 workgroups) 40.5 / 97 us.
constexpr int kSplitMinTok = 64;
static int split_parts(int64_t n, int t, int cus) {
  if (n <= 0 || t <= 0) return 1;
  const int64_t want = ceil_div(static_cast<int64_t>(cus), 3 * n);
  const int64_t cap = std::max<int64_t>(1, t / kSplitMinTok);
  return static_cast<int>(std::max<int64_t>(1, std::min(want, cap)));
}

extern "C" int mmb_mm2_stream_split_parts(int64_t n, int t) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
    (void)hipGetLastError();
    cus = 256;
  }
  return split_parts(n, t, cus);
}

static size_t split_ws_floats(int64_t n, const SplitPlan& q) {
  return static_cast<size_t>(n) * (static_cast<size_t>(q.Pt) * q.Wt + static_cast<size_t>(q.Pf) * q.Wf);
}

extern "C" size_t mmb_mm2_stream_split_ws_bytes(int64_t n, int t, int d, int a_, int vd, int parts) {
  if (n <= 0 || t <= 0 || d <= 0 || a_ <= 0 || vd <= 0) return 0;
  const int P = parts > 0 ? std::min(parts, t) : mmb_mm2_stream_split_parts(n, t);
  return split_ws_floats(n, split_plan_of(t, d, a_, vd, P, parts > 0 ? 1 : kSplitTextX)) * sizeof(float);
}

// mmb_mm2_stream_split, mmb_mm2_stream_split_ft and mmb_mm2_stream_split_tt on
// a table of storage type table_type and frames of storage type frame_type
// (both validated by the caller): the checks, the plan, the launch of the
// kernels instantiated for the pair, the column bounds.
static int split_stream(int table_type, int frame_type, const int32_t* ids, const void* table_, int64_t v,
                        const float* wtab32,
                        const float* text_dense, const float* emb_dense, const float* w_dense, const void* audio,
                        const void* visual, int64_t n, int t, int d, int a_, int vd, float* num_out, void* s_out,
                        int s_half, float* aux_out, int32_t* flag, uint32_t* colmax, void* colmax_ws, int parts,
                        void* ws, size_t ws_bytes, hipStream_t stream) {
  const int fb = frame_bytes(frame_type), tb = table_bytes(table_type);
  const float* table = static_cast<const float*>(table_);  // (StreamArgs::table; a TE kernel reads it as TE)
  StreamArgs s;
  if (const int rc = stream_args(&s, ids, table, v, wtab32, text_dense, emb_dense, w_dense, audio, visual, n,
                                 t, d, a_, vd, num_out, s_out, s_half, aux_out, flag, colmax, colmax_ws))
    return rc;
  // the bounds: a partial row per utterance
  MMB_REQUIRE(s_out && parts >= 0 && (colmax == nullptr || (d <= 2 * kNT && n <= kCmaxRows)));
  // a 16-bit value is never read from an odd address, scalar rows included
  MMB_REQUIRE(fb == 4 || ((reinterpret_cast<uintptr_t>(audio) | reinterpret_cast<uintptr_t>(visual)) & 1) == 0);
  MMB_REQUIRE(tb == 4 || (reinterpret_cast<uintptr_t>(table) & 1) == 0);
  // the empty call returns before the workspace is looked at, and before
  // mmb_mm2_stream_split_parts queries the device
  if (n == 0) return empty_call(colmax, d, stream);
  const int P = parts > 0 ? std::min(parts, t) : mmb_mm2_stream_split_parts(n, t);
  const SplitPlan q = split_plan_of(t, d, a_, vd, P, parts > 0 ? 1 : kSplitTextX);
  MMB_REQUIRE(ws && ws_bytes >= split_ws_floats(n, q) * sizeof(float));
  MMB_REQUIRE(n * (q.Pt + 2 * q.Pf) <= (int64_t{1} << 31) - 1);
  MMB_REQUIRE(3 * d + 2 * a_ + 2 * vd <= kSplitJ * kNT);  // the finish kernel's columns
  const StreamVec vec = stream_vec(s, fb, tb);
  MMB_REQUIRE(units_fit(s, vec));
  float* part = static_cast<float*>(ws);
  const int rc = table_type == MMB_TABLE_F32   ? split_route<float>(s, q, vec, frame_type, part, stream)
                 : table_type == MMB_TABLE_F16 ? split_route_f16(s, q, vec, frame_type, part, stream)
                                               : split_route_bf16(s, q, vec, frame_type, part, stream);
  return reduce_colmax(rc, s, static_cast<int>(n), colmax, stream);
}

extern "C" int mmb_mm2_stream_split(const int32_t* ids, const float* table, int64_t v,
                                    const float* wtab32, const float* text_dense,
                                    const float* emb_dense, const float* w_dense, const float* audio,
                                    const float* visual, int64_t n, int t, int d, int a_, int vd,
                                    float* num_out, void* s_out, int s_half, float* aux_out,
                                    int32_t* flag, uint32_t* colmax, void* colmax_ws, int parts,
                                    void* ws, size_t ws_bytes, hipStream_t stream) {
  return split_stream(MMB_TABLE_F32, MMB_FRAMES_F32, ids, table, v, wtab32, text_dense, emb_dense, w_dense, audio,
                      visual, n, t, d, a_, vd, num_out, s_out, s_half, aux_out, flag, colmax, colmax_ws, parts, ws,
                      ws_bytes, stream);
}

extern "C" int mmb_mm2_stream_split_ft(const int32_t* ids, const float* table, int64_t v, const float* wtab32,
                                       const float* w_dense, const void* audio, const void* visual,
                                       int frame_type, int64_t n, int t, int d, int a_, int vd, float* num_out,
                                       void* s_out, int s_half, float* aux_out, int32_t* flag, uint32_t* colmax,
                                       void* colmax_ws, int parts, void* ws, size_t ws_bytes,
                                       hipStream_t stream) {
  MMB_REQUIRE(frame_bytes(frame_type) != 0);
  MMB_REQUIRE(ids);  // gathered text only
  return split_stream(MMB_TABLE_F32, frame_type, ids, table, v, wtab32, nullptr, nullptr, w_dense, audio, visual, n, t,
                      d, a_, vd, num_out, s_out, s_half, aux_out, flag, colmax, colmax_ws, parts, ws, ws_bytes,
                      stream);
}

extern "C" int mmb_mm2_stream_split_tt(const int32_t* ids, const void* table, int table_type, int64_t v,
                                       const float* wtab32, const float* w_dense, const void* audio,
                                       const void* visual, int frame_type, int64_t n, int t, int d, int a_,
                                       int vd, float* num_out, void* s_out, int s_half, float* aux_out,
                                       int32_t* flag, uint32_t* colmax, void* colmax_ws, int parts, void* ws,
                                       size_t ws_bytes, hipStream_t stream) {
  MMB_REQUIRE(table_bytes(table_type) != 0 && frame_bytes(frame_type) != 0);
  MMB_REQUIRE(ids);  // gathered text only
  return split_stream(table_type, frame_type, ids, table, v, wtab32, nullptr, nullptr, w_dense, audio, visual, n, t,
                      d, a_, vd, num_out, s_out, s_half, aux_out, flag, colmax, colmax_ws, parts, ws, ws_bytes,
                      stream);
}

// the tools build's variant launches, knobs and probes (tools/diag/); the
// product library includes an empty header here
#ifndef MMB_TOOLS_TAIL_SIF
#define MMB_TOOLS_TAIL_SIF "mmb_no_tools.h"
#endif
#include MMB_TOOLS_TAIL_SIF
