// The MMB2 stream and its projection in one kernel: utt_fused_kernel and its
// launchers, shared by the sources that instantiate it -- one per pair of
// frame and word-table element types (fused_kernels.hip: f32 frames on an f32
// table, the entry points and the tools tail; fused_f16_kernels.hip,
// fused_bf16_kernels.hip: 16-bit frames on an f32 table; the six
// fused_t<table>_<frames>_kernels.hip: a 16-bit table), so that no
// translation unit compiles more fused kernels than the f32 one.  The
// template is instantiated for a given (FE, TE) in exactly one of them.
#pragma once
#include "mmb_stream.h"

namespace mmb {

// ---------------------------------------------------------------- fused step
// Stream + projection in ONE kernel (the bench step's MMB2 path): the frame
// sums s of an utterance never leave the chip.  One persistent workgroup per
// CU, 8 waves (two per SIMD):
//   waves 0-3 (streamers)  stream the utterances of a batch of 48 consecutive
//     rows modality by modality (text pass: gathered rows, the a2 row x, aux,
//     the column bounds; then the audio pass, then the visual pass), leaving
//     each (row, modality) piece of sums -- [Sx_m | Sxx_m], fp16 hi | lo of
//     the piece scaled by a power of two -- in an LDS ring slot
//   waves 4-7 (projectors) per piece of a batch: [48, 2 w_m] x [2 w_m, 320]
//     fp16 x3 products (v_mfma_f32_16x16x32_f16, 3 row tiles x 5 column tiles
//     per wave) with A from the ring and B straight from L2 (the piece-ordered
//     weight split, mmb_mm2_split_pieces); the accumulators carry over from
//     piece to piece (rescaled exactly by the ratio of the pieces' power-of-2
//     scales); after the third piece the epilogue of mm2_project_x3b_kernel
//     (text sum, total weight, L2 norm) on 80 columns per wave, the row totals
//     and norms exchanged through LDS
// Why piece-major 48-row batches: every batch re-reads the whole 2.3 MB weight
// image from L2, and that L2 traffic is what competes with the HBM stream
// (r02 ablation: 16-row whole-row batches -- 146 GB of L2 reads per 1M rows --
// took the kernel from 20.2 ms, stream alone, to 26.0 ms).  LDS cannot hold 48
// whole rows (7.3 KB each), but it holds 60 single-modality pieces (2.5 KB):
// the projectors read piece m of the batch while the streamers fill piece m+1.
// Hand-over through LDS counters (the two groups run at their own pace):
//   fill[p % 4]  piece-rows of piece p (= 3 batch + modality) written
//   consumed     projector waves done reading a piece (the streamers wait
//                before overwriting a slot)
//   pbar         the projectors' own exchange points (two per batch)
// Every wait is bounded: after ~0.5 s without progress it raises
// MMB_FLAG_SYNC_TIMEOUT and every later wait returns at once, so a broken
// hand-over ends the kernel (wrong rows, flagged) instead of hanging the GPU.
constexpr int kGR = 48;                 // rows per batch
constexpr int kGRT = kGR / 16;          // MFMA row tiles per batch
constexpr int kGSlots = 62;             // ring slots (piece-rows), at most (fused_lds_bytes)
constexpr int kGUnits = 80;             // 16-byte units per plane (piece <= 640 sums; XOR-16 headroom)
constexpr int kGPlane = kGUnits * 8;    // halves per plane
constexpr int kGSlot = 2 * kGPlane;     // halves per slot (hi | lo)
constexpr int kFTiles = 5;              // 16-column tiles per projector (ldw = 320)
constexpr int kFLdw = 320;
constexpr int kFThreads = 512;
// ring [SL slots] | irs [SL] | counters [8] | cnt, tw [2][48] each | tot [2][48] | ssq [2][4][48]
// | the dynamic schedule's batch and tag slots [8] each
__host__ __device__ constexpr size_t fused_lds_bytes(int sl) {
  return static_cast<size_t>(sl) * kGSlot * sizeof(_Float16) + sl * 4 + 8 * 4 + 2 * 2 * kGR * 4 +
         2 * kGR * 4 + 2 * 4 * kGR * 4 + 2 * 8 * 4;
}
static_assert(fused_lds_bytes(kGSlots) <= 160 * 1024, "fused ring exceeds LDS");
static_assert((kGSlot * 2) % 256 == 0 && (kGPlane * 2) % 256 == 0,
              "slot and plane strides keep the XOR swizzle conflict-free");

struct FusedArgs {
  StreamArgs s;
  const _Float16* img;     // piece-ordered B image (mmb_mm2_split_pieces), ldw = 320
  const float* col_inv;    // [320] 1 / column scale
  const float* c0;         // [320]
  float* out;              // mmb2 [N][D]
  int64_t nb;              // batches = ceil(N / 48)
  int kq[3];               // padded piece widths (multiples of 32)
  int balanced;            // rows past the last full round split evenly over the workgroups
  unsigned* sched;         // the launch's batch counter, zero at launch (nullable: static order)
  int64_t big, nu;         // dynamic order: units [0, big) are 48-row batches, the rest 12 rows
};

// the bounded waits' budget (tools/diag: a test shortens it to drive the
// timeout path)
#ifndef MMB_HOOK_FUSED_WAIT_ITERS
#define MMB_HOOK_FUSED_WAIT_ITERS (1 << 23)
#endif
__device__ __forceinline__ int fused_wait_iters() { return MMB_HOOK_FUSED_WAIT_ITERS; }

// bounded wait for *p >= target (workgroup scope); false once anything timed out
__device__ __forceinline__ bool fused_wait(int* p, int target, int* abort_flag, int32_t* gflag) {
  const int iters = fused_wait_iters();
  for (int it = 0; it < iters; ++it) {
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= target) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      return true;
    }
    if (__hip_atomic_load(abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return false;
    __builtin_amdgcn_s_sleep(2);
  }
  __hip_atomic_store(abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (gflag && (threadIdx.x & (kWave - 1)) == 0) atomicOr(gflag, MMB_FLAG_SYNC_TIMEOUT);
  return false;
}
// one increment per wave, ordered after this wave's earlier LDS / global writes
__device__ __forceinline__ void fused_signal(int* p) {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  if ((threadIdx.x & (kWave - 1)) == 0)
    __hip_atomic_fetch_add(p, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the same without waiting for this wave's global loads / stores (the
// pipelined streamer: its next frame groups stay in flight); the LDS writes it
// orders are complete before the increment (lgkmcnt), and LDS operations of
// one wave retire in order
__device__ __forceinline__ void fused_signal_lds(int* p) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if ((threadIdx.x & (kWave - 1)) == 0)
    __hip_atomic_fetch_add(p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// A column unit (4 values) of a frame or a word-table row as it is loaded: a
// float4, or of a 16-bit type the 8-byte unit, kept packed until it is summed.
template <class FE>
using frame_unit = std::conditional_t<std::is_same_v<FE, float>, float4, u2>;
template <bool NT, class FE>
__device__ __forceinline__ frame_unit<FE> ld_unit(const FE* p) {
  if constexpr (std::is_same_v<FE, float>) {
    return ldnt4<NT>(p);
  } else if constexpr (NT) {
    return __builtin_nontemporal_load(reinterpret_cast<const u2*>(p));
  } else {
    return *reinterpret_cast<const u2*>(p);
  }
}
template <class FE>
__device__ __forceinline__ float4 unit_f32x4(const frame_unit<FE>& q) {
  if constexpr (std::is_same_v<FE, float>) {
    return q;
  } else {
    return frame_f32x4<FE>(q);
  }
}

// Text piece of utterance i (one wave, lane l owns float4 columns l, l + 64):
// the weighted sum num = sum_t w_t E_t, Sx, Sxx of the gathered rows, the
// count of nonzero weights and their sum (utt_sums' text half).  TE: the word
// table's element type; a 16-bit row unit is one 8-byte load, kept packed
// until it is summed (gathered text only: dense text is f32).
template <int UNR, class TE = float>
__device__ __forceinline__ void text_piece(const StreamArgs& a, int64_t i, int lane, float4 (&num)[2],
                                           float4 (&sx)[2], float4 (&sxx)[2], float& cnt, float& sw) {
  const int UT = a.D >> 2;
  const TE* tsrc = frames<TE>(a.ids ? a.table : a.text_dense);
  const bool gather = a.ids != nullptr;
  int rid = -1;
  float w = 0.f;
  if (lane < a.L) {
    int64_t off;
    stage_token(a, i, lane, off, w);
    rid = off < 0 ? -1 : (gather ? static_cast<int>(off / a.D) : lane);
  }
  cnt = wave_sum((w != 0.f) ? 1.f : 0.f);
  sw = wave_sum_dpp_f32(w);  // DPP rows, as the pipelined streamers (bit-identical variants)
  if (lane == 0 && cnt == 0.f && a.flag) atomicOr(a.flag, MMB_FLAG_ZERO_WEIGHTS);
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int c = 0; c < 2; ++c) num[c] = sx[c] = sxx[c] = z4;
  const int64_t dbase = i * a.L;
  const int ct0 = 4 * min(lane, UT - 1), ct1 = 4 * min(lane + kWave, UT - 1);
  auto frame = [&](int t, frame_unit<TE> (&v)[2], float& wt, bool& ok) {
    const int r = __builtin_amdgcn_readlane(rid, t);
    wt = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), t));
    ok = r >= 0;
    const int64_t o = (gather ? static_cast<int64_t>(ok ? r : 0) : dbase + t) * a.D;
    v[0] = ld_unit<false>(tsrc + o + ct0);
    v[1] = ld_unit<false>(tsrc + o + ct1);
  };
  auto accum = [&](const frame_unit<TE> (&v)[2], float wt, bool ok) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      float4 x;
      if constexpr (std::is_same_v<TE, float>) {
        x = ok ? v[c] : z4;
      } else {  // (a 16-bit row unit: widened here)
        x = ok ? unit_f32x4<TE>(v[c]) : z4;
      }
      fma4(num[c], wt, x);
      add4(sx[c], x);
      sq4(sxx[c], x);
    }
  };
  int t = 0;
  for (; t + UNR <= a.L; t += UNR) {
    frame_unit<TE> v[UNR][2];
    float wt[UNR];
    bool ok[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) frame(t + u, v[u], wt[u], ok[u]);
#pragma unroll
    for (int u = 0; u < UNR; ++u) accum(v[u], wt[u], ok[u]);
  }
  for (; t + 4 <= a.L; t += 4) {  // tail groups: keep loads in flight
    frame_unit<TE> v[4][2];
    float wt[4];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) frame(t + u, v[u], wt[u], ok[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) accum(v[u], wt[u], ok[u]);
  }
  for (; t < a.L; ++t) {
    frame_unit<TE> v[2];
    float wt;
    bool ok;
    frame(t, v, wt, ok);
    accum(v, wt, ok);
  }
}

// Audio / visual piece: Sx, Sxx over the L frames [L][W] of FE at `base`
// (read-once streams: non-temporal loads).
template <int UNR, bool NT, class FE = float>
__device__ __forceinline__ void frame_piece(const FE* base, int W, int L, int lane,
                                            float4 (&sx)[2], float4 (&sxx)[2]) {
  const int UW = W >> 2;
  const int c0 = 4 * min(lane, UW - 1), c1 = 4 * min(lane + kWave, UW - 1);
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  sx[0] = sx[1] = sxx[0] = sxx[1] = z4;
  int t = 0;
  for (; t + UNR <= L; t += UNR) {
    frame_unit<FE> v[UNR][2];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      v[u][0] = ld_unit<NT>(base + static_cast<int64_t>(t + u) * W + c0);
      v[u][1] = ld_unit<NT>(base + static_cast<int64_t>(t + u) * W + c1);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float4 x = unit_f32x4<FE>(v[u][c]);
        add4(sx[c], x);
        sq4(sxx[c], x);
      }
  }
  for (; t + 4 <= L; t += 4) {  // tail groups: keep loads in flight
    frame_unit<FE> v[4][2];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      v[u][0] = ld_unit<NT>(base + static_cast<int64_t>(t + u) * W + c0);
      v[u][1] = ld_unit<NT>(base + static_cast<int64_t>(t + u) * W + c1);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float4 x = unit_f32x4<FE>(v[u][c]);
        add4(sx[c], x);
        sq4(sxx[c], x);
      }
  }
  for (; t < L; ++t) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float4 x = unit_f32x4<FE>(ld_unit<NT>(base + static_cast<int64_t>(t) * W + (c ? c1 : c0)));
      add4(sx[c], x);
      sq4(sxx[c], x);
    }
  }
}

// The pipelined streamers' frame loads (one frame of a group in flight; the
// group's storage is a float4 and a float per frame whatever the piece, since
// a piece's tail prefetches the next piece's first group into it):
//   f32 rows (text of an f32   one b128 load (lane l: columns 4 l .. 4 l + 3)
//   table or dense, frames)    and, TAIL, one b32 load of column 256 + l
//   16-bit rows (text of a     one b64 load of the same four columns, held
//   16-bit table, frames)      packed in va.x | va.y, and, TAIL, one b16 load
//                              held zero-extended in vb
// o0 / o1 are the lane's byte offsets of the two loads, so the frame's (a
// scalar).  Both loads clamp their column to the row's last, share the
// descriptor, the scalar row offset and the cache policy; the loads per frame
// are the same for every FE and TE, and with them the counted vmcnt waits.
// (The text of a 16-bit table TE is gathered: dense text is f32, and the
// entry point hands a TE kernel ids.)
template <class FE, bool TEXT, class TE = float>
constexpr int kFrameBytes = std::is_same_v<std::conditional_t<TEXT, TE, FE>, float> ? 4 : 2;
// an element of that many bytes: what a row's buffer descriptor is based on
// (a typed row pointer, not bytes: the f32 instantiations keep their code)
template <int BYTES>
using frame_row_t = std::conditional_t<BYTES == 4, float, uint16_t>;
template <class FE, bool TEXT, bool TAIL, int POL, class TE = float, class R>
__device__ __forceinline__ void load_frame(R rsrc, int o0, int o1, int so, float4& va, float& vb) {
  if constexpr (kFrameBytes<FE, TEXT, TE> == 4) {
    va = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, o0, so, POL));
    if constexpr (TAIL) vb = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, o1, so, POL));
  } else {
    const u2 q = __builtin_bit_cast(u2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, o0, so, POL));
    va.x = __uint_as_float(q.x);
    va.y = __uint_as_float(q.y);
    if constexpr (TAIL)
      vb = __uint_as_float(static_cast<uint32_t>(
          __builtin_bit_cast(uint16_t, __builtin_amdgcn_raw_buffer_load_b16(rsrc, o1, so, POL))));
  }
}
// what load_frame left of a frame (FE) or a table row (TE), widened (exactly) to f32
template <class FE>
__device__ __forceinline__ float4 group_f32x4(const float4& va) {
  if constexpr (std::is_same_v<FE, float>) {
    return va;
  } else {
    return frame_f32x4<FE>(u2{__float_as_uint(va.x), __float_as_uint(va.y)});
  }
}
template <class FE>
__device__ __forceinline__ float group_f32(float vb) {
  if constexpr (std::is_same_v<FE, float>) {
    return vb;
  } else {
    return frame_f32<FE>(__float_as_uint(vb));
  }
}

// DIAG (timing-only builds, MMB_FUSED_DIAG; wrong MMB2 rows): bit 7 the
// epilogue without its x re-read, bit 8 without its MMB2 stores; bit 4 every B
// chunk read from the piece's first chunk, bit 5 no B loads; bit 0 the
// projectors only hand the slots back (no loads, MFMAs or epilogue), bit 1
// no MFMAs (B loads kept live), bit 2 no epilogue, bit 3 the streamers skip
// the frames (constant sums: the projectors alone)
// per-workgroup wall-clock marks of the fused kernel (tools/diag defines
// them: mmb_diag_fused_probe)
#ifndef FUSED_PROBE
#define FUSED_PROBE(slot) \
  do {                    \
  } while (0)
#endif

// TM (the pipelined streamers): bit m set = piece m's rows are wider than 256
// columns and carry a tail load and tail sums (fused_tail_mask); a set bit on
// a narrower piece only costs redundant loads, the results are the same.
// FE: the element type of the audio / visual frames (float, f16_t, bf16_t;
// a.audio and a.visual are then read through const FE*).  The 16-bit units
// are widened exactly where a frame is summed, and the sums' statements are
// the f32 instantiation's in their order: a launch on 16-bit frames writes,
// bit for bit, what the same launch writes on those frames upcast to f32.
// TE: the element type of the word table (a.table is then read through
// const TE*; gathered text only).  A 16-bit row travels as the 16-bit frames
// do -- the same two loads, packed until summed, the exact widening -- so the
// same equality holds for the table upcast to f32, for each FE.
template <int UNR, bool NT, int DIAG = 0, int PIPE = 0, int SL = kGSlots, int TM = 7, class FE = float,
          class TE = float>
__global__ __launch_bounds__(kFThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void utt_fused_kernel(
    FusedArgs f) {
  const StreamArgs& a = f.s;
  extern __shared__ __attribute__((aligned(16))) _Float16 flds[];
  _Float16* ring = flds;
  float* s_irs = reinterpret_cast<float*>(flds + SL * kGSlot);
  int* ctr = reinterpret_cast<int*>(s_irs + SL);   // fill[4], consumed, pbar, abort, -
  float* s_cnt = reinterpret_cast<float*>(ctr + 8);     // [2][48]
  float* s_tw = s_cnt + 2 * kGR;                        // [2][48]
  float* s_tot = s_tw + 2 * kGR;                        // [2][48]
  float* s_ssq = s_tot + 2 * kGR;                       // [2][4][48]
  int* s_bat = reinterpret_cast<int*>(s_ssq + 2 * 4 * kGR);  // [8] global batch of local batch j (slot j & 7)
  int* s_tag = s_bat + 8;                                // [8] j + 1 once slot j & 7 holds batch j
  int* fill = ctr;
  int* consumed = ctr + 4;
  int* pbar = ctr + 5;
  int* abort_flag = ctr + 6;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  if (tid < 8) {
    ctr[tid] = 0;
    s_tag[tid] = 0;
  }
  if (tid == 0) FUSED_PROBE(0);
  __syncthreads();
  const int64_t N = a.N;
  const int G = gridDim.x;
  const int D = a.D;
  // This workgroup's batches of 48 rows: batch blockIdx.x + j G of the row
  // space (round robin: the CUs stream neighbouring rows -- contiguous
  // per-CU ranges measured 23.07 vs 22.32 ms).  With f.balanced the rows
  // past the last full round (N mod 48 G) are split evenly over the
  // workgroups instead of being whole batches of a few of them (a CU with
  // one batch more than another runs ~0.28 ms longer).
  const int64_t full = N / (static_cast<int64_t>(kGR) * G);  // full rounds
  // Dynamic schedule (r05; the pipelined streamer with a counter): local
  // batch j is whatever global batch the streamers' wave 0 drew from the
  // launch's counter for it (one batch ahead of its own use), so a CU that
  // streams faster takes more batches.  The static round robin left the
  // workgroups' finishing times 0.3-0.7 ms apart at 1M rows (the even XCDs
  // slower; tools/fused_balance.py, gpurun_out r05ab).  Neighbouring CUs
  // still draw neighbouring batches.
  const bool dyn = PIPE == 2 && f.sched != nullptr;
  auto batch = [&](int64_t j, int64_t& row0, int64_t& rend) -> bool {
    if (dyn) {
      int64_t u = blockIdx.x + j * G;  // local batches 0 and 1: the round robin's units
      if (j >= 2) {
        if (!fused_wait(&s_tag[j & 7], static_cast<int>(j) + 1, abort_flag, a.flag)) return false;
        u = s_bat[j & 7];
      }
      if (u >= f.nu) return false;
      // the last round's worth of rows in quarter batches: the end of the
      // kernel waits for one 12-row unit, not one 48-row batch (~0.3 ms)
      row0 = u < f.big ? u * kGR : f.big * kGR + (u - f.big) * (kGR / 4);
      rend = min<int64_t>(N, row0 + (u < f.big ? kGR : kGR / 4));
      return true;
    }
    if (f.balanced && j >= full) {
      if (j > full) return false;
      const int64_t t0 = full * kGR * G, tail = N - t0, b = blockIdx.x;
      const int64_t per = tail / G, rem = tail % G;
      row0 = t0 + b * per + (b < rem ? b : rem);
      rend = row0 + per + (b < rem ? 1 : 0);
      return row0 < rend;
    }
    const int64_t Bj = blockIdx.x + j * G;
    row0 = Bj * kGR;
    rend = min<int64_t>(N, row0 + kGR);
    return Bj < f.nb;
  };

  if (wave < 4) {
    // ------------------------------------------------------------ streamer
    const int wdt[3] = {a.D, a.A, a.Vd};
    float4 cmx[2];
    cmx[0] = cmx[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    float cmt = 0.f;  // the pipelined streamers' bound of column 256 + lane (in place of cmx[1])
    // Row q (utterance i) of batch j, modality m summed: its power-of-2 scale,
    // the text row's x / aux / column bounds, then the scaled fp16 hi | lo
    // sums into the ring slot (once the slot's previous piece-row was read by
    // every projector) and one fill increment.  DRAIN: the increment waits for
    // every earlier global access of this wave (the group-at-a-time streamer);
    // the pipelined streamer waits only for its LDS writes, its next loads
    // stay in flight (its x / aux stores are drained once per batch, before
    // the audio piece's first increment -- the projectors read x only after
    // the visual piece).
    //
    // TL, the layout of a row's columns from 256 on (num1 / sx1 / sxx1): 2 =
    // a second float4 per lane, columns 4 (64 + lane) (the group-at-a-time
    // streamer), 1 = one float per lane, column 256 + lane (the pipelined
    // streamers), 0 = the piece has no such columns (W <= 256; the arguments
    // are unused).  Lanes past the row's end hold a clamped duplicate in
    // either layout: the row maximum is the same, and nothing of them is
    // stored.  The ring positions written are the same in all three.
    auto finish_row = [&](auto drain_c, auto tl_c, int64_t j, int m, int q, int64_t i, const float4& num0,
                          const float4& sx0, const float4& sxx0, auto num1, auto sx1, auto sxx1,
                          float cnt, float sw) {
      constexpr int TL = decltype(tl_c)::value;
      const int W = wdt[m], U = W >> 2;
      const int p = 3 * static_cast<int>(j) + m;  // piece sequence number
      float mx = fmaxf(0.f, fmaxf(amax4(sx0), amax4(sxx0)));
      if constexpr (TL == 2) mx = fmaxf(mx, fmaxf(amax4(sx1), amax4(sxx1)));
      if constexpr (TL == 1) mx = fmaxf(mx, fmaxf(fabsf(sx1), fabsf(sxx1)));
      const float rs = row_scale(wave_max_dpp_f32(mx));
      if (m == 0) {
        if (lane < U) {
          const float4 xr = div4(num0, cnt);
          st4(a.num_out + i * D + 4 * lane, xr);  // x = the a2 row
          cmx[0] = bmax4(cmx[0], xr);
        }
        if constexpr (TL == 2) {
          if (lane + kWave < U) {
            const float4 xr = div4(num1, cnt);
            st4(a.num_out + i * D + 4 * (lane + kWave), xr);
            cmx[1] = bmax4(cmx[1], xr);
          }
        }
        if constexpr (TL == 1) {
          if (4 * kWave + lane < W) {
            const float xr = num1 / cnt;
            a.num_out[i * D + 4 * kWave + lane] = xr;
            cmt = bmax(cmt, fabsf(xr));
          }
        }
        if (lane == 0) {
          a.aux_out[i] = cnt;  // planar [3][N]: count | sum w | text-piece scale
          a.aux_out[N + i] = sw;
          a.aux_out[2 * N + i] = rs;
          s_cnt[(j & 1) * kGR + q] = cnt;
          s_tw[(j & 1) * kGR + q] = sw;
        }
      }
      // the slot's previous piece-row (pos - 60) must have been read by every projector
      const int pos = p * kGR + q;
      const int slot = pos % SL;
      // (DIAG 64, timing only: never wait -- the ring's back-pressure removed)
      if ((DIAG & 64) == 0 && pos >= SL)
        fused_wait(consumed, ((pos - SL) / kGR + 1) * 4, abort_flag, a.flag);
      _Float16* srow = ring + slot * kGSlot;
      const int qx = q & 15;  // row within its MFMA row tile: the XOR swizzle key
      auto put = [&](int k, float4 v) {
        const float x4[4] = {v.x * rs, v.y * rs, v.z * rs, v.w * rs};
        h4 h, l;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          h[e] = static_cast<_Float16>(x4[e]);
          l[e] = static_cast<_Float16>(x4[e] - static_cast<float>(h[e]));
        }
        const int o = (((k >> 3) ^ qx) << 3) + (k & 7);
        *reinterpret_cast<h4*>(srow + o) = h;
        *reinterpret_cast<h4*>(srow + kGPlane + o) = l;
      };
      // one column's hi and lo halves, at the position put() gives it
      auto put1 = [&](int k, float v) {
        const float x = v * rs;
        const _Float16 h = static_cast<_Float16>(x);
        const int o = (((k >> 3) ^ qx) << 3) + (k & 7);
        srow[o] = h;
        srow[kGPlane + o] = static_cast<_Float16>(x - static_cast<float>(h));
      };
      if (lane < U) {
        put(4 * lane, sx0);
        put(W + 4 * lane, sxx0);
      }
      if constexpr (TL == 2) {
        if (lane + kWave < U) {
          put(4 * (lane + kWave), sx1);
          put(W + 4 * (lane + kWave), sxx1);
        }
      }
      if constexpr (TL == 1) {
        if (4 * kWave + lane < W) {
          put1(4 * kWave + lane, sx1);
          put1(W + 4 * kWave + lane, sxx1);
        }
      }
      for (int k = 2 * W + 4 * lane; k < f.kq[m]; k += 4 * kWave) put(k, make_float4(0.f, 0.f, 0.f, 0.f));
      if (lane == 0) s_irs[slot] = 1.f / rs;  // a power of two: exact
      if constexpr (decltype(drain_c)::value) {
        fused_signal(&fill[p & 3]);
      } else {
        fused_signal_lds(&fill[p & 3]);
      }
    };

    if constexpr (PIPE == 0) {
      for (int64_t j = 0;; ++j) {
        int64_t row0, rend;
        if (!batch(j, row0, rend)) break;
#pragma unroll 1
        for (int m = 0; m < 3; ++m) {
          const int W = wdt[m];
#pragma unroll 1
          for (int r = 0; r < kGR / 4; ++r) {
            const int q = wave + 4 * r;
            const int64_t i = row0 + q;
            if (i >= rend) break;
            float4 num[2], sx[2], sxx[2];
            float cnt = 0.f, sw = 0.f;
            if constexpr ((DIAG & 8) != 0) {
              const float4 o4 = make_float4(1.f, 1.f, 1.f, 1.f);
              num[0] = num[1] = sx[0] = sx[1] = sxx[0] = sxx[1] = o4;
              cnt = sw = 1.f;
            } else if (m == 0) {
              text_piece<UNR, TE>(a, i, lane, num, sx, sxx, cnt, sw);
            } else {
              const FE* base = m == 1 ? frames<FE>(a.audio) + i * a.L * a.A : frames<FE>(a.visual) + i * a.L * a.Vd;
              frame_piece<UNR, NT, FE>(base, W, a.L, lane, sx, sxx);
            }
            finish_row(std::true_type{}, std::integral_constant<int, 2>{}, j, m, q, i, num[0], sx[0], sxx[0],
                       num[1], sx[1], sxx[1], cnt, sw);
          }
        }
      }
    } else {
      // Pipelined streamer: the (row, frame group) sequence of one (batch,
      // modality) piece -- this wave's rows i0 + 4 r, ceil(L / UNR) groups of
      // UNR frames each -- as ONE load pipeline two groups deep: group g + 1's
      // UNR or 2 UNR loads are issued before group g is summed (alternating register
      // sets b0 / b1; the compiler's counted vmcnt waits only for the older
      // group), so loads stay in flight across group and row boundaries where
      // the group-at-a-time streamer drained them.  Text rows: row r + 1's ids
      // are loaded while row r's first group is summed, its weights gathered
      // (wtab[id]) at the second -- the next row's first group is issued after
      // that (>= 3 groups per row, launch_fused).  Per lane the frames are
      // summed in the same order as text_piece / frame_piece: bit-identical.
      // (A pipeline running on across piece and batch boundaries, one issue /
      // consume pair for all three modalities, measured 29.4 vs 22.1 ms: the
      // shared register sets made the compiler drain every group, vmcnt(0).)
      const bool gather = a.ids != nullptr;  // (always, of a 16-bit table: dense text is f32)
      const int L = a.L;
      // the wave index made visibly wave-uniform (SGPR): rows, loop bounds and
      // buffer descriptors derive from it (a descriptor in VGPRs would be
      // waterfall-looped around every load)
      const int uw = __builtin_amdgcn_readfirstlane(wave);
      auto tok_issue = [&](int64_t i, int& raw, float& wd) {
        raw = -1;
        wd = 0.f;
        if (lane < L) {
          const int64_t ft = i * L + lane;
          if (gather) raw = a.ids[ft];
          if (a.w_dense) wd = a.w_dense[ft];
        }
      };
      auto tok_resolve = [&](int raw, float wd, int& rid, float& w) {  // stage_token's semantics
        rid = -1;
        w = 0.f;
        if (lane < L) {
          if (gather) {
            int64_t id = raw;
            w = a.w_dense ? wd : ((id >= 0 && id < a.V) ? a.wtab[id] : 0.f);
            if (id < 0) id += a.V;
            if (id < 0 || id >= a.V) {
              if (a.flag) atomicOr(a.flag, MMB_FLAG_ID_RANGE);
              w = 0.f;
            } else {
              rid = static_cast<int>(id);
            }
          } else {
            w = wd;
            rid = lane;
          }
        }
      };
      // A frame group in flight: per frame one b128 load (lane l: columns 4 l
      // .. 4 l + 3) and, where the piece is wider than 256 columns (TM bit m),
      // one b32 load of column 256 + l -- 5 VGPRs per frame where two b128
      // loads took 8, 3 of them dead on the 300-wide rows' 53 clamped lanes.
      // Widths are <= 320 (mmb_mm2_stream_project_supported): 64 tail lanes
      // suffice.  Both loads clamp their column to the row's last (no exec
      // masking: the masked second load measured slower, below), share the
      // descriptor, the scalar row offset and the cache policy.  On 16-bit
      // frames (FE) the two loads of an audio / visual frame are a b64 and a
      // b16 (load_frame): 3 VGPRs per frame, in the same storage.
      struct Grp {
        float4 a[UNR];
        float b[UNR];
      };
      static_assert(4 * UNR + 8 < 64, "two groups of two loads per frame and a row's stores fit vmcnt's 6 bits");
      auto piece = [&](auto m_c, int64_t j, int64_t i0, int nrows) {
        constexpr int m = decltype(m_c)::value;
        constexpr bool TEXT = m == 0;
        constexpr bool TAIL = ((TM >> m) & 1) != 0;
        const int W = wdt[m], UW = W >> 2;
        const int ngr = (L + UNR - 1) / UNR, ng = nrows * ngr;
        const void* src = TEXT ? (gather ? a.table : a.text_dense) : (m == 1 ? a.audio : a.visual);
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        int cur = 0;                        // the row being summed
        int rid_c = -1, rid_n = -1, raw_n = -1;
        float w_c = 0.f, w_n = 0.f, wd_n = 0.f;
        float4 num, sx, sxx;
        float numt = 0.f, sxt = 0.f, sxxt = 0.f;  // column 256 + lane
        float cnt = 0.f, sw = 0.f;
        if constexpr (TEXT) {
          int raw;
          float wd;
          tok_issue(i0, raw, wd);
          tok_resolve(raw, wd, rid_c, w_c);
        }
        // loads through buffer descriptors: one scalar offset per frame (the
        // gathered row's or the frame's), per-lane column offsets vo0 / vo1 --
        // no 64-bit address arithmetic in VGPRs.  (The second column load
        // issued on its 11 live lanes only, the others zeroed, measured 23.37
        // vs 22.24 ms: the divergent branch costs more than the clamped
        // duplicate addresses, which the L1 coalesces.)
        constexpr int EB = kFrameBytes<FE, TEXT, TE>;  // bytes per element of this piece's rows
        using RowE = frame_row_t<EB>;
        const int vo0 = 4 * EB * min(lane, UW - 1), vo1 = EB * min(4 * kWave + lane, W - 1);
        auto issue = [&](int g, Grp& v) {
          const int rr = g / ngr, t0 = (g - rr * ngr) * UNR;
          const int64_t i = i0 + 4 * rr;
          int rid = 0;
          if constexpr (TEXT) rid = rr == cur ? rid_c : rid_n;
          const bool rowbase = !TEXT || !gather;  // frames [L][W] of row i
          const RowE* rsrc_base = frames<RowE>(src);
          const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(
              const_cast<RowE*>(rowbase ? rsrc_base + i * L * W : rsrc_base), 0,
              rowbase ? L * W * EB : static_cast<int>(a.V * D * EB), 0x00020000);
#pragma unroll
          for (int u = 0; u < UNR; ++u) {
            const int t = min(t0 + u, L - 1);
            int so;
            if constexpr (TEXT) {
              const int r = __builtin_amdgcn_readlane(rid, t);
              so = gather ? (r >= 0 ? r : 0) * D * EB : t * W * EB;
            } else {
              so = t * W * EB;
            }
            constexpr int pol = (!TEXT && NT) ? 2 : 0;  // non-temporal frame streams
            load_frame<FE, TEXT, TAIL, pol, TE>(rsrc, vo0, vo1, so, v.a[u], v.b[u]);
          }
        };
        auto sum_frame = [&](int t, const float4& va, float vb) {
          if constexpr (TEXT) {
            const int r = __builtin_amdgcn_readlane(rid_c, t);
            const float wt = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w_c), t));
            const bool ok = r >= 0;  // an out-of-range id (flagged) contributes a zero row
            float4 x;
            if constexpr (std::is_same_v<TE, float>) {
              x = ok ? va : z4;
            } else {  // (a 16-bit row: the packed unit widened here)
              x = ok ? group_f32x4<TE>(va) : z4;
            }
            fma4(num, wt, x);
            add4(sx, x);
            sq4(sxx, x);
            if constexpr (TAIL) {
              float xt;
              if constexpr (std::is_same_v<TE, float>) {
                xt = ok ? vb : 0.f;
              } else {
                xt = ok ? group_f32<TE>(vb) : 0.f;
              }
              numt = fmaf(wt, xt, numt);
              sxt += xt;
              sxxt = fmaf(xt, xt, sxxt);
            }
          } else {  // (16-bit frames: the packed unit and tail widened here)
            const float4 x = group_f32x4<FE>(va);
            add4(sx, x);
            sq4(sxx, x);
            if constexpr (TAIL) {
              const float xt = group_f32<FE>(vb);
              sxt += xt;
              sxxt = fmaf(xt, xt, sxxt);
            }
          }
        };
        auto consume = [&](int g, const Grp& v) {
          const int rr = g / ngr, gg = g - rr * ngr, t0 = gg * UNR;
          if (gg == 0) {
            num = sx = sxx = z4;
            numt = sxt = sxxt = 0.f;
            if constexpr (TEXT) {
              cnt = static_cast<float>(__builtin_popcountll(__builtin_amdgcn_ballot_w64(w_c != 0.f)));
              sw = wave_sum_dpp_f32(w_c);
              // every weight 0: x is 0/0 = NaN (numpy's answer); TruncatedSVD
              // would reject the split -- report it through the flag word
              if (lane == 0 && cnt == 0.f && a.flag) atomicOr(a.flag, MMB_FLAG_ZERO_WEIGHTS);
              if (rr + 1 < nrows) tok_issue(i0 + 4 * (rr + 1), raw_n, wd_n);
            }
          }
          if constexpr (TEXT) {
            if (gg == 1 && rr + 1 < nrows) tok_resolve(raw_n, wd_n, rid_n, w_n);
          }
          if (t0 + UNR <= L) {
#pragma unroll
            for (int u = 0; u < UNR; ++u) sum_frame(t0 + u, v.a[u], TAIL ? v.b[u] : 0.f);
          } else {
#pragma unroll
            for (int u = 0; u < UNR; ++u)
              if (t0 + u < L) sum_frame(t0 + u, v.a[u], TAIL ? v.b[u] : 0.f);
          }
          if (gg == ngr - 1) {
            const int q = uw + 4 * rr;
            finish_row(std::false_type{}, std::integral_constant<int, TAIL ? 1 : 0>{}, j, m, q, i0 + 4 * rr, num,
                       sx, sxx, numt, sxt, sxxt, cnt, sw);
            cur = rr + 1;
            if constexpr (TEXT) {
              rid_c = rid_n;
              w_c = w_n;
            }
          }
        };
        Grp b0, b1;
        issue(0, b0);
        int g = 0;
#pragma unroll 1
        for (; g + 2 < ng; g += 2) {
          issue(g + 1, b1);
          consume(g, b0);
          issue(g + 2, b0);
          consume(g + 1, b1);
        }
        if (g + 1 < ng) {
          issue(g + 1, b1);
          consume(g, b0);
          consume(g + 1, b1);
        } else {
          consume(g, b0);
        }
      };
      // PIPE == 2: the same pipeline, and each piece's tail also issues the
      // NEXT piece's first group (text -> audio -> visual -> the next batch's
      // text) once its own next-to-last group is summed, so loads stay in
      // flight across piece and batch boundaries too; the next batch's first
      // text row is staged during the visual piece's last groups.  Pieces with
      // an odd group count drain as before.
      Grp pb0, pb1;
      bool pre = false;  // pb0 holds this piece's group 0 (issued by the previous piece)
      int rid_pre = -1, raw_p = -1;
      float w_pre = 0.f, wd_p = 0.f;
      auto piece2 = [&](auto m_c, int64_t j, int64_t i0, int nrows, int64_t ni0, int nnr) {
        constexpr int M = decltype(m_c)::value;
        constexpr bool TEXT = M == 0;
        constexpr bool TAIL = ((TM >> M) & 1) != 0;
        const int W = wdt[M], UW = W >> 2;
        const int ngr = (L + UNR - 1) / UNR, ng = nrows * ngr;
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool has_next = M < 2 || nnr > 0;
        if constexpr (M == 2) {
          // the text piece's x / aux stores complete before any visual
          // increment (the projectors read x after the visual piece): with
          // group 0 in flight the newest operations are its loads, one or
          // two per frame
          if (pre) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(UNR * (TAIL ? 2 : 1)) : "memory");
          } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          }
        }
        int cur = 0;
        int rid_c = -1, rid_n = -1, raw_n = -1;
        float w_c = 0.f, w_n = 0.f, wd_n = 0.f;
        float4 num, sx, sxx;
        float numt = 0.f, sxt = 0.f, sxxt = 0.f;  // column 256 + lane
        float cnt = 0.f, sw = 0.f;
        if constexpr (TEXT) {
          if (pre) {
            rid_c = rid_pre;
            w_c = w_pre;
          } else {
            int raw;
            float wd;
            tok_issue(i0, raw, wd);
            tok_resolve(raw, wd, rid_c, w_c);
          }
        }
        constexpr int EB = kFrameBytes<FE, TEXT, TE>;  // bytes per element of this piece's rows
        const int vo0 = 4 * EB * min(lane, UW - 1), vo1 = EB * min(4 * kWave + lane, W - 1);
        // group g of this piece (or, NX, group 0 of the next piece) into v
        auto load_group = [&](auto nx_c, int g, Grp& v) {
          constexpr bool NX = decltype(nx_c)::value;
          constexpr int MM = NX ? (M + 1) % 3 : M;
          constexpr bool T2 = MM == 0;
          constexpr bool TAIL2 = ((TM >> MM) & 1) != 0;
          constexpr int E2 = kFrameBytes<FE, T2, TE>;
          const int rr = NX ? 0 : g / ngr, t0 = NX ? 0 : (g - rr * ngr) * UNR;
          const int64_t i = NX ? (M == 2 ? ni0 : i0) : i0 + 4 * rr;
          const int W2 = wdt[MM], U2 = W2 >> 2;
          const void* s2 = T2 ? (gather ? a.table : a.text_dense) : (MM == 1 ? a.audio : a.visual);
          const int o0 = NX ? 4 * E2 * min(lane, U2 - 1) : vo0, o1 = NX ? E2 * min(4 * kWave + lane, W2 - 1) : vo1;
          int rid = 0;
          if constexpr (T2) rid = NX ? rid_pre : (rr == cur ? rid_c : rid_n);
          const bool rowbase = !T2 || !gather;
          using Row2 = frame_row_t<E2>;
          const Row2* r2 = frames<Row2>(s2);
          const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(
              const_cast<Row2*>(rowbase ? r2 + i * L * W2 : r2), 0,
              rowbase ? L * W2 * E2 : static_cast<int>(a.V * D * E2), 0x00020000);
#pragma unroll
          for (int u = 0; u < UNR; ++u) {
            const int t = min(t0 + u, L - 1);
            int so;
            if constexpr (T2) {
              const int r = __builtin_amdgcn_readlane(rid, t);
              so = gather ? (r >= 0 ? r : 0) * D * E2 : t * W2 * E2;
            } else {
              so = t * W2 * E2;
            }
            constexpr int pol = (!T2 && NT) ? 2 : 0;  // non-temporal frame streams
            load_frame<FE, T2, TAIL2, pol, TE>(rsrc, o0, o1, so, v.a[u], v.b[u]);
          }
        };
        auto issue = [&](int g, Grp& v) { load_group(std::false_type{}, g, v); };
        auto sum_frame = [&](int t, const float4& va, float vb) {
          if constexpr (TEXT) {
            const int r = __builtin_amdgcn_readlane(rid_c, t);
            const float wt = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w_c), t));
            const bool ok = r >= 0;  // an out-of-range id (flagged) contributes a zero row
            float4 x;
            if constexpr (std::is_same_v<TE, float>) {
              x = ok ? va : z4;
            } else {  // (a 16-bit row: the packed unit widened here)
              x = ok ? group_f32x4<TE>(va) : z4;
            }
            fma4(num, wt, x);
            add4(sx, x);
            sq4(sxx, x);
            if constexpr (TAIL) {
              float xt;
              if constexpr (std::is_same_v<TE, float>) {
                xt = ok ? vb : 0.f;
              } else {
                xt = ok ? group_f32<TE>(vb) : 0.f;
              }
              numt = fmaf(wt, xt, numt);
              sxt += xt;
              sxxt = fmaf(xt, xt, sxxt);
            }
          } else {  // (16-bit frames: the packed unit and tail widened here)
            const float4 x = group_f32x4<FE>(va);
            add4(sx, x);
            sq4(sxx, x);
            if constexpr (TAIL) {
              const float xt = group_f32<FE>(vb);
              sxt += xt;
              sxxt = fmaf(xt, xt, sxxt);
            }
          }
        };
        auto consume = [&](int g, const Grp& v) {
          const int rr = g / ngr, gg = g - rr * ngr, t0 = gg * UNR;
          if (gg == 0) {
            num = sx = sxx = z4;
            numt = sxt = sxxt = 0.f;
            if constexpr (TEXT) {
              cnt = static_cast<float>(__builtin_popcountll(__builtin_amdgcn_ballot_w64(w_c != 0.f)));
              sw = wave_sum_dpp_f32(w_c);
              // every weight 0: x is 0/0 = NaN (numpy's answer); TruncatedSVD
              // would reject the split -- report it through the flag word
              if (lane == 0 && cnt == 0.f && a.flag) atomicOr(a.flag, MMB_FLAG_ZERO_WEIGHTS);
              if (rr + 1 < nrows) tok_issue(i0 + 4 * (rr + 1), raw_n, wd_n);
            }
          }
          if constexpr (TEXT) {
            if (gg == 1 && rr + 1 < nrows) tok_resolve(raw_n, wd_n, rid_n, w_n);
          }
          if constexpr (M == 2) {  // the next batch's first text row
            if (has_next && ng >= 4 && g == ng - 4) tok_issue(ni0, raw_p, wd_p);
            if (has_next && ng >= 4 && g == ng - 3) tok_resolve(raw_p, wd_p, rid_pre, w_pre);
          }
          if (t0 + UNR <= L) {
#pragma unroll
            for (int u = 0; u < UNR; ++u) sum_frame(t0 + u, v.a[u], TAIL ? v.b[u] : 0.f);
          } else {
#pragma unroll
            for (int u = 0; u < UNR; ++u)
              if (t0 + u < L) sum_frame(t0 + u, v.a[u], TAIL ? v.b[u] : 0.f);
          }
          if (gg == ngr - 1) {
            const int q = uw + 4 * rr;
            finish_row(std::false_type{}, std::integral_constant<int, TAIL ? 1 : 0>{}, j, M, q, i0 + 4 * rr, num,
                       sx, sxx, numt, sxt, sxxt, cnt, sw);
            cur = rr + 1;
            if constexpr (TEXT) {
              rid_c = rid_n;
              w_c = w_n;
            }
          }
        };
        if (!pre) issue(0, pb0);
        int g = 0;
#pragma unroll 1
        for (; g + 2 < ng; g += 2) {
          issue(g + 1, pb1);
          consume(g, pb0);
          issue(g + 2, pb0);
          consume(g + 1, pb1);
        }
        if (g + 1 < ng) {
          issue(g + 1, pb1);
          consume(g, pb0);
          if (has_next) {
            if constexpr (M == 2) {
              if (ng < 4) {  // too few groups to stage the tokens on the way
                tok_issue(ni0, raw_p, wd_p);
                tok_resolve(raw_p, wd_p, rid_pre, w_pre);
              }
            }
            load_group(std::true_type{}, 0, pb0);
          }
          consume(g + 1, pb1);
          pre = has_next;
        } else {
          consume(g, pb0);
          pre = false;
        }
      };
      // Local batches 0 and 1 are the round robin's units (every workgroup
      // drawing at once at the start queued 512 atomics on one word); from 2
      // on, streamer wave 0 draws local batch j + 2's unit at the top of batch
      // j and publishes it after the batch's text piece, so the atomic's
      // return is not waited for where it is issued; the other waves need it
      // at the top of batch j + 1, the projectors later still
      unsigned drawn = 0;
      auto draw_issue = [&]() {
        if (dyn && uw == 0 && lane == 0)
          drawn = __hip_atomic_fetch_add(f.sched, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      };
      auto draw_commit = [&](int64_t j) {  // publishes local batch j + 2
        if (dyn && uw == 0 && lane == 0) {
          const unsigned b = 2u * G + drawn;
          s_bat[(j + 2) & 7] = static_cast<int>(b < 0x7fffffffu ? b : 0x7fffffffu);
          __hip_atomic_store(&s_tag[(j + 2) & 7], static_cast<int>(j) + 3, __ATOMIC_RELEASE,
                             __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      };
      auto rows_of = [&](int64_t jb, int64_t& i0) -> int {
        int64_t row0, rend;
        if (!batch(jb, row0, rend)) {
          i0 = 0;
          return dyn ? -1 : 0;  // (dynamic: -1 = no batch, 0 = a batch without this wave's rows)
        }
        i0 = row0 + uw;
        return i0 < rend ? static_cast<int>(min<int64_t>(kGR / 4, (rend - i0 + 3) / 4)) : 0;
      };
      // dynamic order: every wave counts kGR / 4 fill increments per piece,
      // its rows' and the rest as padding after them, so the projectors'
      // targets stay kGR per piece whatever the unit's rows (a 12-row unit
      // followed by more units would otherwise leave the next targets short)
      auto pad = [&](int64_t j, int m, int nrows) {
        if (dyn && nrows < kGR / 4 && lane == 0) {
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __hip_atomic_fetch_add(&fill[(3 * static_cast<int>(j) + m) & 3], kGR / 4 - nrows, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      };
      if constexpr (PIPE == 2) {
        int64_t i0, ni0;
        int nrows = rows_of(0, i0);
        for (int64_t j = 0; nrows > 0 || (dyn && nrows == 0); ++j) {
          draw_issue();
          const int nnr = rows_of(j + 1, ni0);
          if (nrows > 0) {
            const int nn = nnr > 0 ? nnr : 0;
            piece2(std::integral_constant<int, 0>{}, j, i0, nrows, ni0, nn);
            draw_commit(j);
            pad(j, 0, nrows);
            piece2(std::integral_constant<int, 1>{}, j, i0, nrows, ni0, nn);
            pad(j, 1, nrows);
            piece2(std::integral_constant<int, 2>{}, j, i0, nrows, ni0, nn);
            pad(j, 2, nrows);
          } else {  // a unit without rows for this wave (its last < 4 rows)
            pre = false;
            draw_commit(j);
            for (int m = 0; m < 3; ++m) pad(j, m, 0);
          }
          i0 = ni0;
          nrows = nnr;
        }
      } else {
        for (int64_t j = 0;; ++j) {
          int64_t row0, rend;
          if (!batch(j, row0, rend)) break;
          const int64_t i0 = row0 + uw;
          const int nrows = i0 < rend ? static_cast<int>(min<int64_t>(kGR / 4, (rend - i0 + 3) / 4)) : 0;
          if (nrows == 0) continue;
          piece(std::integral_constant<int, 0>{}, j, i0, nrows);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // x / aux stores before the audio increments
          piece(std::integral_constant<int, 1>{}, j, i0, nrows);
          piece(std::integral_constant<int, 2>{}, j, i0, nrows);
        }
      }
    }
    if (a.cmax_part) {  // this wave's column bounds (mmb_gram_i8)
      const int64_t wid = static_cast<int64_t>(blockIdx.x) * 4 + wave;
      if (lane < (D >> 2)) st4(a.cmax_part + wid * D + 4 * lane, cmx[0]);
      if constexpr (PIPE == 0) {
        if (lane + kWave < (D >> 2)) st4(a.cmax_part + wid * D + 4 * (lane + kWave), cmx[1]);
      } else {
        if (4 * kWave + lane < D) a.cmax_part[wid * D + 4 * kWave + lane] = cmt;
      }
    }
    FUSED_PROBE(1 + wave);
    return;
  }

  // -------------------------------------------------------------- projector
  const int pw = wave - 4;
  const int q = lane & 15, g = lane >> 4;  // A row / B column in a tile; k group
  constexpr int CH = 2 * kFLdw * 32, PL = kFLdw * 32;  // B image chunk / plane (halves)
  const int nch = (f.kq[0] + f.kq[1] + f.kq[2]) / 32;
  const int cb[3] = {0, f.kq[0] / 32, (f.kq[0] + f.kq[1]) / 32};
  const auto brsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(f.img), 0, nch * CH * 2,
                                                       0x00020000);
  int boff[kFTiles];
  float cinv[kFTiles], cadd[kFTiles];
#pragma unroll
  for (int t = 0; t < kFTiles; ++t) {
    const int col = 16 * (kFTiles * pw + t) + q;
    boff[t] = col * 32 + ((g ^ x3_swz(col)) << 3);
    cinv[t] = f.col_inv[col];
    cadd[t] = f.c0[col];
  }
  // column D (the total weight) lives in projector tD_w, tile tD_t, lane q == tD_q
  const int tD = D >> 4, tD_w = tD / kFTiles, tD_t = tD % kFTiles, tD_q = D & 15;
  // this projector's tiles holding columns <= D (the rest of the 320 are
  // zero); 256 <= D < 320 leaves at most one dead tile, on projector 3
  const int ntiles = max(kFTiles - 1, min(kFTiles, tD + 1 - kFTiles * pw));
  int ep = 0;  // projector exchange points passed
  for (int64_t j = 0;; ++j) {
    int64_t row0, rend;
    if (!batch(j, row0, rend)) break;
    const int nvalid = static_cast<int>(rend - row0);
    f32x4 acc[kGRT][kFTiles];
#pragma unroll
    for (int rt = 0; rt < kGRT; ++rt)
#pragma unroll
      for (int t = 0; t < kFTiles; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float irs[kGRT][4];
#pragma unroll 1
    for (int m = 0; m < 3; ++m) {
      const int p = 3 * static_cast<int>(j) + m;
      fused_wait(&fill[p & 3], kGR * (p >> 2) + (dyn ? kGR : nvalid), abort_flag, a.flag);
      if constexpr ((DIAG & 1) != 0) {
        fused_signal(consumed);
        continue;
      }
      // this piece's power-of-2 scales of the lane's output rows 16 rt + 4 g + jj;
      // the running sums move to this piece's scale (exact: ratios of powers of 2)
#pragma unroll
      for (int rt = 0; rt < kGRT; ++rt)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const float v = s_irs[(p * kGR + 16 * rt + 4 * g + jj) % SL];
          if (m > 0) {
            const float ratio = irs[rt][jj] / v;
#pragma unroll
            for (int t = 0; t < kFTiles; ++t) acc[rt][t][jj] *= ratio;
          }
          irs[rt][jj] = v;
        }
      const _Float16* arow[kGRT];
#pragma unroll
      for (int rt = 0; rt < kGRT; ++rt) arow[rt] = ring + ((p * kGR + 16 * rt + q) % SL) * kGSlot;
      const int npc = f.kq[m] / 32, c0g = cb[m];
      // the K loop for NT live column tiles (tiles past column D hold zero
      // padding: projector 3 at D = 300 skips their loads and MFMAs)
      auto kloop = [&](auto nt_c) {
        constexpr int NL = decltype(nt_c)::value;
        half8 bh[2][NL], bl[2][NL];
        auto ld_b = [&](int c, half8 (&h)[NL], half8 (&l)[NL]) {
          // DIAG 16: every chunk reads the piece's chunk 0 (a 20 KB L2 footprint)
          const int so = (DIAG & 16) ? c0g * CH * 2 : (c0g + (c < npc ? c : npc - 1)) * CH * 2;
#pragma unroll
          for (int t = 0; t < NL; ++t) {
            if constexpr ((DIAG & 32) != 0) {  // no B loads at all
              h[t] = l[t] = half8{1, 1, 1, 1, 1, 1, 1, 1};
            } else {
              h[t] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(brsrc, boff[t] * 2, so, 0));
              l[t] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(brsrc, (boff[t] + PL) * 2, so, 0));
            }
          }
        };
        auto chunk = [&](int c, const half8 (&h)[NL], const half8 (&l)[NL]) {
          const int o = (((4 * c + g) ^ q) << 3);
#pragma unroll
          for (int rt = 0; rt < kGRT; ++rt) {
            const half8 ah = *reinterpret_cast<const half8*>(arow[rt] + o);
            const half8 al = *reinterpret_cast<const half8*>(arow[rt] + kGPlane + o);
            if constexpr ((DIAG & 2) != 0) {
              asm volatile("" ::"v"(ah), "v"(al));
#pragma unroll
              for (int t = 0; t < NL; ++t) asm volatile("" ::"v"(h[t]), "v"(l[t]));
            } else {
#pragma unroll
              for (int t = 0; t < NL; ++t) {
                acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, h[t], acc[rt][t], 0, 0, 0);
                acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, l[t], acc[rt][t], 0, 0, 0);
                acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, h[t], acc[rt][t], 0, 0, 0);
              }
            }
          }
        };
        ld_b(0, bh[0], bl[0]);
        ld_b(1, bh[1], bl[1]);
#pragma unroll 1
        for (int c = 0; c < npc; c += 2) {
          chunk(c, bh[0], bl[0]);
          ld_b(c + 2, bh[0], bl[0]);
          if (c + 1 < npc) {
            chunk(c + 1, bh[1], bl[1]);
            ld_b(c + 3, bh[1], bl[1]);
          }
        }
      };
      if (ntiles == kFTiles) {
        kloop(std::integral_constant<int, kFTiles>{});
      } else {
        kloop(std::integral_constant<int, kFTiles - 1>{});
      }
      // this projector's LDS reads of the piece's slots are done (lgkmcnt
      // only: its weight-image loads in flight and the previous epilogue's
      // MMB2 stores do not guard the slots; 22.48 -> 22.45 ms, r02z)
      fused_signal_lds(consumed);
    }
    if constexpr ((DIAG & 5) != 0) {
#pragma unroll
      for (int rt = 0; rt < kGRT; ++rt)
#pragma unroll
        for (int t = 0; t < kFTiles; ++t) asm volatile("" ::"v"(acc[rt][t]));
      continue;
    }

    // epilogue: lane value (rt, t, jj) = row 16 rt + 4 g + jj, column 16 (5 pw + t) + q
    const float* cntb = s_cnt + (j & 1) * kGR;
    const float* twb = s_tw + (j & 1) * kGR;
    float* tot = s_tot + (j & 1) * kGR;
    float* ssq = s_ssq + (j & 1) * 4 * kGR;
#pragma unroll
    for (int rt = 0; rt < kGRT; ++rt) {
      float xv[kFTiles][4];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int64_t rowc = min(row0 + 16 * rt + 4 * g + jj, N - 1);
#pragma unroll
        for (int t = 0; t < kFTiles; ++t) {
          const int col = 16 * (kFTiles * pw + t) + q;
          if constexpr ((DIAG & 128) != 0) {  // timing only: no x re-read
            xv[t][jj] = static_cast<float>(col);
          } else {
            xv[t][jj] = a.num_out[rowc * D + min(col, D - 1)];
          }
        }
      }
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int r = 16 * rt + 4 * g + jj;
        const float cn = cntb[r], tw = twb[r];
#pragma unroll
        for (int t = 0; t < kFTiles; ++t) {
          const int col = 16 * (kFTiles * pw + t) + q;
          const float add = col < D ? text_sum(xv[t][jj], cn) : (col == D ? tw : 0.f);
          acc[rt][t][jj] = acc[rt][t][jj] * (cinv[t] * irs[rt][jj]) + add + cadd[t];
        }
        if (pw == tD_w && q == tD_q) {
#pragma unroll
          for (int t = 0; t < kFTiles; ++t)
            if (t == tD_t) tot[r] = acc[rt][t][jj];
        }
      }
    }
    fused_signal_lds(pbar);  // the row totals exchanged through LDS only
    fused_wait(pbar, 4 * ++ep, abort_flag, a.flag);
#pragma unroll
    for (int rt = 0; rt < kGRT; ++rt) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int r = 16 * rt + 4 * g + jj;
        const float rtot = 1.f / tot[r];
        float ss = 0.f;
#pragma unroll
        for (int t = 0; t < kFTiles; ++t) {
          const int col = 16 * (kFTiles * pw + t) + q;
          acc[rt][t][jj] *= rtot;
          if (col < D) ss = fmaf(acc[rt][t][jj], acc[rt][t][jj], ss);
        }
        ss = row16_sum(ss);
        if (q == 0) ssq[pw * kGR + r] = ss;
      }
    }
    fused_signal_lds(pbar);
    fused_wait(pbar, 4 * ++ep, abort_flag, a.flag);
#pragma unroll
    for (int rt = 0; rt < kGRT; ++rt) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int r = 16 * rt + 4 * g + jj;
        const float inv = 1.f / sqrtf((ssq[r] + ssq[kGR + r]) + (ssq[2 * kGR + r] + ssq[3 * kGR + r]));
        if (r < nvalid) {
          float* orow = f.out + (row0 + r) * D;
#pragma unroll
          for (int t = 0; t < kFTiles; ++t) {
            const int col = 16 * (kFTiles * pw + t) + q;
            if constexpr ((DIAG & 256) != 0) {  // timing only: no MMB2 stores
              asm volatile("" ::"v"(acc[rt][t][jj] * inv));
            } else {
              if (col < D) orow[col] = acc[rt][t][jj] * inv;
            }
          }
        }
      }
    }
  }
  FUSED_PROBE(1 + wave);
}


template <int DIAG, int UNR = 8, int PIPE = 0, int SL = kGSlots, int TM = 7, class FE = float, class TE = float>
static void launch_fused_v(const FusedArgs& f, int grid, hipStream_t stream) {
  constexpr size_t lds = fused_lds_bytes(SL);
  allow_dynamic_lds<&utt_fused_kernel<UNR, true, DIAG, PIPE, SL, TM, FE, TE>>(lds);
  utt_fused_kernel<UNR, true, DIAG, PIPE, SL, TM, FE, TE><<<grid, kFThreads, lds, stream>>>(f);
}
// the pipelined streamer specialised for the pieces that carry a row tail
// (a piece-level, wave-uniform choice made here, once per launch)
// (the mask TM: bit 0 text, bit 1 audio, bit 2 visual; asked as "no tail",
// visual first, so that the kernels are instantiated in the order TM = 0..7)
template <int UNR, int PIPE, class FE = float, class TE = float>
static void launch_fused_tm(const FusedArgs& f, int grid, hipStream_t stream) {
  dispatch3(f.s.Vd <= 4 * kWave, f.s.A <= 4 * kWave, f.s.D <= 4 * kWave, [&](auto v, auto a, auto t) {
    constexpr int TM = (t.value ? 0 : 1) | (a.value ? 0 : 2) | (v.value ? 0 : 4);
    launch_fused_v<0, UNR, PIPE, kGSlots, TM, FE, TE>(f, grid, stream);
  });
}
// the pipelined streamer's frames per load group (two groups in flight per
// wave: 20 frames, 100 VGPRs of buffers).  Same-process sweep at 1M rows, T =
// 40 (four whole groups per row), fused kernel ms: 8 frames 21.3, 10 frames
// 20.9, 12 frames 22.0 (its last group of a row is one third live); the
// parent's float4 tails with 8 frames 22.1.  The other
// candidates live in the tools build (MMB_FUSED_UNR).  The 16-bit
// instantiations keep the group size and depth (60 VGPRs of buffers), for
// the frames and for the rows of a 16-bit table alike.
constexpr int kFUnr = 10;
// streamer: 1 = pipelined (two groups in flight: kernel 23.35 -> 22.49 ms,
// step 25.14 -> 24.41 ms in a same-process A/B, r02k); 2 (default) = also
// prefetching across piece and batch boundaries (22.32 -> 22.14 ms, r02y);
// 0 = one group at a time, 8 frames each, float4 row tails (the fallback for
// rows of < 3 frame groups or a word table >= 2 GB, and the bit-identical
// reference of the tests)
template <class TE = float>
static bool fused_pipe_ok(const FusedArgs& f, int un) {
  // the pipelined streamer stages a text row's tokens two groups before its
  // first group is issued (ids at the row before's first group, wtab[id] at
  // its second): >= 3 groups of un frames per row -- T >= 21 at the product's
  // 10-frame groups, shorter rows take the fallback; it addresses the word
  // table through one buffer descriptor (< 2^31 bytes: a 16-bit table keeps
  // it up to twice the rows)
  return (f.s.L + un - 1) / un >= 3 &&
         (f.s.ids == nullptr || f.s.V * f.s.D * static_cast<int>(sizeof(TE)) < (int64_t{1} << 31));
}

static int fused_grid(int64_t nb, hipStream_t stream) {
  return static_cast<int>(std::min<int64_t>(nb, std::min(stream_cu_count(stream), kCmaxRows / 4)));
}

// the product's two kernels for frames of type FE and a word table of type
// TE: the pipelined streamer per tail mask, or the group-at-a-time fallback
template <class FE, class TE = float>
static int launch_fused_frames(const FusedArgs& f, int grid, hipStream_t stream) {
  if (fused_pipe_ok<TE>(f, kFUnr)) {
    launch_fused_tm<kFUnr, 2, FE, TE>(f, grid, stream);
  } else {
    launch_fused_v<0, 8, 0, kGSlots, 7, FE, TE>(f, grid, stream);
  }
  MMB_LAUNCH_CHECK();
  return MMB_OK;
}

// the 16-bit instantiations' launches, one source each: 16-bit frames on an
// f32 table (fused_f16_kernels.hip, fused_bf16_kernels.hip), called by
// mmb_mm2_stream_project_ft, and a 16-bit table under each frame type
// (fused_t<table>_<frames>_kernels.hip), called by mmb_mm2_stream_project_tt
#pragma GCC visibility push(hidden)
int launch_fused_f16(const FusedArgs& f, int grid, hipStream_t stream);
int launch_fused_bf16(const FusedArgs& f, int grid, hipStream_t stream);
int launch_fused_tf16_f32(const FusedArgs& f, int grid, hipStream_t stream);
int launch_fused_tf16_f16(const FusedArgs& f, int grid, hipStream_t stream);
int launch_fused_tf16_bf16(const FusedArgs& f, int grid, hipStream_t stream);
int launch_fused_tbf16_f32(const FusedArgs& f, int grid, hipStream_t stream);
int launch_fused_tbf16_f16(const FusedArgs& f, int grid, hipStream_t stream);
int launch_fused_tbf16_bf16(const FusedArgs& f, int grid, hipStream_t stream);
#pragma GCC visibility pop

}  // namespace mmb
