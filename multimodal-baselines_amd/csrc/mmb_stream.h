// What the stream sources share (narrow_fused_kernels.hip, through
// mmb_stream_kernels.h the three SIF sources, through mmb_fused.h the fused
// sources, through mmb_split_kernels.h and mmb_text_cache.h the two split_tab
// sources and, for the element types, mm2_kernels.hip; included by them
// only): the
// kernels' argument block and limits, the frame and table element types, the device
// helpers more than one kernel family uses, and the declarations of the entry
// points' host-side front end (defined once, in sif_kernels.hip).  No
// __global__ function lives here: every kernel is in exactly one code object.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "mmb_common.h"

namespace mmb {

constexpr int kNT = 320;              // threads per utterance workgroup
constexpr int kTokChunk = 512;        // tokens staged per LDS chunk
constexpr int kRedFloats = kNT * 4;   // one accumulator image: R*F <= NT*VEC

struct StreamArgs {
  const int32_t* ids;
  const float* table;
  int64_t V;
  const float* wtab;        // f32 weight table (gather mode without w_dense)
  const float* w_dense;     // [N,L] given weights
  const float* text_dense;  // [N,L,D] dense text frames (MMB2 drop-in mode)
  const float* emb_dense;   // [N,L,D] rows for the weighted sum (may alias text_dense)
  const void* audio;        // [N,L,A]   elements of the kernel's frame type FE,
  const void* visual;       // [N,L,Vd]  read through frames<FE>()
  int64_t N;
  int L, D, A, Vd, Kp;
  float* x_out;
  float* num_out;
  float* cnt_out;
  float* s_out;     // [N][Kp] fp32, or with s_half [N][2][Kp] fp16 (hi | lo, row-scaled)
  float* aux_out;
  int32_t* flag;
  int s_half;
  float* cmax_part;  // per-wave (wave kernel) / per-workgroup running max |x| rows [P][D], or null
};

// max of two column bounds |x| >= 0 on their bits: for non-negative floats the
// unsigned order is the float order, and a NaN (|NaN| = 0x7fc00000..) ranks
// above inf -- so a non-finite x reaches the bound (and mmb_gram_i8 then
// writes NaN into G, as the f64 Gram would), where fmaxf would drop a NaN
__device__ __forceinline__ float bmax(float a, float b) {
  return __uint_as_float(max(__float_as_uint(a), __float_as_uint(b)));
}
__device__ __forceinline__ float4 bmax4(float4 m, float4 x) {
  return make_float4(bmax(m.x, fabsf(x.x)), bmax(m.y, fabsf(x.y)), bmax(m.z, fabsf(x.z)),
                     bmax(m.w, fabsf(x.w)));
}

template <int VEC>
__device__ __forceinline__ void ldv(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = *p;
  }
}
// Frame element types of the MMB2 stream kernels (mmb_mm2_stream_ft): f32, or
// 16-bit storage widened to f32 in registers right after the load.  Both
// widenings are exact (fp16 subnormals included), so a kernel instantiated
// for a 16-bit type sums what its f32 instantiation sums on the upcast
// frames, bit for bit.
using f16_t = _Float16;  // IEEE binary16
struct bf16_t {          // bfloat16: the high half of an f32
  uint16_t bits;
};
using u2 = unsigned __attribute__((ext_vector_type(2)));  // four 16-bit frame values
// StreamArgs::audio / ::visual as the frames of type FE they hold
template <class FE>
__device__ __forceinline__ const FE* frames(const void* p) {
  return static_cast<const FE*>(p);
}
// bytes of a frame value of storage type frame_type (MMB_FRAMES_*, include/mmb.h); 0: not a frame type
inline int frame_bytes(int frame_type) {
  return frame_type == MMB_FRAMES_F32 ? 4 : (frame_type == MMB_FRAMES_F16 || frame_type == MMB_FRAMES_BF16) ? 2 : 0;
}
template <class FE>
__device__ __forceinline__ float frame_f32(uint32_t bits16) {
  if constexpr (std::is_same_v<FE, bf16_t>) {
    return __uint_as_float(bits16 << 16);
  } else {
    return static_cast<float>(__builtin_bit_cast(f16_t, static_cast<uint16_t>(bits16)));
  }
}
// one 8-byte unit of four 16-bit values -> f32 (bf16: a shift / a mask per value)
template <class FE>
__device__ __forceinline__ float4 frame_f32x4(u2 q) {
  if constexpr (std::is_same_v<FE, bf16_t>) {
    return make_float4(__uint_as_float(q.x << 16), __uint_as_float(q.x & 0xffff0000u),
                       __uint_as_float(q.y << 16), __uint_as_float(q.y & 0xffff0000u));
  } else {
    return make_float4(frame_f32<FE>(q.x & 0xffffu), frame_f32<FE>(q.x >> 16),
                       frame_f32<FE>(q.y & 0xffffu), frame_f32<FE>(q.y >> 16));
  }
}

// Word-table element types of mmb_sif_wavg_tt / mmb_mm2_stream_tt: f32, or
// the same two 16-bit storage types, widened in the same exact way right
// after the load -- so a kernel instantiated for a 16-bit table type TE sums
// what its f32 instantiation sums on the upcast table, bit for bit.
// StreamArgs::table stays a float pointer; a TE kernel reads it as TE.
// bytes of a table value of storage type table_type (MMB_TABLE_*, include/mmb.h); 0: not a table type
inline int table_bytes(int table_type) {
  return table_type == MMB_TABLE_F32 ? 4 : (table_type == MMB_TABLE_F16 || table_type == MMB_TABLE_BF16) ? 2 : 0;
}
// element f of the table as f32 (the workgroup kernels' row-0 shortcut)
template <class TE>
__device__ __forceinline__ float table_f32(const float* table, int f) {
  if constexpr (std::is_same_v<TE, float>) {
    return table[f];
  } else {
    return frame_f32<TE>(reinterpret_cast<const uint16_t*>(table)[f]);
  }
}
// ldv on a 16-bit table row: plain cached loads (the rows are the reused
// data), a unit of 4 values one 8-byte load, a scalar one a 2-byte load
template <int VEC, class TE>
__device__ __forceinline__ void ldv16(const TE* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 q = frame_f32x4<TE>(*reinterpret_cast<const u2*>(p));
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = frame_f32<TE>(*reinterpret_cast<const uint16_t*>(p));
  }
}

// the same, non-temporal: for the read-once frame streams (a 16-bit unit of
// 4 values is one 8-byte load, a scalar one a 2-byte load)
template <int VEC, class FE>
__device__ __forceinline__ void ldv_nt(const FE* p, float (&v)[VEC]) {
  if constexpr (!std::is_same_v<FE, float>) {
    if constexpr (VEC == 4) {
      const float4 q = frame_f32x4<FE>(__builtin_nontemporal_load(reinterpret_cast<const u2*>(p)));
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      v[0] = frame_f32<FE>(__builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(p)));
    }
  } else if constexpr (VEC == 4) {
    using f4 = float __attribute__((ext_vector_type(4)));
    const f4 q = __builtin_nontemporal_load(reinterpret_cast<const f4*>(p));
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = __builtin_nontemporal_load(p);
  }
}

// Power-of-2 scale that brings a row's max |value| into [2^14, 2^15): the
// projection GEMM splits the sums into fp16 hi/lo pairs (mm2_kernels.hip) and
// needs them in fp16's full-precision range.  Exact (a power of two).
__device__ __forceinline__ float row_scale(float m) {
  if (!(m > 0.f) || !isfinite(m)) return 1.f;
  int ex;
  frexpf(m, &ex);  // m = f * 2^ex, f in [0.5, 1)
  return ldexpf(1.f, 15 - ex);
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}

// Resolve token t of utterance i: element offset of its text row (or -1) and
// its SIF weight.  Semantics of sif_functions.py:8-15 (weight gather, id<0 ->
// 0) and numpy/torch fancy indexing for the row (negative ids wrap).
__device__ __forceinline__ void stage_token(const StreamArgs& a, int64_t i, int t, int64_t& off,
                                            float& w) {
  const int64_t ft = i * a.L + t;
  if (a.ids) {
    int64_t id = a.ids[ft];
    if (a.w_dense) {
      w = a.w_dense[ft];
    } else {
      w = (id >= 0 && id < a.V) ? a.wtab[id] : 0.f;
    }
    if (id < 0) id += a.V;
    if (id < 0 || id >= a.V) {
      if (a.flag) atomicOr(a.flag, MMB_FLAG_ID_RANGE);
      off = -1;
      w = 0.f;
    } else {
      off = id * a.D;
    }
  } else {
    w = a.w_dense ? a.w_dense[ft] : 0.f;
    off = ft * a.D;
  }
}

// Token staging of the workgroup kernel.  In gather mode the tokens whose
// row is table row 0 (id 0: the reference's pad / OOV index, ~72 % of a POM
// transcript) are not staged: they are counted (c0) and their weights summed
// (w0), and row 0 enters the sums once at the end as w0 * E0, c0 * E0,
// c0 * E0^2 -- one load instead of c0.  The other tokens are compacted in
// token order (wave ballots + a fixed-order prefix over the waves), so the
// text loop runs over rows that carry new bytes only.  Out-of-range ids
// (flagged) are dropped: they contribute nothing (sif_functions.py:8-15).

// The text rows of a staged token chunk (workgroup kernels): row slot rT
// of the chunk's nkeep kept tokens, CT column units of VT floats at cT.
// Branch-free per row (a negative offset loads row 0 and contributes
// nothing) and SPLIT (the weighted sum over a different dense tensor) a
// template argument, so the TU unrolled rows' loads issue together: a
// runtime `split_emb` test per row put a branch and a wait for that row's
// load after every load (r06: the gfx950 ISA of the split-part kernel).
// TE: the rows' element type (a 16-bit word table: widened after the load).
template <bool MM2, bool SPLIT, int VT, int TU, class TE = float>
__device__ __forceinline__ void text_rows(const TE* tsrc, const TE* esrc, const int64_t* s_off,
                                          const float* s_w, int nkeep, int rT, int RT, int cT,
                                          float (&num)[VT], float (&sx)[VT], float (&sxx)[VT]) {
#pragma unroll TU
  for (int t = rT; t < nkeep; t += RT) {
    const float w = s_w[t];
    const int64_t off = s_off[t];
    const bool ok = off >= 0;
    const int64_t o = ok ? off : 0;
    float v[VT];
    if constexpr (std::is_same_v<TE, float>) {
      ldv<VT>(tsrc + o + cT * VT, v);
    } else {
      ldv16<VT, TE>(tsrc + o + cT * VT, v);
    }
#pragma unroll
    for (int e = 0; e < VT; ++e) v[e] = ok ? v[e] : 0.f;
    if constexpr (SPLIT) {
      static_assert(std::is_same_v<TE, float>, "a second dense tensor is f32");
      float u[VT];
      ldv<VT>(esrc + o + cT * VT, u);
#pragma unroll
      for (int e = 0; e < VT; ++e) num[e] = fmaf(w, ok ? u[e] : 0.f, num[e]);
    } else {
#pragma unroll
      for (int e = 0; e < VT; ++e) num[e] = fmaf(w, v[e], num[e]);
    }
    if constexpr (MM2) {
#pragma unroll
      for (int e = 0; e < VT; ++e) {
        sx[e] += v[e];
        sxx[e] = fmaf(v[e], v[e], sxx[e]);
      }
    }
  }
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
using nf4 = float __attribute__((ext_vector_type(4)));
// Frame streams are read exactly once: NT=true marks them non-temporal so they
// do not evict the (Zipf-hot) word-table rows from L2 / Infinity Cache.
template <bool NT>
__device__ __forceinline__ float4 ldnt4(const float* p) {
  if constexpr (NT) {
    const nf4 v = __builtin_nontemporal_load(reinterpret_cast<const nf4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
  } else {
    return *reinterpret_cast<const float4*>(p);
  }
}
__device__ __forceinline__ void fma4(float4& acc, float w, float4 v) {
  acc.x = fmaf(w, v.x, acc.x); acc.y = fmaf(w, v.y, acc.y);
  acc.z = fmaf(w, v.z, acc.z); acc.w = fmaf(w, v.w, acc.w);
}
__device__ __forceinline__ void add4(float4& acc, float4 v) {
  acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
}
__device__ __forceinline__ void sq4(float4& acc, float4 v) {
  acc.x = fmaf(v.x, v.x, acc.x); acc.y = fmaf(v.y, v.y, acc.y);
  acc.z = fmaf(v.z, v.z, acc.z); acc.w = fmaf(v.w, v.w, acc.w);
}
__device__ __forceinline__ float amax4(float4 v) {
  return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
}
__device__ __forceinline__ float4 div4(float4 v, float c) {
  return make_float4(v.x / c, v.y / c, v.z / c, v.w / c);
}
using h4 = _Float16 __attribute__((ext_vector_type(4)));
// Output rows (x, s planes) are written once and read back by a later kernel,
// far beyond what L2 / Infinity Cache hold: NTS=true writes them non-temporal.
template <bool NTS>
__device__ __forceinline__ void stnt4(float* p, float4 v) {
  if constexpr (NTS) {
    __builtin_nontemporal_store(nf4{v.x, v.y, v.z, v.w}, reinterpret_cast<nf4*>(p));
  } else {
    *reinterpret_cast<float4*>(p) = v;
  }
}
// x * rs (rs a power of two: exact) as fp16 hi + fp16 lo = the residual
template <bool NTS = false>
__device__ __forceinline__ void split_store4(_Float16* hi, _Float16* lo, float4 v, float rs) {
  const float x[4] = {v.x * rs, v.y * rs, v.z * rs, v.w * rs};
  h4 h, l;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    h[e] = static_cast<_Float16>(x[e]);
    l[e] = static_cast<_Float16>(x[e] - static_cast<float>(h[e]));
  }
  if constexpr (NTS) {
    __builtin_nontemporal_store(h, reinterpret_cast<h4*>(hi));
    __builtin_nontemporal_store(l, reinterpret_cast<h4*>(lo));
  } else {
    *reinterpret_cast<h4*>(hi) = h;
    *reinterpret_cast<h4*>(lo) = l;
  }
}

// Three run-time bits as compile-time constants: f(c0, c1, c2) with a
// std::true_type or std::false_type for each bit -- the one place where the
// launchers' eight template cases (a bit per modality) are spelled out.
template <class F>
static auto dispatch3(bool b0, bool b1, bool b2, F f) {
  auto pick = [](bool b, auto g) {
    if (b) return g(std::true_type{});
    return g(std::false_type{});
  };
  return pick(b0, [&](auto c0) {
    return pick(b1, [&](auto c1) { return pick(b2, [&](auto c2) { return f(c0, c1, c2); }); });
  });
}

// rows of the column-bound partials (one per wave / workgroup of a launch)
constexpr int kCmaxRows = 8192;

// ------------------------------------------------ the entry points' front end
// What mmb_sif_wavg and the MMB2 stream entry points of the three sources do
// alike (sif_kernels.hip defines and describes them).  Internal to the
// library: not exported.
#pragma GCC visibility push(hidden)
bool set_text_source(StreamArgs* s, const int32_t* ids, const float* table, int64_t v,
                     const float* wtab32, const float* text_dense, const float* emb_dense,
                     const float* w_dense);
int stream_args(StreamArgs* s, const int32_t* ids, const float* table, int64_t v, const float* wtab32,
                const float* text_dense, const float* emb_dense, const float* w_dense, const void* audio,
                const void* visual, int64_t n, int t, int d, int a_, int vd, float* num_out, void* s_out,
                int s_half, float* aux_out, int32_t* flag, const uint32_t* colmax, void* colmax_ws);
int empty_call(uint32_t* colmax, int d, hipStream_t stream);
int reduce_colmax(int rc, const StreamArgs& s, int parts, uint32_t* colmax, hipStream_t stream);
// vector eligibility of the three modalities: rows of whole 4-value column
// units from a base aligned to one unit -- 4 * tbytes (table_bytes; dense
// text: 16) of text, 4 * fbytes (frame_bytes) of audio / visual
struct StreamVec {
  bool t, a, v;
};
StreamVec stream_vec(const StreamArgs& s, int fbytes = 4, int tbytes = 4);
bool units_fit(const StreamArgs& s, const StreamVec& vec);
#pragma GCC visibility pop

}  // namespace mmb
