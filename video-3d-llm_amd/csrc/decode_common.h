// What the decode linears share around their K loops (decode.hip: 16-bit and e4m3 weights; gemm_fp4.hip: MXFP4): the row map, the
// finished output, the two tails (VALU and matrix-core), the activation-row setup, and on the host the argument check and the
// run-time -> compile-time dispatch.  The epilogue codes are include/v3d.h's V3D_DEC_*.
#pragma once
#include "v3d_common.h"
#include <type_traits>

namespace v3d {

constexpr int DEC_MAX_ROWS = 32;     // scenes / questions decoding together (r04: 32; the attention side: DEC_MAXROWS in attention.hip)

__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + __expf(-x)); }

__device__ __forceinline__ uint4 ldg_nt(const uint4* p) {
  uint4 r;
  r.x = __builtin_nontemporal_load(&p->x);
  r.y = __builtin_nontemporal_load(&p->y);
  r.z = __builtin_nontemporal_load(&p->z);
  r.w = __builtin_nontemporal_load(&p->w);
  return r;
}

using dec_f32x4 = __attribute__((ext_vector_type(4))) float;
using dec_bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using dec_f16x8 = __attribute__((ext_vector_type(8))) _Float16;
__device__ __forceinline__ dec_f32x4 dec_mfma(bf16_t, const uint4& a, const uint4& b, dec_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(dec_bf16x8, a), __builtin_bit_cast(dec_bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ dec_f32x4 dec_mfma(f16_t, const uint4& a, const uint4& b, dec_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(dec_f16x8, a), __builtin_bit_cast(dec_f16x8, b), c, 0, 0, 0);
}

// ---- the row map ------------------------------------------------------------------------------------------------------------------
// Weight row of output o.  SwiGLU weights are tile-interleaved - 64 gate rows, then their 64 up rows - so this is o's GATE row and its
// up row is + 64; a 16-output group (o % 16 == 0) owns the 16 consecutive rows from here (and the 16 from + 64).
template <int EPI>
__device__ __forceinline__ int dec_row0(int o) { return EPI == V3D_DEC_SWIGLU ? (o >> 6) * 128 + (o & 63) : o; }

// The four weight rows of a VALU workgroup -> its first output: four outputs, or (SwiGLU) two outputs = two (gate, up) row pairs.
template <int EPI>
__device__ __forceinline__ int dec_valu_rows(int (&rows)[4]) {
  if (EPI == V3D_DEC_SWIGLU) {
    const int o0 = blockIdx.x * 2;
    rows[0] = dec_row0<EPI>(o0); rows[1] = rows[0] + 64;
    rows[2] = dec_row0<EPI>(o0 + 1); rows[3] = rows[2] + 64;
    return o0;
  }
  const int o0 = blockIdx.x * 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) rows[r] = o0 + r;
  return o0;
}

// ---- the finished output ----------------------------------------------------------------------------------------------------------
// SwiGLU: silu(gate = v0) * (up = v1), each factor rounded as the separate linears and the activation kernel would; otherwise v0 (+ bias),
// the linear's own output rounding, (+ residual).  A value EPI does not use is not read.
template <typename T, int EPI>
__device__ __forceinline__ T dec_finish(float v0, float v1, float bias_value, float res_value) {
  if (EPI == V3D_DEC_SWIGLU) return from_f32<T>(round_to<T>(silu_f(round_to<T>(v0))) * round_to<T>(v1));
  if (EPI == V3D_DEC_BIAS) v0 += bias_value;
  v0 = round_to<T>(v0);                                     // the linear's own output rounding
  if (EPI == V3D_DEC_RES) v0 += res_value;
  return from_f32<T>(v0);
}

// The storing form: element (m, n) of the output; bias[n] / res[m][n] are loaded only when EPI needs them.
template <typename T, int EPI>
struct DecStore {
  const T* __restrict__ bias;
  const T* __restrict__ res;
  int64_t ldr;
  T* __restrict__ out;
  int64_t ldo;
  __device__ __forceinline__ void operator()(float v0, float v1, int m, int n) const {
    const float bv = EPI == V3D_DEC_BIAS ? to_f32(bias[n]) : 0.f;
    const float rv = EPI == V3D_DEC_RES ? to_f32(res[m * ldr + n]) : 0.f;
    out[m * ldo + n] = dec_finish<T, EPI>(v0, v1, bv, rv);
  }
};

// ---- the VALU tail ----------------------------------------------------------------------------------------------------------------
// s[m][r] = this thread's part of activation row m against weight row rows[r]: wave shuffle, the four waves meet in red and are added in
// order 0..3, then `fin` (a DecStore) finishes output (m, n).  SCALED (e4m3): the sum is multiplied by its weight row's scale sw first.
template <typename T, int EPI, int M, bool SCALED, typename Fin>
__device__ __forceinline__ void dec_valu_tail(float (&s)[M][4], float (&red)[M][4][4], const int (&rows)[4], int o0,
                                              const float* __restrict__ sw, Fin fin) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s[m][r] += __shfl_xor(s[m][r], off);
    }
  if (lane == 0) {
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[m][r][wave] = s[m][r];
  }
  __syncthreads();
  auto sum = [&](int m, int r) { return red[m][r][0] + red[m][r][1] + red[m][r][2] + red[m][r][3]; };
  if (EPI == V3D_DEC_SWIGLU) {
    if (tid < 2 * M) {
      const int m = tid >> 1, t2 = tid & 1;
      float g = sum(m, 2 * t2), u = sum(m, 2 * t2 + 1);
      if (SCALED) { g *= sw[rows[2 * t2]]; u *= sw[rows[2 * t2 + 1]]; }
      fin(g, u, m, o0 + t2);
    }
  } else if (tid < 4 * M) {
    const int m = tid >> 2, r = tid & 3, n = o0 + r;
    float v = sum(m, r);
    if (SCALED) v *= sw[n];
    fin(v, v, m, n);
  }
}

// ---- the matrix-core tail ---------------------------------------------------------------------------------------------------------
// Eight waves each hold a K slice's 16 x 16 accumulator tiles acc[q][b] (q: 16-row weight group, b: 16-row block of activation rows).
// They meet in LDS - `part(w, q, b)` -> the 256 floats of wave w's tile, wherever the kernel keeps them - and are added in order 0..7.
// tid / lane / wave are the KERNEL's own values (lane = tid & 63, wave = tid >> 6): formed again in here, the compiler folds them into
// the LDS address before it inlines the helper, and the K loops above it then allocate one or two registers differently.
struct DecElem { int b, t8, row, m; };
__device__ __forceinline__ DecElem dec_elem(int e) {        // e < 256 MB: float t8 of block b = weight row 4 (l >> 4) + i, scene l & 15 of the block
  const int b = e >> 8, t8 = e & 255, l = t8 >> 2, i = t8 & 3;
  return DecElem{b, t8, 4 * (l >> 4) + i, (l & 15) + 16 * b};
}

template <bool CLEAR, int RG, int MB, typename Part>                       // CLEAR: each accumulator is zeroed as soon as it is stored
__device__ __forceinline__ void dec_part_put(int lane, int wave, dec_f32x4 (&acc)[RG][MB], Part part) {
#pragma unroll
  for (int q = 0; q < RG; ++q)
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      *reinterpret_cast<float4*>(part(wave, q, b) + lane * 4) = make_float4(acc[q][b][0], acc[q][b][1], acc[q][b][2], acc[q][b][3]);
      if (CLEAR) acc[q][b] = dec_f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

template <int SW, typename Part>
__device__ __forceinline__ void dec_part_sum(Part part, int q0, const DecElem& el, float (&v)[SW]) {
#pragma unroll
  for (int q = 0; q < SW; ++q) {
    v[q] = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) v[q] += part(w, q0 + q, el.b)[el.t8];
  }
}

// The whole tail of a kernel whose workgroup owns the OG 16-output groups from output o0 (weight groups [og][gate | up]): put, barrier,
// sum, the optional per-row weight scale (SCALED, e4m3), and `fin(v0, v1, m, n)` for the rows that exist.
template <typename T, int EPI, int MB, int OG, bool SCALED, int RG, typename Part, typename Fin>
__device__ __forceinline__ void dec_mfma_tail(int tid, int lane, int wave, dec_f32x4 (&acc)[RG][MB], Part part, int o0, int M,
                                              const float* __restrict__ sw, Fin fin) {
  constexpr int SW = EPI == V3D_DEC_SWIGLU ? 2 : 1;
  static_assert(RG == SW * OG, "accumulator groups");
  dec_part_put<false>(lane, wave, acc, part);
  __syncthreads();
  for (int e = tid; e < 256 * MB * OG; e += 512) {
    const int og = OG == 1 ? 0 : e / (256 * MB);
    const DecElem el = dec_elem(e - og * 256 * MB);
    float v[SW];
    dec_part_sum<SW>(part, SW * og, el, v);
    if (SCALED) {
#pragma unroll
      for (int q = 0; q < SW; ++q) v[q] *= sw[dec_row0<EPI>(o0 + 16 * og) + 64 * q + el.row];
    }
    if (el.m < M) fin(v[0], v[SW - 1], el.m, o0 + 16 * og + el.row);
  }
}

// ---- activation rows of the matrix-core forms -------------------------------------------------------------------------------------
// Lane (r, g) feeds scene r + 16 b of block b.  Absent scenes (beyond M) point at row 0 so that no load needs a branch; col_ok says which
// they are (their fragments are zeroed, or their columns never stored).
template <typename T, int MB>
__device__ __forceinline__ void dec_x_rows(const T* __restrict__ x, int64_t ldx, int M, int r, int offset, bool (&col_ok)[MB], const T* (&xrow)[MB]) {
#pragma unroll
  for (int b = 0; b < MB; ++b) {
    col_ok[b] = r + 16 * b < M;
    xrow[b] = x + (int64_t)(col_ok[b] ? r + 16 * b : 0) * ldx + offset;
  }
}

// ---- host: argument check and dispatch --------------------------------------------------------------------------------------------
// What the three *_rows entry points require alike, in one order.  ptrs_ok / shape_ok / aligned are the weight format's own conditions;
// mfma_ok = the shape has a matrix-core form (then up to DEC_MAX_ROWS rows, else the VALU form's 4).  own_stride_text: the 16-bit entry
// reports a bad activation stride under its own message, the quantised ones under "alignment".
inline int dec_check_rows(const char* who, bool ptrs_ok, int dtype, bool shape_ok, bool mfma_ok, bool aligned, bool own_stride_text, int64_t ldx,
                          int M, int N, int K, int epilogue, const void* bias, const void* res) {
  V3D_REQUIRE(ptrs_ok, "%s: null pointer", who);
  V3D_REQUIRE(dtype == V3D_F16 || dtype == V3D_BF16, "%s: dtype must be f16 or bf16", who);
  V3D_REQUIRE(N > 0 && K > 0 && shape_ok, "%s: bad shape N=%d K=%d", who, N, K);
  const int max_rows = mfma_ok ? DEC_MAX_ROWS : 4;
  V3D_REQUIRE(M >= 1 && M <= max_rows, "%s: 1 to %d activation rows for this shape (got %d)", who, max_rows, M);
  V3D_REQUIRE(N % 4 == 0 && (epilogue != V3D_DEC_SWIGLU || N % 128 == 0), "%s: N=%d not supported", who, N);
  const bool stride_ok = M == 1 || (ldx % 8 == 0 && ldx >= K);
  V3D_REQUIRE(aligned && (own_stride_text || stride_ok), "%s: alignment", who);
  V3D_REQUIRE(stride_ok, "%s: activation row stride %lld", who, (long long)ldx);
  V3D_REQUIRE(epilogue != V3D_DEC_BIAS || bias, "%s: bias epilogue without bias", who);
  V3D_REQUIRE(epilogue != V3D_DEC_RES || res, "%s: residual epilogue without residual", who);
  return V3D_OK;
}

template <int V> using dec_int = std::integral_constant<int, V>;

// run-time value -> compile-time one: f(dec_int<V>{}) for the listed V that equals v, the LAST one for every other v
template <int V, int... Rest, typename F>
inline void dec_pick(int v, F&& f) {
  if constexpr (sizeof...(Rest) == 0) f(dec_int<V>{});
  else if (v == V) f(dec_int<V>{});
  else dec_pick<Rest...>(v, f);
}

// (dtype, epilogue) -> launch(T{}, dec_int<EPI>{}), then the launch check.  dtype has been checked (dec_check_rows).
template <typename F>
inline int dec_dispatch(int dtype, int epilogue, const char* who, F&& launch) {
  auto with = [&](auto t) {
    switch (epilogue) {
      case V3D_DEC_NONE: launch(t, dec_int<V3D_DEC_NONE>{}); break;
      case V3D_DEC_BIAS: launch(t, dec_int<V3D_DEC_BIAS>{}); break;
      case V3D_DEC_RES: launch(t, dec_int<V3D_DEC_RES>{}); break;
      case V3D_DEC_SWIGLU: launch(t, dec_int<V3D_DEC_SWIGLU>{}); break;
      default: set_error("%s: unknown epilogue %d", who, epilogue); return (int)V3D_E_INVALID;
    }
    return check_launch(who);
  };
  return dtype == V3D_BF16 ? with(bf16_t{}) : with(f16_t{});
}

}  // namespace v3d
