// What the visual-token kernels share, each stated once: the voxeliser, the sinusoid's value, the bilinear tap, and the body of
// one output token row (pool + PE add + newline rows) that visual_tokens.hip, pe_points.hip and pe_mlp.hip instantiate with their
// own PE source; train.hip's backward uses the same tap.
//
// The rounding contract lives here.  Every f32 operation is a single IEEE operation in the order written (__f*_rn cannot be
// contracted, whatever -ffp-contract the including file is built with); the one fused multiply-add the reference does use is
// written explicitly as fmaf.  A pooled value is rounded to T, then the PE add is rounded to T: two rounding points, no others.
#pragma once
#include "v3d_common.h"

namespace v3d {

// ----------------------------------------------------------------------------------------
// discrete_coords (llava/model/llava_arch.py:259-272), torch-on-CPU dtype rules
// (pinned exhaustively for fp16 by tests/golden/discrete_coords.npz):
//   clamp; t = T(x - lo); q = T(float(t) / float(voxel)); r = rint(q)
// ----------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ float voxelise(float x, float lo, float hi, float voxel) {
  // torch.maximum / minimum propagate NaN
  if (x == x) {
    x = x < lo ? lo : x;
    x = x > hi ? hi : x;
  }
  const float t = round_to<T>(__fsub_rn(x, lo));
  const float q = round_to<T>(__fdiv_rn(t, voxel));
  return rintf(q);
}

struct Range { float lo[3], hi[3], voxel; };

inline int fill_range(Range& rg, const float* lo, const float* hi, float voxel, const char* who) {
  V3D_REQUIRE(lo && hi, "%s: min/max range pointers are null", who);
  V3D_REQUIRE(voxel > 0.0f, "%s: voxel_size must be > 0", who);
  for (int i = 0; i < 3; ++i) { rg.lo[i] = lo[i]; rg.hi[i] = hi[i]; }
  rg.voxel = voxel;
  return V3D_OK;
}

// position_encoding.py:27-40: feature j of an axis is sin(p/dim_t[j]) for even j, cos for odd j
// (the odd-num_feats branch pads one column and drops it again: same rule).
// p/dim_t is an IEEE f32 division as in the reference; the trig is evaluated in double and
// rounded once to f32, i.e. the correctly rounded f32 value (torch's vectorised sin/cos is
// within 1 ulp of it).
__device__ __forceinline__ float pe_value(float p, float dim_t, int j) {
  const float arg = __fdiv_rn(p, dim_t);
  return (float)((j & 1) ? cos((double)arg) : sin((double)arg));
}

// a PE table row: the nf values of one id at a shift of up to vec - 1 elements, zero bits around them, whole 16-byte vectors
__host__ __device__ inline int table_row_elems(int nf, int vec) { return ((nf + vec - 1) / vec) * vec + vec; }

// ATen upsample_bilinear2d, align_corners=False: source index = fma(scale, o + .5, -.5), clamped at 0
struct Taps { int i0, i1; float l0, l1; };

__device__ __forceinline__ Taps bilinear_tap(int o, int n_in, int n_out) {
  const float scale = __fdiv_rn((float)n_in, (float)n_out);
  float src = fmaf(scale, (float)o + 0.5f, -0.5f);   // single rounding, as ATen's builds do
  src = src < 0.0f ? 0.0f : src;
  Taps t;
  t.i0 = (int)src;
  t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
  t.l1 = __fsub_rn(src, (float)t.i0);
  t.l0 = __fsub_rn(1.0f, t.l1);
  return t;
}

// ----------------------------------------------------------------------------------------
// The body of the three fused kernels: one output token row.  One workgroup = one OUTPUT token row of C channels; lane = one
// 16-byte vector of channels.  Everything that depends only on the token (taps, blend weights, what the PE source sets up per
// token) is workgroup-uniform and lives in SGPRs.
//
//   POOL   : x = h0*(w0*x00 + w1*x01) + h1*(w0*x10 + w1*x11) in f32, rounded to T
//   PE     : x = T(x + pe[channel])                      (llava_arch.py:515, add in the model dtype)
//   NEWLINE: row (v, oh, n) of the output is `newline`
//
// Per output token the kernel reads 4 input rows (2 when a tap pair collapses at an edge) and writes one row: algorithmic HBM
// traffic is feat + out, every input row being touched exactly once except tap row/col 13 (twice).
//
// `Src` supplies the PE operand.  The kernels differ in WHEN they issue its loads, which is deliberate (see each source), hence
// one hook per place:
//   Src::ON            false: there is no PE add at all (x + 0 would turn a -0 into +0)
//   src.token(cell)    once per token, cell = (v * n + oh) * n + ow: what is workgroup-uniform
//   src.vector(k)      per vector, BEFORE the feature-row loads are issued
//   src.operand(k)     per vector, after the blend: loads what the operand needs (table rows, the points)
//   src.value(j)       channel j of that operand, already rounded to T; evaluated inside the add loop, in channel order
// A source that selects among its members by a lane's value reads them into locals first (AxisTablePE::operand says why).
// ----------------------------------------------------------------------------------------
template <typename T, bool POOL, typename Src>
__device__ __forceinline__ void token_row_body(const T* __restrict__ feat, const T* __restrict__ newline, T* __restrict__ out,
                                               int64_t out_stride, int side, int n, int C, int newline_on, Src& src) {
  constexpr int VEC = 16 / sizeof(T);
  const int vpt = C / VEC;                      // vectors per token
  const int cols = newline_on ? n + 1 : n;      // output rows per grid row
  const int tok = blockIdx.x;
  const int v = tok / (n * cols);
  const int rem = tok - v * (n * cols);
  const int oh = rem / cols, ow = rem - oh * cols;
  uint4* dst = reinterpret_cast<uint4*>(out + (size_t)tok * out_stride);

  if (ow == n) {  // newline row
    const uint4* nl = reinterpret_cast<const uint4*>(newline);
    for (int k = threadIdx.x; k < vpt; k += blockDim.x) dst[k] = nl[k];
    return;
  }

  const int in_side = POOL ? side : n;
  const T* frame = feat + (size_t)v * in_side * in_side * C;
  Taps th, tw;
  const uint4 *r00, *r01, *r10, *r11;
  if (POOL) {
    th = bilinear_tap(oh, side, n);
    tw = bilinear_tap(ow, side, n);
    r00 = reinterpret_cast<const uint4*>(frame + ((size_t)th.i0 * side + tw.i0) * C);
    r01 = reinterpret_cast<const uint4*>(frame + ((size_t)th.i0 * side + tw.i1) * C);
    r10 = reinterpret_cast<const uint4*>(frame + ((size_t)th.i1 * side + tw.i0) * C);
    r11 = reinterpret_cast<const uint4*>(frame + ((size_t)th.i1 * side + tw.i1) * C);
  } else {
    r00 = reinterpret_cast<const uint4*>(frame + ((size_t)oh * n + ow) * C);
    r01 = r10 = r11 = r00;
  }
  if constexpr (Src::ON) src.token((size_t)(v * n + oh) * n + ow);

  for (int k = threadIdx.x; k < vpt; k += blockDim.x) {
    if constexpr (Src::ON) src.vector(k);
    float x[VEC];
    if (POOL) {
      const uint4 a = r00[k], b = r01[k], c = r10[k], d = r11[k];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float top = __fadd_rn(__fmul_rn(tw.l0, vec_get<T>(a, j)), __fmul_rn(tw.l1, vec_get<T>(b, j)));
        const float bot = __fadd_rn(__fmul_rn(tw.l0, vec_get<T>(c, j)), __fmul_rn(tw.l1, vec_get<T>(d, j)));
        x[j] = round_to<T>(__fadd_rn(__fmul_rn(th.l0, top), __fmul_rn(th.l1, bot)));
      }
    } else {
      const uint4 a = r00[k];
#pragma unroll
      for (int j = 0; j < VEC; ++j) x[j] = vec_get<T>(a, j);
    }
    if constexpr (Src::ON) {
      src.operand(k);
#pragma unroll
      for (int j = 0; j < VEC; ++j) x[j] = __fadd_rn(x[j], src.value(j));
    }
    dst[k] = vec_pack<T>(x);
  }
}

// Host side of the three entry points: the argument checks they share, in one order and wording, the token count and the
// workgroup size.  `who` is the entry point's own name; `vec` the elements of a 16-byte vector; `pe_vectors` the form's own
// vector operand (a table, PE rows), null when it has none.
struct TokenRowPlan { int64_t tokens; int threads; };

inline int plan_token_rows(const char* who, const void* feat, const void* pe_vectors, const void* newline, const void* out,
                           int64_t out_stride, int vec, int V, int side, int n, int C, int flags, TokenRowPlan* plan) {
  const bool pool = flags & V3D_VT_POOL, nl = flags & V3D_VT_NEWLINE;
  V3D_REQUIRE(feat && out, "%s: null pointer", who);
  V3D_REQUIRE(!nl || newline, "%s: NEWLINE needs a newline row", who);
  V3D_REQUIRE(V > 0 && n > 0 && C > 0 && (!pool || side >= n), "%s: bad shape V=%d side=%d n=%d C=%d", who, V, side, n, C);
  V3D_REQUIRE(C % vec == 0, "%s: C=%d must be a multiple of %d", who, C, vec);
  V3D_REQUIRE(out_stride >= C && out_stride % vec == 0, "%s: out_stride=%lld", who, (long long)out_stride);
  V3D_REQUIRE(aligned16(feat) && aligned16(out) && aligned16(pe_vectors) && (!nl || aligned16(newline)),
              "%s: pointers must be 16-byte aligned", who);
  plan->tokens = (int64_t)V * n * (nl ? n + 1 : n);
  V3D_REQUIRE(plan->tokens < (1ll << 31), "%s: too many tokens", who);
  const int vpt = C / vec;
  plan->threads = ((vpt + 63) / 64) * 64;
  if (plan->threads > 512) plan->threads = 512;
  return V3D_OK;
}

}  // namespace v3d
