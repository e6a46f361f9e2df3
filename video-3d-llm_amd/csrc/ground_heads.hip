// Training kernels of the 'mlp' and 'score' grounding heads (llava_qwen.py:59-86, 283-293, 313-322) beside the infonce loss of train.hip:
//   v3d_ground_rowdot_bce   the score tail of both heads and its BCE loss in one launch: s_i = sum_c X[i, c] w[c] (+ bias),
//                           loss = mean_i weight_i (max(s_i, 0) - s_i t_i + log1p(e^-|s_i|)), and dX = ds (x) w, dw = sum_i ds_i X_i,
//                           dbias = sum_i ds_i with ds_i = weight_i (sigmoid(s_i) - t_i) / n.  'mlp': X = the object features,
//                           w = the head's query output (products rounded to the dtype, `(q * obj).sum(-1)`), so dw = dq; 'score':
//                           X = the scoring MLP's LayerNorm-ReLU rows, w / bias = ground_head_score.3.
//   v3d_mul_rows_grad       backward of m = o * q_row (`obj_feat * query_feat`): do = dm * q, dq = sum_i dm_i * o_i.
// Small row work: v3d_ground_rowdot_bce is ONE workgroup (the loss needs every score before any gradient), so it is bound by latency,
// not by HBM bandwidth; v3d_mul_rows_grad streams its rows over C / 256 workgroups.  Every sum is folded in a fixed order (no atomics),
// so two calls give identical bits.
#include "v3d_common.h"

namespace v3d {

namespace {

constexpr int RB_THREADS = 1024, RB_WAVES = RB_THREADS / 64, RB_MAX_N = 1024, RB_MAX_C = 3584;

__device__ __forceinline__ float gh_wave_sum(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

}  // namespace

// One workgroup of 16 waves; n <= 1024 rows, C <= 3584 columns in 8-wide vectors.
//   1. scores: one wave per row (rows i = wave, wave + 16, ...), each lane sums its vectors in order, then a butterfly over the wave;
//   2. wave 0: the loss terms and ds_i (lane-strided, butterfly), sum ds_i = dbias;
//   3. dX rows as in 1; dw: G = min(1024 / (C / 8), n) row groups, group g sums the rows g, g + G, ... in order for its column
//      vector, the G partials (<= 1024 * 8 floats of LDS) are added in group order.
template <typename T, bool ROUNDED>
__global__ __launch_bounds__(RB_THREADS) void ground_rowdot_bce_kernel(const T* __restrict__ X, int64_t ldx, int n, const T* __restrict__ w, int C,
                                                                       const T* __restrict__ bias, const uint8_t* __restrict__ positive, float pos_weight,
                                                                       float* __restrict__ loss, float* __restrict__ scores, T* __restrict__ dX,
                                                                       int64_t lddx, T* __restrict__ dw, T* __restrict__ dbias) {
  __shared__ float s_ds[RB_MAX_N];
  __shared__ float s_part[RB_THREADS * 8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nv = C / 8;
  const float b = bias ? to_f32(bias[0]) : 0.f;
  for (int i = wave; i < n; i += RB_WAVES) {
    const T* row = X + (int64_t)i * ldx;
    float acc = 0.f;
    for (int k = lane; k < nv; k += 64) {
      const uint4 xv = *reinterpret_cast<const uint4*>(row + k * 8);
      const uint4 wv = *reinterpret_cast<const uint4*>(w + k * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float pr = vec_get<T>(xv, j) * vec_get<T>(wv, j);
        acc += ROUNDED ? round_to<T>(pr) : pr;
      }
    }
    acc = gh_wave_sum(acc);
    if (lane == 0) s_ds[i] = acc + b;                                  // the score, replaced by ds_i below
  }
  __syncthreads();
  if (wave == 0) {
    const float inv_n = 1.0f / (float)n;
    float l = 0.f, db = 0.f;
    for (int i = lane; i < n; i += 64) {                               // each lane reads and rewrites only its own entries
      const float s = s_ds[i];
      const bool t = positive[i] != 0;
      const float wt = t ? pos_weight : 1.0f;
      const float e = expf(-fabsf(s));                                 // in (0, 1]: no overflow for any logit
      l += wt * (fmaxf(s, 0.f) - (t ? s : 0.f) + log1pf(e));
      const float sig = s >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
      const float ds = wt * (sig - (t ? 1.0f : 0.f)) * inv_n;
      if (scores) scores[i] = s;
      s_ds[i] = ds;
      db += ds;
    }
    l = gh_wave_sum(l);
    db = gh_wave_sum(db);
    if (lane == 0) {
      *loss = l * inv_n;
      if (dbias) *dbias = from_f32<T>(db);
    }
  }
  __syncthreads();
  for (int i = wave; i < n; i += RB_WAVES) {
    const float ds = s_ds[i];
    T* drow = dX + (int64_t)i * lddx;
    for (int k = lane; k < nv; k += 64) {
      const uint4 wv = *reinterpret_cast<const uint4*>(w + k * 8);
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = ds * vec_get<T>(wv, j);
      *reinterpret_cast<uint4*>(drow + k * 8) = vec_pack<T>(o);
    }
  }
  const int G = min(RB_THREADS / nv, n);
  const int g = tid / nv, k = tid - g * nv;
  if (g < G) {
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = g; i < n; i += G) {
      const float ds = s_ds[i];
      const uint4 xv = *reinterpret_cast<const uint4*>(X + (int64_t)i * ldx + k * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = fmaf(ds, vec_get<T>(xv, j), a[j]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) s_part[g * C + k * 8 + j] = a[j];      // g * C + C <= (1024 / nv) * nv * 8
  }
  __syncthreads();
  for (int c = tid; c < C; c += RB_THREADS) {
    float a = 0.f;
    for (int gg = 0; gg < G; ++gg) a += s_part[gg * C + c];
    dw[c] = from_f32<T>(a);
  }
}

// 256 threads = 32 column vectors of 8 x 8 row groups; workgroup x takes the columns [256 x, 256 x + 256).  Row group g walks the
// rows g, g + 8, ... in order: do = dm * q (one rounding), dq partials in f32; the 8 partials are added in group order.
template <typename T>
__global__ __launch_bounds__(256) void mul_rows_grad_kernel(const T* __restrict__ dm, int64_t lddm, const T* __restrict__ o, int64_t ldo,
                                                            const T* __restrict__ q, int n, int C, T* __restrict__ dout, int64_t lddo,
                                                            T* __restrict__ dq) {
  __shared__ float s_part[8 * 256];
  const int tid = threadIdx.x, kk = tid & 31, g = tid >> 5;
  const int k = blockIdx.x * 32 + kk;
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (k < C / 8) {
    const uint4 qv = *reinterpret_cast<const uint4*>(q + k * 8);
    for (int i = g; i < n; i += 8) {
      const uint4 dv = *reinterpret_cast<const uint4*>(dm + (int64_t)i * lddm + k * 8);
      const uint4 ov = *reinterpret_cast<const uint4*>(o + (int64_t)i * ldo + k * 8);
      float r[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = vec_get<T>(dv, j);
        r[j] = d * vec_get<T>(qv, j);
        a[j] = fmaf(d, vec_get<T>(ov, j), a[j]);
      }
      *reinterpret_cast<uint4*>(dout + (int64_t)i * lddo + k * 8) = vec_pack<T>(r);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) s_part[g * 256 + kk * 8 + j] = a[j];
  __syncthreads();
  const int c = blockIdx.x * 256 + tid;
  if (c < C) {
    float s = 0.f;
#pragma unroll
    for (int gg = 0; gg < 8; ++gg) s += s_part[gg * 256 + tid];
    dq[c] = from_f32<T>(s);
  }
}

}  // namespace v3d

using namespace v3d;

extern "C" int v3d_ground_rowdot_bce(const void* x, int64_t ldx, int n, const void* w, int C, const void* bias, int products_rounded,
                                     const uint8_t* positive, float pos_weight, float* loss, float* scores, void* dx, int64_t lddx, void* dw,
                                     void* dbias, int dtype, void* stream) {
  V3D_REQUIRE(x && w && positive && loss && dx && dw, "v3d_ground_rowdot_bce: null pointer");
  V3D_REQUIRE(n >= 1 && n <= RB_MAX_N && C >= 8 && C <= RB_MAX_C && C % 8 == 0, "v3d_ground_rowdot_bce: 1 to %d rows, C a multiple of 8 up to %d (n=%d, C=%d)",
              RB_MAX_N, RB_MAX_C, n, C);
  V3D_REQUIRE(ldx >= C && lddx >= C && ldx % 8 == 0 && lddx % 8 == 0 && aligned16(x) && aligned16(w) && aligned16(dx),
              "v3d_ground_rowdot_bce: rows must be 16-byte aligned (ld a multiple of 8, >= C)");
  V3D_REQUIRE(x != dx, "v3d_ground_rowdot_bce: dx must not overwrite x");
  V3D_REQUIRE(dtype == V3D_F16 || dtype == V3D_BF16, "v3d_ground_rowdot_bce: dtype must be f16 or bf16");
  hipStream_t st = (hipStream_t)stream;
#define V3D_RB(T, R) hipLaunchKernelGGL((ground_rowdot_bce_kernel<T, R>), dim3(1), dim3(RB_THREADS), 0, st, (const T*)x, ldx, n, (const T*)w, C, \
                                        (const T*)bias, positive, pos_weight, loss, scores, (T*)dx, lddx, (T*)dw, (T*)dbias)
  if (dtype == V3D_BF16) { if (products_rounded) V3D_RB(bf16_t, true); else V3D_RB(bf16_t, false); }
  else { if (products_rounded) V3D_RB(f16_t, true); else V3D_RB(f16_t, false); }
#undef V3D_RB
  return check_launch("v3d_ground_rowdot_bce");
}

extern "C" int v3d_mul_rows_grad(const void* dm, int64_t lddm, const void* o, int64_t ldo, const void* q, int n, int C, void* dout, int64_t lddo,
                                 void* dq, int dtype, void* stream) {
  V3D_REQUIRE(dm && o && q && dout && dq, "v3d_mul_rows_grad: null pointer");
  V3D_REQUIRE(n >= 1 && C >= 8 && C % 8 == 0, "v3d_mul_rows_grad: n >= 1 rows, C a multiple of 8 (n=%d, C=%d)", n, C);
  V3D_REQUIRE(lddm >= C && ldo >= C && lddo >= C && lddm % 8 == 0 && ldo % 8 == 0 && lddo % 8 == 0 && aligned16(dm) && aligned16(o) &&
              aligned16(q) && aligned16(dout), "v3d_mul_rows_grad: rows must be 16-byte aligned (ld a multiple of 8, >= C)");
  V3D_REQUIRE(dtype == V3D_F16 || dtype == V3D_BF16, "v3d_mul_rows_grad: dtype must be f16 or bf16");
  const dim3 grid((unsigned)((C / 8 + 31) / 32));
  if (dtype == V3D_BF16) hipLaunchKernelGGL(mul_rows_grad_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dm, lddm, (const bf16_t*)o, ldo,
                                            (const bf16_t*)q, n, C, (bf16_t*)dout, lddo, (bf16_t*)dq);
  else hipLaunchKernelGGL(mul_rows_grad_kernel<f16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const f16_t*)dm, lddm, (const f16_t*)o, ldo,
                          (const f16_t*)q, n, C, (f16_t*)dout, lddo, (f16_t*)dq);
  return check_launch("v3d_mul_rows_grad");
}
