// The learned 3-D position encoding, PositionEmbeddingMLP (position_encoding.py:52-84):
//     Linear(3, 512) -> LayerNorm(512) -> ReLU -> Linear(512, hidden)      on the aggregated (optionally voxelised) coordinates.
//
//   v3d_pe_mlp_hidden            : the first three stages, one wave per row (the second Linear is v3d_gemm with V3D_EPI_BIAS)
//   v3d_visual_tokens_rows       : v3d_visual_tokens with the PE read from a row tensor instead of a table
//   v3d_visual_tokens_rows_grad  : v3d_visual_tokens_grad + the compact gradient of those PE rows
//   v3d_pe_mlp_wgrad             : dw0[j, a] = sum over rows of dz[r, j] x[r, a], f32, fixed order
//
// The rounding points are the 16-bit torch modules' own ("The MLP position encoding, stated once"):
//     z = T(x w0^T + b0),  h = relu(T(LN(z) g + beta)) with f32 row statistics,  pe = T(h w3^T + b3),  token = T(pooled + pe).
// Compiled with -ffp-contract=off (the bilinear blend rounds like the reference's f32 ops: visual_common.h); the multiply-adds that
// are meant to be fused are written as fmaf.
#include "visual_common.h"

namespace v3d {

constexpr int PE_MLP_HIDDEN = 512;   // PositionEmbeddingMLP.hidden_size: a row is one wave's worth, 8 elements per lane

__device__ __forceinline__ float mlp_wave_sum(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

// One wave per row, rows wave-strided; lane l owns columns 8 l .. 8 l + 7: its 24 weights of w0 [512, 3] are three 16-byte vectors,
// b0 / g / beta one each, all kept in registers over the wave's rows.  K = 3 is three fused multiply-adds per element - on the MFMA
// GEMM it would be padded to 64.  The row statistics follow v3d_layernorm: a plain f32 sum for the mean, then the sum of squared
// differences, each as 8 adds per lane and six shuffle adds.  A row touches no other row's values: a NaN row stays in its row.
template <typename T>
__global__ __launch_bounds__(256) void pe_mlp_hidden_kernel(const T* __restrict__ x, const T* __restrict__ w0, const T* __restrict__ b0,
                                                            const T* __restrict__ ln_w, const T* __restrict__ ln_b, float eps, int64_t N,
                                                            T* __restrict__ z_out, T* __restrict__ h_out) {
  constexpr int H = PE_MLP_HIDDEN;
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
  const uint4* wv = reinterpret_cast<const uint4*>(w0) + lane * 3;
  const uint4 w[3] = {wv[0], wv[1], wv[2]};
  const uint4 bv = reinterpret_cast<const uint4*>(b0)[lane];
  const uint4 gv = reinterpret_cast<const uint4*>(ln_w)[lane];
  const uint4 ev = reinterpret_cast<const uint4*>(ln_b)[lane];
  float wx[8], wy[8], wz[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {     // element 3 j + a of the lane's 24: vector (3 j + a) / 8, slot (3 j + a) % 8
    wx[j] = vec_get<T>(w[(3 * j) >> 3], (3 * j) & 7);
    wy[j] = vec_get<T>(w[(3 * j + 1) >> 3], (3 * j + 1) & 7);
    wz[j] = vec_get<T>(w[(3 * j + 2) >> 3], (3 * j + 2) & 7);
  }
  for (int64_t row = wave; row < N; row += n_waves) {
    const float px = to_f32(x[row * 3]), py = to_f32(x[row * 3 + 1]), pz = to_f32(x[row * 3 + 2]);
    float z[8], s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      z[j] = round_to<T>(fmaf(pz, wz[j], fmaf(py, wy[j], fmaf(px, wx[j], vec_get<T>(bv, j)))));
      s += z[j];
    }
    if (z_out) reinterpret_cast<uint4*>(z_out + row * H)[lane] = vec_pack<T>(z);
    const float mean = mlp_wave_sum(s) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float d = z[j] - mean; q = fmaf(d, d, q); }
    const float rstd = 1.0f / sqrtf(mlp_wave_sum(q) / (float)H + eps);
    float h[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float y = round_to<T>((z[j] - mean) * rstd * vec_get<T>(gv, j) + vec_get<T>(ev, j));
      h[j] = y < 0.0f ? 0.0f : y;             // torch's relu: NaN stays NaN, -0 stays -0 only where y is; 0 for every negative
    }
    reinterpret_cast<uint4*>(h_out + row * H)[lane] = vec_pack<T>(h);
  }
}

// ----------------------------------------------------------------------------------------
// v3d_visual_tokens with PE rows: token_row_body (visual_common.h) with the PE operand read from row (v, oh, ow) of
// pe [V n n, C] (row stride pe_stride) instead of three table rows,
//   PE     : x = T(x + pe[row][channel])
// ----------------------------------------------------------------------------------------
template <typename T>
struct RowPE {
  static constexpr bool ON = true;
  const T* pe;
  int64_t pe_stride;
  const uint4* prow;
  uint4 p;

  __device__ __forceinline__ void token(size_t cell) { prow = reinterpret_cast<const uint4*>(pe + cell * pe_stride); }
  __device__ __forceinline__ void vector(int k) { p = prow[k]; }      // the PE row's load is issued first, ahead of the feature rows
  __device__ __forceinline__ void operand(int) {}
  __device__ __forceinline__ float value(int j) const { return vec_get<T>(p, j); }
};

template <typename T, bool POOL>
__global__ __launch_bounds__(512) void visual_tokens_rows_kernel(const T* __restrict__ feat, const T* __restrict__ pe, int64_t pe_stride,
                                                                 const T* __restrict__ newline, T* __restrict__ out, int64_t out_stride,
                                                                 int side, int n, int C, int newline_on) {
  RowPE<T> src;
  src.pe = pe; src.pe_stride = pe_stride;
  token_row_body<T, POOL>(feat, newline, out, out_stride, side, n, C, newline_on, src);
}

// dpe[(v, oh, ow), :] = dout[(v, oh, ow) among cols = n + 1 | n rows per grid row, :]: the PE add passes the gradient through, the
// newline rows carry none.  One workgroup per compact row, 16-byte copies.
template <typename T>
__global__ __launch_bounds__(256) void pe_rows_grad_kernel(const T* __restrict__ dout, int64_t dstride, T* __restrict__ dpe, int64_t pstride,
                                                           int n, int cols, int C) {
  const int row = blockIdx.x;                 // (v * n + oh) * n + ow
  const int ow = row % n, vh = row / n;
  const uint4* src = reinterpret_cast<const uint4*>(dout + ((size_t)vh * cols + ow) * dstride);
  uint4* dst = reinterpret_cast<uint4*>(dpe + (size_t)row * pstride);
  for (int k = threadIdx.x; k < C / 8; k += 256) dst[k] = src[k];
}

// ----------------------------------------------------------------------------------------
// dw0[j, a] = sum_r dz[r, j] x[r, a]: the partial-sum scheme of v3d_colsum.  partial[b, 3 j + a] = the sum over rows
// [32 b, 32 b + 32) in order (a product of two 16-bit values is exact in f32, so the fused multiply-add rounds once, as an add
// would); the partials are then summed as colsum_final_kernel of train.hip does: thread (c, g) sums every 64th partial in order,
// the 64 group sums are added in order.  No atomics: two runs give the same bits.
// ----------------------------------------------------------------------------------------
constexpr int WG_RPB = 32;

template <typename T>
__global__ __launch_bounds__(64) void pe_mlp_wgrad_partial_kernel(const T* __restrict__ dz, int64_t lddz, const T* __restrict__ x, int64_t rows,
                                                                  float* __restrict__ partial) {
  constexpr int H = PE_MLP_HIDDEN;
  const int lane = threadIdx.x;               // columns 8 lane .. 8 lane + 7
  const int64_t rb = (int64_t)blockIdx.x * WG_RPB;
  float acc[8][3];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 0.f;
  for (int i = 0; i < WG_RPB && rb + i < rows; ++i) {
    const int64_t r = rb + i;
    const uint4 g = reinterpret_cast<const uint4*>(dz + r * lddz)[lane];
    const float px = to_f32(x[r * 3]), py = to_f32(x[r * 3 + 1]), pz = to_f32(x[r * 3 + 2]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = vec_get<T>(g, j);
      acc[j][0] = fmaf(d, px, acc[j][0]);
      acc[j][1] = fmaf(d, py, acc[j][1]);
      acc[j][2] = fmaf(d, pz, acc[j][2]);
    }
  }
  float* o = partial + (int64_t)blockIdx.x * (3 * H) + lane * 24;
#pragma unroll
  for (int j = 0; j < 8; ++j) { o[3 * j] = acc[j][0]; o[3 * j + 1] = acc[j][1]; o[3 * j + 2] = acc[j][2]; }
}

template <typename TO>
__global__ __launch_bounds__(1024) void pe_mlp_wgrad_final_kernel(const float* __restrict__ partial, int64_t n_part, int cols, TO* __restrict__ out) {
  __shared__ float red[64][16];
  const int cl = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  float s = 0.f;
  if (c < cols)
    for (int64_t b = g; b < n_part; b += 64) s += partial[b * cols + c];
  red[g][cl] = s;
  __syncthreads();
  if (g == 0 && c < cols) {
    float t = red[0][cl];
#pragma unroll
    for (int i = 1; i < 64; ++i) t += red[i][cl];
    out[c] = from_f32<TO>(t);
  }
}

}  // namespace v3d

using namespace v3d;

#define V3D_PE_MLP_16(dtype, ...)                                             \
  switch (dtype) {                                                            \
    case V3D_F16: { using T = v3d::f16_t; __VA_ARGS__; } break;               \
    case V3D_BF16: { using T = v3d::bf16_t; __VA_ARGS__; } break;             \
    default: v3d::set_error("16-bit dtypes only (got code %d)", (int)(dtype)); return V3D_E_INVALID; \
  }

extern "C" int v3d_pe_mlp_hidden(const void* x, const void* w0, const void* b0, const void* ln_w, const void* ln_b, float eps, int64_t N,
                                 int hidden, int dtype, void* z, void* h, void* stream) {
  V3D_REQUIRE(x && w0 && b0 && ln_w && ln_b && h, "v3d_pe_mlp_hidden: null pointer");
  V3D_REQUIRE(hidden == PE_MLP_HIDDEN, "v3d_pe_mlp_hidden: hidden=%d, the kernel covers %d (PositionEmbeddingMLP.hidden_size)", hidden, PE_MLP_HIDDEN);
  V3D_REQUIRE(N >= 1 && N < (1ll << 31), "v3d_pe_mlp_hidden: N=%lld", (long long)N);
  V3D_REQUIRE(aligned16(w0) && aligned16(b0) && aligned16(ln_w) && aligned16(ln_b) && aligned16(h) && (!z || aligned16(z)),
              "v3d_pe_mlp_hidden: weights and outputs must be 16-byte aligned");
  int64_t blocks = (N + 15) / 16;              // about four rows per wave: the weights are loaded once per wave
  if (blocks > 2048) blocks = 2048;
  V3D_PE_MLP_16(dtype, hipLaunchKernelGGL(pe_mlp_hidden_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const T*)x,
                                          (const T*)w0, (const T*)b0, (const T*)ln_w, (const T*)ln_b, eps, N, (T*)z, (T*)h));
  return check_launch("v3d_pe_mlp_hidden");
}

extern "C" int v3d_visual_tokens_rows(const void* feat, const void* pe, int64_t pe_stride, const void* newline, void* out, int64_t out_stride,
                                      int dtype, int V, int side, int n, int C, int flags, void* stream) {
  const bool pool = flags & V3D_VT_POOL, nl = flags & V3D_VT_NEWLINE;
  V3D_REQUIRE(pe, "v3d_visual_tokens_rows: null pointer");
  V3D_REQUIRE(!(flags & ~(V3D_VT_POOL | V3D_VT_PE | V3D_VT_NEWLINE)), "v3d_visual_tokens_rows: flags %d (POOL, PE, NEWLINE)", flags);
  TokenRowPlan plan;
  if (int e = plan_token_rows("v3d_visual_tokens_rows", feat, pe, newline, out, out_stride, 8, V, side, n, C, flags, &plan)) return e;
  V3D_REQUIRE(pe_stride >= C && pe_stride % 8 == 0, "v3d_visual_tokens_rows: pe_stride=%lld", (long long)pe_stride);
  hipStream_t st = (hipStream_t)stream;
  V3D_PE_MLP_16(dtype, {
    if (pool) hipLaunchKernelGGL((visual_tokens_rows_kernel<T, true>), dim3((unsigned)plan.tokens), dim3(plan.threads), 0, st, (const T*)feat, (const T*)pe,
                                 pe_stride, (const T*)newline, (T*)out, out_stride, side, n, C, nl ? 1 : 0);
    else hipLaunchKernelGGL((visual_tokens_rows_kernel<T, false>), dim3((unsigned)plan.tokens), dim3(plan.threads), 0, st, (const T*)feat, (const T*)pe,
                            pe_stride, (const T*)newline, (T*)out, out_stride, side, n, C, nl ? 1 : 0);
  });
  return check_launch("v3d_visual_tokens_rows");
}

extern "C" int v3d_visual_tokens_rows_grad(const void* dout, int64_t dout_stride, void* dfeat, float* dnewline, void* dpe, int64_t dpe_stride,
                                           int dtype, int V, int side, int n, int C, int flags, void* stream) {
  V3D_REQUIRE(dpe, "v3d_visual_tokens_rows_grad: null pointer");
  V3D_REQUIRE(dpe_stride >= C && dpe_stride % 8 == 0 && aligned16(dpe), "v3d_visual_tokens_rows_grad: dpe_stride=%lld / alignment", (long long)dpe_stride);
  // dfeat and dnewline: the contract (and the argument checks) of v3d_visual_tokens_grad, whose kernels run unchanged
  if (int e = v3d_visual_tokens_grad(dout, dout_stride, dfeat, dnewline, dtype, V, side, n, C, flags, stream)) return e;
  const int cols = (flags & V3D_VT_NEWLINE) ? n + 1 : n;
  const int64_t rows = (int64_t)V * n * n;
  V3D_REQUIRE(rows < (1ll << 31), "v3d_visual_tokens_rows_grad: too many tokens");
  V3D_PE_MLP_16(dtype, hipLaunchKernelGGL(pe_rows_grad_kernel<T>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, (const T*)dout,
                                          dout_stride, (T*)dpe, dpe_stride, n, cols, C));
  return check_launch("v3d_visual_tokens_rows_grad");
}

extern "C" int64_t v3d_pe_mlp_wgrad_workspace_bytes(int64_t rows, int hidden) {
  if (rows <= 0 || hidden <= 0) return 0;
  return ((rows + WG_RPB - 1) / WG_RPB) * (int64_t)(3 * hidden) * 4;
}

extern "C" int v3d_pe_mlp_wgrad(const void* dz, int64_t lddz, const void* x, int64_t rows, int hidden, int dtype, float* workspace, void* dw0,
                                int out_dtype, void* stream) {
  V3D_REQUIRE(dz && x && workspace && dw0, "v3d_pe_mlp_wgrad: null pointer");
  V3D_REQUIRE(hidden == PE_MLP_HIDDEN, "v3d_pe_mlp_wgrad: hidden=%d, the kernel covers %d", hidden, PE_MLP_HIDDEN);
  V3D_REQUIRE(rows >= 1 && lddz >= hidden && lddz % 8 == 0 && aligned16(dz), "v3d_pe_mlp_wgrad: rows / row stride / alignment");
  const int64_t n_part = (rows + WG_RPB - 1) / WG_RPB;
  V3D_REQUIRE(n_part < (1ll << 31), "v3d_pe_mlp_wgrad: too many rows");
  hipStream_t st = (hipStream_t)stream;
  V3D_PE_MLP_16(dtype, hipLaunchKernelGGL(pe_mlp_wgrad_partial_kernel<T>, dim3((unsigned)n_part), dim3(64), 0, st, (const T*)dz, lddz, (const T*)x,
                                          rows, workspace));
  if (int e = check_launch("v3d_pe_mlp_wgrad")) return e;
  const int cols = 3 * hidden;
  const dim3 grid((cols + 15) / 16);
  switch (out_dtype) {
    case V3D_F32: hipLaunchKernelGGL(pe_mlp_wgrad_final_kernel<float>, grid, dim3(1024), 0, st, workspace, n_part, cols, (float*)dw0); break;
    case V3D_F16: hipLaunchKernelGGL(pe_mlp_wgrad_final_kernel<f16_t>, grid, dim3(1024), 0, st, workspace, n_part, cols, (f16_t*)dw0); break;
    case V3D_BF16: hipLaunchKernelGGL(pe_mlp_wgrad_final_kernel<bf16_t>, grid, dim3(1024), 0, st, workspace, n_part, cols, (bf16_t*)dw0); break;
    default: set_error("v3d_pe_mlp_wgrad: unknown output dtype %d", out_dtype); return V3D_E_INVALID;
  }
  return check_launch("v3d_pe_mlp_wgrad");
}
