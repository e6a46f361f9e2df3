// FP8 (OCP e4m3) path for the LLM linears - BASELINE configs[3] ("fp8 MFMA LLM GEMMs, tolerance re-stated").
// The reference has no fp8 code: this is the bf16 linear  y = x W^T  evaluated as
//     y[m,n] = sa[m] * sw[n] * sum_k qa[m,k] * qw[n,k]          qa = e4m3(x / sa), sa[m] = amax_k |x[m,k]| / 448
// with per-row (token) activation scales and per-output-channel weight scales, f32 accumulation on
// v_mfma_scale_f32_16x16x128_f8f6f4 (block scales pinned to 2^0): twice the MFMA rate of bf16 and half the
// operand bytes through LDS.  Lane layout of that instruction was measured (tools/probes/mfma_scale_f8_layout.hip):
// lane l holds row l&15, k-bytes [32*(l>>4), +32) of A and of B; C/D as every 16x16 MFMA.
//
// The prefill kernel is the shared tile of gemm_q8_tile.h (schedule, epilogue, launch and argument checks live there) with the
// WfE4m3 weight format: a K-step is a 128-byte LDS row on both sides, i.e. the same LDS image, DMA staging and XOR swizzle as the
// bf16 kernel, and a fragment is the 32 bytes = logical chunks 2g, 2g+1 of the lane's row (g = lane>>4).  This file keeps the
// entry point and the e4m3 quantisers.
#include "gemm_q8_tile.h"

namespace v3d {

template <typename T, int EPI>
__global__ __launch_bounds__(512, 2) void gemm_fp8_kernel(Q8GemmArgs p) { q8_gemm_tile<T, EPI, WfE4m3>(p); }

// The e4m3 quantisers share: scale = amax / 448, floored at the smallest normal f32 (1 if the row is zero), and 8 values times
// 1 / scale packed into 8 saturated bytes.  The floor keeps 1 / scale finite: below amax = 448 * 2^-126 the quotient is an f32
// subnormal, its reciprocal inf, and the zeros of such a row would become 0 * inf = the NaN byte.
__device__ __forceinline__ float e4m3_row_scale(float amax) { return amax > 0.f ? fmaxf(amax / 448.0f, 1.17549435e-38f) : 1.0f; }

template <class F>
__device__ __forceinline__ uint2 e4m3_pack8(F at, float inv) {      // at(j) = the j-th value
  int w0 = 0, w1 = 0;
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(at(0) * inv, at(1) * inv, w0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(at(2) * inv, at(3) * inv, w0, true);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(at(4) * inv, at(5) * inv, w1, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(at(6) * inv, at(7) * inv, w1, true);
  return make_uint2((uint32_t)w0, (uint32_t)w1);
}

// Row-wise e4m3 quantisation: scale[r] = max(amax|x[r,:]| / 448, 2^-126) (1 if the row is zero), q = sat_e4m3(x / scale).
// One wave per row, two passes over the row (second pass from L2).
template <typename T>
__global__ __launch_bounds__(256) void quantize_rows_fp8_kernel(const T* __restrict__ x, int64_t ldx, int64_t rows, int cols,
                                                                uint8_t* __restrict__ q, int64_t ldq, float* __restrict__ scale) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const uint4* xr = reinterpret_cast<const uint4*>(x + row * ldx);
  const int nv = cols / 8;
  float amax = 0.f;
  for (int k = lane; k < nv; k += 64) {
    const uint4 v = xr[k];
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(vec_get<T>(v, j)));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
  const float sc = e4m3_row_scale(amax);
  const float inv = 1.0f / sc;
  if (lane == 0) scale[row] = sc;
  uint2* qr = reinterpret_cast<uint2*>(q + row * ldq);
  for (int k = lane; k < nv; k += 64) {
    const uint4 v = xr[k];
    qr[k] = e4m3_pack8([&](int j) { return vec_get<T>(v, j); }, inv);
  }
}

// Long rows (4096 < cols <= 32768, the SwiGLU output): one WORKGROUP per row with the row held in registers between the
// amax reduction and the conversion - one read of the row instead of two.  Same arithmetic as the wave-per-row kernel
// (amax is order-independent), so the results are bit-identical.
template <typename T>
__global__ __launch_bounds__(256) void quantize_row_block_fp8_kernel(const T* __restrict__ x, int64_t ldx, int cols, uint8_t* __restrict__ q,
                                                                     int64_t ldq, float* __restrict__ scale) {
  constexpr int MAXV = 16;                          // 16-byte vectors per thread: 256 x 16 x 8 = 32768 columns
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const uint4* xr = reinterpret_cast<const uint4*>(x + row * ldx);
  const int nv = cols / 8;
  uint4 v[MAXV];
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int k = i * 256 + tid;
    if (k < nv) {
      v[i] = xr[k];
#pragma unroll
      for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(vec_get<T>(v[i], j)));
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
  if ((tid & 63) == 0) red[tid >> 6] = amax;
  __syncthreads();
  amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float sc = e4m3_row_scale(amax);
  const float inv = 1.0f / sc;
  if (tid == 0) scale[row] = sc;
  uint2* qr = reinterpret_cast<uint2*>(q + row * ldq);
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int k = i * 256 + tid;
    if (k < nv) qr[k] = e4m3_pack8([&](int j) { return vec_get<T>(v[i], j); }, inv);
  }
}

// Qwen2RMSNorm (modeling_qwen2.py:85-90) fused with the row-wise e4m3 quantisation of its output: the normalised row
// y = w * T(x * rstd) is formed exactly as v3d_rmsnorm forms it (rounded to T), its amax gives the scale, and only the
// e4m3 image + scale leave the chip (one read of x, half a write) - the 16-bit y is never stored.  One wave per row,
// cols <= 4096.
template <typename T>
__global__ __launch_bounds__(256) void rmsnorm_quantize_fp8_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ w, float eps,
                                                                   int64_t rows, int cols, uint8_t* __restrict__ q, int64_t ldq,
                                                                   float* __restrict__ scale) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nv = cols / 8;
  const uint4* xr = reinterpret_cast<const uint4*>(x + row * ldx);
  uint4 v[8];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = i * 64 + lane;
    if (k < nv) {
      v[i] = xr[k];
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float f = vec_get<T>(v[i], j); ss = fmaf(f, f, ss); }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
  const float r = 1.0f / sqrtf(ss / (float)cols + eps);
  float y[8][8];
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = i * 64 + lane;
    if (k < nv) {
      const uint4 wv = reinterpret_cast<const uint4*>(w)[k];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        y[i][j] = round_to<T>(vec_get<T>(wv, j) * round_to<T>(vec_get<T>(v[i], j) * r));
        amax = fmaxf(amax, fabsf(y[i][j]));
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
  const float sc = e4m3_row_scale(amax);
  const float inv = 1.0f / sc;
  if (lane == 0) scale[row] = sc;
  uint2* qr = reinterpret_cast<uint2*>(q + row * ldq);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = i * 64 + lane;
    if (k < nv) qr[k] = e4m3_pack8([&](int j) { return y[i][j]; }, inv);
  }
}

template <typename T>
static int launch_fp8(const Q8GemmArgs& p, int epi, hipStream_t st) {
  return q8_launch<q8_lds_bytes<WfE4m3>, gemm_fp8_kernel<T, Q8_EPI_NONE>, gemm_fp8_kernel<T, Q8_EPI_BIAS>, gemm_fp8_kernel<T, Q8_EPI_RES>,
                   gemm_fp8_kernel<T, Q8_EPI_SWIGLU>>(p, epi, "v3d_gemm_fp8", st);
}

}  // namespace v3d

using namespace v3d;

extern "C" int v3d_quantize_fp8_rows(const void* x, int64_t ldx, int64_t rows, int cols, int dtype, void* q, int64_t ldq,
                                     float* scale, void* stream) {
  V3D_REQUIRE(x && q && scale, "v3d_quantize_fp8_rows: null pointer");
  V3D_REQUIRE(rows >= 0 && cols > 0 && cols % 8 == 0 && ldx % 8 == 0 && ldq % 8 == 0 && ldq >= cols, "v3d_quantize_fp8_rows: bad shape");
  V3D_REQUIRE(aligned16(x) && (reinterpret_cast<uintptr_t>(q) & 7) == 0, "v3d_quantize_fp8_rows: alignment");
  if (rows == 0) return V3D_OK;
  if (cols > 4096 && cols <= 32768 && rows < (1ll << 31)) {       // long rows: one workgroup per row, single read
    if (dtype == V3D_BF16) hipLaunchKernelGGL(quantize_row_block_fp8_kernel<bf16_t>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, cols, (uint8_t*)q, ldq, scale);
    else if (dtype == V3D_F16) hipLaunchKernelGGL(quantize_row_block_fp8_kernel<f16_t>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, (const f16_t*)x, ldx, cols, (uint8_t*)q, ldq, scale);
    else { set_error("v3d_quantize_fp8_rows: dtype must be f16 or bf16"); return V3D_E_INVALID; }
    return check_launch("v3d_quantize_fp8_rows");
  }
  const unsigned blocks = (unsigned)((rows + 3) / 4);
  if (dtype == V3D_BF16) hipLaunchKernelGGL(quantize_rows_fp8_kernel<bf16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, rows, cols, (uint8_t*)q, ldq, scale);
  else if (dtype == V3D_F16) hipLaunchKernelGGL(quantize_rows_fp8_kernel<f16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const f16_t*)x, ldx, rows, cols, (uint8_t*)q, ldq, scale);
  else { set_error("v3d_quantize_fp8_rows: dtype must be f16 or bf16"); return V3D_E_INVALID; }
  return check_launch("v3d_quantize_fp8_rows");
}

extern "C" int v3d_gemm_fp8(const void* A, int64_t lda, const float* scale_a, const void* W, int64_t ldw, const float* scale_w,
                            const void* bias, const void* res, int64_t ldr, void* out, int64_t ldo, int M, int N, int K,
                            int out_dtype, int epilogue, void* stream) {
  const Q8GemmArgs p{(const uint8_t*)A, (const uint8_t*)W, nullptr, scale_a, scale_w, bias, res, out, M, N, K, lda, ldw, 0, ldr, ldo, 0, 0};
  if (int rc = q8_validate("v3d_gemm_fp8", p, scale_w != nullptr, ldw >= K, out_dtype, epilogue)) return rc;
  hipStream_t st = (hipStream_t)stream;
  return out_dtype == V3D_BF16 ? launch_fp8<bf16_t>(p, epilogue, st) : launch_fp8<f16_t>(p, epilogue, st);
}

extern "C" int v3d_rmsnorm_quantize_fp8(const void* x, int64_t ldx, const void* weight, float eps, int64_t rows, int cols, int dtype,
                                        void* q, int64_t ldq, float* scale, void* stream) {
  V3D_REQUIRE(x && weight && q && scale, "v3d_rmsnorm_quantize_fp8: null pointer");
  V3D_REQUIRE(rows >= 0 && cols > 0 && cols % 8 == 0 && cols <= 4096, "v3d_rmsnorm_quantize_fp8: cols=%d unsupported", cols);
  V3D_REQUIRE(ldx % 8 == 0 && ldq % 8 == 0 && aligned16(x) && aligned16(weight) && (reinterpret_cast<uintptr_t>(q) & 7) == 0,
              "v3d_rmsnorm_quantize_fp8: alignment");
  if (rows == 0) return V3D_OK;
  const unsigned blocks = (unsigned)((rows + 3) / 4);
  if (dtype == V3D_BF16) hipLaunchKernelGGL(rmsnorm_quantize_fp8_kernel<bf16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, (const bf16_t*)weight, eps, rows, cols, (uint8_t*)q, ldq, scale);
  else if (dtype == V3D_F16) hipLaunchKernelGGL(rmsnorm_quantize_fp8_kernel<f16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const f16_t*)x, ldx, (const f16_t*)weight, eps, rows, cols, (uint8_t*)q, ldq, scale);
  else { set_error("v3d_rmsnorm_quantize_fp8: dtype must be f16 or bf16"); return V3D_E_INVALID; }
  return check_launch("v3d_rmsnorm_quantize_fp8");
}
