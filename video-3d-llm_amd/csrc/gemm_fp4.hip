// MXFP4 (OCP MX v1.0: e2m1 codes + one E8M0 exponent per 32 k) weights for the LLM linears.  Not a reference code path (the
// reference runs 16-bit only); the contract is include/v3d.h and tests/test_gpu_fp4.py.
//   W [N, K]  ->  q [N, K/2] bytes (even k in the low nibble)  +  e [N, K/32] bytes (2^(e-127))
//   prefill (W4A8):  y[m,n] = sa[m] * sum_k qa[m,k] * deq(W)[n,k]      qa/sa as v3d_quantize_fp8_rows writes them
//   decode  (W4A16): y[m,n] = sum_k x[m,k] * deq(W)[n,k]               deq(W) widened exactly to the activation type
//
// v_mfma_scale_f32_16x16x128_f8f6f4 with an fp4 first operand (cbsz = 4) and an e4m3 second operand, measured with
// tools/probes/mfma_scale_f4_layout.hip:
//   * fp4 operand: lane l holds row l&15 and the 32 k [32 g, +32), g = l>>4, as 16 bytes in registers 0..3 (registers 4..7 are
//     ignored); nibble i of those 16 bytes (low nibble of a byte first) is k = 32 g + i;
//   * e4m3 operand against it: lane l holds row l&15; bytes 0..15 (registers 0..3) are k = 16 g + 0..15 and bytes 16..31
//     (registers 4..7) are k = 64 + 16 g + 0..15.  (Two e4m3 operands, gemm_fp8.hip, only need the SAME order on both sides,
//     which is why that probe could call it "k-bytes [32 g, +32)"; against an fp4 operand the true order shows.)  The activation
//     fragment is therefore the 16-byte chunks g and 4 + g of the lane's 128-byte row;
//   * the block-scale register is per lane: byte `opsel` of lane l's register scales the 32 k that lane l holds, i.e. exactly
//     one MX block of row l&15.  The public [N, K/32] scale array therefore needs no repack: lane l loads byte
//     e[n0 + l&15][4*kt + (l>>4)] and passes it with opsel 0 (the activation side passes the constant 127 = 2^0);
//   * C/D as every 16x16 MFMA (lane l: column l&15, rows 4*(l>>4) + r).
// v_cvt_scalef32_pk_{bf16,f16,f32}_fp4(src, scale, sel) widens byte `sel` of src: element 0 is the low nibble, element 1 the
// high nibble, multiplied by 2^(exponent field of scale - 127) (the mantissa of the scale is ignored).
//
// Prefill kernel = the shared tile of gemm_q8_tile.h (schedule, epilogue, launch and argument checks live there) with the WfMxfp4
// weight format.  The activation tile keeps its 128-byte rows and XOR swizzle; the weight tile has 64-byte rows (4 chunks of 16
// bytes, chunk ^ ((row >> 2) & 3): the 16 rows that read one chunk together spread over all banks), so a stage is 48 KiB instead of
// 64 and a weight fragment is ONE ds_read_b128.  The 32 KiB that frees stays unused (the epilogue needs 64 KiB, two stages give 96).
// Measured once (profiles/fp4_linears.txt) this kernel takes 1.06-1.12 x gemm_fp8_kernel's time;
// only those end-to-end times were measured, no counters.  HYPOTHESIS, not measured: the four block exponents a lane fetches per
// K-step are single-byte global loads at a row stride of lde (uncoalesced, issued beside the MFMA phases) and cost more than the
// halved weight staging saves.  FOLLOW-UP (open, not a closed design): stage the K-step's [256 x 4] exponent tile (1 KiB) through
// LDS with the weight DMA, or repack the exponents at load so that a lane's four bytes are one dword; the freed LDS also allows
// a third stage.
#include "gemm_q8_tile.h"
#include "decode_common.h"

namespace v3d {

using f4_f32x2 = __attribute__((ext_vector_type(2))) float;

template <typename T, int EPI>
__global__ __launch_bounds__(512, 2) void gemm_mxfp4_kernel(Q8GemmArgs p) { q8_gemm_tile<T, EPI, WfMxfp4>(p); }

// MXFP4 quantiser.  Per block of 32 k: e = clamp(floor(log2(amax)) - 2 + 127, 0, 254) (127 for an all-zero block) - for a finite
// 16-bit input that is the f32 exponent field of amax minus 2, clamped below; elements are w * 2^(127 - e) (exact) rounded to
// the nearest of {0, .5, 1, 1.5, 2, 3, 4, 6} with ties to the even code, saturating at 6; a code of magnitude zero carries no
// sign.  One lane = 8 elements = 4 code bytes; the 4 lanes of a block share its amax.
__device__ __forceinline__ uint32_t f4_code(float w, float mul) {
  const float v = fabsf(w) * mul;
  const uint32_t c = (uint32_t)(v > 0.25f) + (uint32_t)(v >= 0.75f) + (uint32_t)(v > 1.25f) + (uint32_t)(v >= 1.75f) + (uint32_t)(v > 2.5f) +
                     (uint32_t)(v >= 3.5f) + (uint32_t)(v > 5.0f);
  return (c != 0 && w < 0.f) ? (c | 8u) : c;
}

template <typename T>
__global__ __launch_bounds__(256) void quantize_mxfp4_kernel(const T* __restrict__ x, int64_t ldx, int64_t rows, int cols, uint8_t* __restrict__ q,
                                                             int64_t ldq, uint8_t* __restrict__ e, int64_t lde) {
  const int nv = cols / 8;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= rows * nv) return;                      // nv % 4 == 0: the four lanes of a block leave together
  const int64_t row = t / nv;
  const int c = (int)(t - row * nv);
  const uint4 v = reinterpret_cast<const uint4*>(x + row * ldx)[c];
  float f[8], amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) { f[j] = vec_get<T>(v, j); amax = fmaxf(amax, fabsf(f[j])); }
  amax = fmaxf(amax, __shfl_xor(amax, 1));
  amax = fmaxf(amax, __shfl_xor(amax, 2));
  int ex = (int)((__float_as_uint(amax) >> 23) & 0xffu) - 2;
  ex = ex < 0 ? 0 : ex;
  if (amax == 0.f) ex = 127;
  // 2^(127 - ex): exponent field 254 - ex, and 2^-127 (ex = 254, unreachable from a finite 16-bit input) as a subnormal
  const float mul = __uint_as_float(ex < 254 ? (uint32_t)(254 - ex) << 23 : 0x00400000u);
  uint32_t word = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) word |= f4_code(f[j], mul) << (4 * j);
  reinterpret_cast<uint32_t*>(q + row * ldq)[c] = word;
  if ((c & 3) == 0) e[row * lde + (c >> 2)] = (uint8_t)ex;
}

// ---- decode linears (W4A16; the parts around the K loops are decode_common.h's) -------------------------------------------------
__device__ __forceinline__ float f4_scale(uint32_t e) { return __uint_as_float(e << 23); }     // only the exponent field is read

// 8 codes (one 32-bit word, k ascending from the low nibble) times 2^(e-127), as 8 values of the activation type
__device__ __forceinline__ uint4 f4_widen8(bf16_t, uint32_t w, float sc) {
  typedef __bf16 b2 __attribute__((ext_vector_type(2)));
  const b2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 0), p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 1);
  const b2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 2), p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 3);
  return make_uint4(__builtin_bit_cast(uint32_t, p0), __builtin_bit_cast(uint32_t, p1), __builtin_bit_cast(uint32_t, p2), __builtin_bit_cast(uint32_t, p3));
}
__device__ __forceinline__ uint4 f4_widen8(f16_t, uint32_t w, float sc) {
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  const h2 p0 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 0), p1 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 1);
  const h2 p2 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 2), p3 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 3);
  return make_uint4(__builtin_bit_cast(uint32_t, p0), __builtin_bit_cast(uint32_t, p1), __builtin_bit_cast(uint32_t, p2), __builtin_bit_cast(uint32_t, p3));
}

// VALU form (one row; up to 4 rows for shapes without a matrix-core form): linear_decode_fp8_kernel over 4-bit codes.  Workgroup =
// 4 waves = FOUR weight rows, K split over the 256 threads in 16-byte chunks = 32 weights = exactly one MX block; the codes are
// widened to f32 with their block scale by v_cvt_scalef32_pk_f32_fp4 (exact).  Each activation row's arithmetic is the M = 1
// arithmetic, so batching never changes a result bit.
template <typename T, int EPI, int M>
__global__ __launch_bounds__(256, 4) void linear_decode_mxfp4_kernel(
    const T* __restrict__ x, int64_t ldx, const uint8_t* __restrict__ W, int64_t ldw, const uint8_t* __restrict__ E, int64_t lde,
    const T* __restrict__ bias, const T* __restrict__ res, int64_t ldr, T* __restrict__ out, int64_t ldo, int N, int K) {
  __shared__ float red[M][4][4];
  const int tid = threadIdx.x;
  const int kv = K / 32;
  int rows[4];
  const int o0 = dec_valu_rows<EPI>(rows);
  float s[M][4];
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) s[m][r] = 0.f;
  const uint4* wr[4];
  const uint8_t* er[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { wr[r] = reinterpret_cast<const uint4*>(W + (int64_t)rows[r] * ldw); er[r] = E + (int64_t)rows[r] * lde; }
  for (int k = tid; k < kv; k += 256) {
    uint4 w4[4];
    float sc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { w4[r] = ldg_nt(wr[r] + k); sc[r] = f4_scale(__builtin_nontemporal_load(er[r] + k)); }
#pragma unroll
    for (int q = 0; q < 4; ++q) {                   // 8 weights of each row against 8 activations of each activation row
      uint4 xv[M];
#pragma unroll
      for (int m = 0; m < M; ++m) xv[m] = reinterpret_cast<const uint4*>(x + m * ldx)[4 * k + q];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t ww = q == 0 ? w4[r].x : q == 1 ? w4[r].y : q == 2 ? w4[r].z : w4[r].w;
        const f4_f32x2 c0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(ww, sc[r], 0), c1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(ww, sc[r], 1);
        const f4_f32x2 c2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(ww, sc[r], 2), c3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(ww, sc[r], 3);
#pragma unroll
        for (int m = 0; m < M; ++m) {
          s[m][r] = fmaf(c0[0], vec_get<T>(xv[m], 0), s[m][r]);
          s[m][r] = fmaf(c0[1], vec_get<T>(xv[m], 1), s[m][r]);
          s[m][r] = fmaf(c1[0], vec_get<T>(xv[m], 2), s[m][r]);
          s[m][r] = fmaf(c1[1], vec_get<T>(xv[m], 3), s[m][r]);
          s[m][r] = fmaf(c2[0], vec_get<T>(xv[m], 4), s[m][r]);
          s[m][r] = fmaf(c2[1], vec_get<T>(xv[m], 5), s[m][r]);
          s[m][r] = fmaf(c3[0], vec_get<T>(xv[m], 6), s[m][r]);
          s[m][r] = fmaf(c3[1], vec_get<T>(xv[m], 7), s[m][r]);
        }
      }
    }
  }
  dec_valu_tail<T, EPI, M, false>(s, red, rows, o0, nullptr, DecStore<T, EPI>{bias, res, ldr, out, ldo});
}

// Matrix-core form (2..32 rows), as linear_decode_fp8_mfma_kernel: a workgroup owns 16 outputs (SwiGLU: 16 gate + 16 up rows), its 8
// waves split K in tiles of 256.  A tile is 16 rows x 128 BYTES of codes, loaded with full-line coalescing (2 x 16 bytes per lane)
// into the wave-private LDS tile, plus the 8 block exponents of the lane's row (one 8-byte load); the fragment of a k step is
// 4 bytes per lane = 8 codes, widened with the block scale to the activation type by v_cvt_scalef32_pk_{bf16,f16}_fp4 (exact)
// and fed to v_mfma_f32_16x16x32 against the 16-bit activation rows.  Column m of the result depends on row m of x only.
template <typename T, int EPI, int MB>
__global__ __launch_bounds__(512) void linear_decode_mxfp4_mfma_kernel(const T* __restrict__ x, int64_t ldx, int M, const uint8_t* __restrict__ W,
                                                                       int64_t ldw, const uint8_t* __restrict__ E, int64_t lde,
                                                                       const T* __restrict__ bias, const T* __restrict__ res, int64_t ldr,
                                                                       T* __restrict__ out, int64_t ldo, int N, int K) {
  constexpr int RG = EPI == V3D_DEC_SWIGLU ? 2 : 1;
  constexpr int PITCH = 144;
  __shared__ __attribute__((aligned(16))) char tile[8][RG][16 * PITCH];
  __shared__ float part[8][RG][MB][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int lr = lane >> 3, lc = lane & 7;
  const int o0 = blockIdx.x * 16;
  const uint8_t* wbase[RG];
  const uint8_t* ebase[RG];
#pragma unroll
  for (int q = 0; q < RG; ++q) {
    wbase[q] = W + (int64_t)(dec_row0<EPI>(o0) + 64 * q + lr) * ldw + 16 * lc;
    ebase[q] = E + (int64_t)(dec_row0<EPI>(o0) + 64 * q + r) * lde;
  }
  bool col_ok[MB];
  const T* xrow[MB];
  dec_x_rows(x, ldx, M, r, 8 * g, col_ok, xrow);
  dec_f32x4 acc[RG][MB];
#pragma unroll
  for (int q = 0; q < RG; ++q)
#pragma unroll
    for (int b = 0; b < MB; ++b) acc[q][b] = dec_f32x4{0.f, 0.f, 0.f, 0.f};
  const int tiles = K / 256;
  for (int s = wave; s < tiles; s += 8) {
    const int k0 = 256 * s;
    uint4 wreg[RG][2], xb[MB][8];
    uint32_t ex[RG][2];
#pragma unroll
    for (int q = 0; q < RG; ++q) {
#pragma unroll
      for (int j = 0; j < 2; ++j) wreg[q][j] = ldg_nt(reinterpret_cast<const uint4*>(wbase[q] + (int64_t)(8 * j) * ldw + k0 / 2));
      const uint32_t* ep = reinterpret_cast<const uint32_t*>(ebase[q] + k0 / 32);
      ex[q][0] = __builtin_nontemporal_load(ep); ex[q][1] = __builtin_nontemporal_load(ep + 1);
    }
#pragma unroll
    for (int b = 0; b < MB; ++b)
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        xb[b][t] = make_uint4(0u, 0u, 0u, 0u);
        if (col_ok[b]) xb[b][t] = *reinterpret_cast<const uint4*>(xrow[b] + k0 + 32 * t);
      }
#pragma unroll
    for (int q = 0; q < RG; ++q)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        *reinterpret_cast<uint4*>(&tile[wave][q][(8 * j + lr) * PITCH + lc * 16]) = wreg[q][j];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int q = 0; q < RG; ++q) {
        const uint32_t w4 = *reinterpret_cast<const uint32_t*>(&tile[wave][q][r * PITCH + (4 * t + g) * 4]);
        const uint4 a = f4_widen8(T{}, w4, f4_scale((ex[q][t >> 2] >> (8 * (t & 3))) & 0xffu));
#pragma unroll
        for (int b = 0; b < MB; ++b) acc[q][b] = dec_mfma(T{}, a, xb[b][t], acc[q][b]);
      }
  }
  dec_mfma_tail<T, EPI, MB, 1, false>(tid, lane, wave, acc, [&](int w, int q, int b) { return &part[w][q][b][0]; }, o0, M, nullptr,
                                      DecStore<T, EPI>{bias, res, ldr, out, ldo});
}

template <typename T>
static int launch_mxfp4(const Q8GemmArgs& p, int epi, hipStream_t st) {
  return q8_launch<q8_lds_bytes<WfMxfp4>, gemm_mxfp4_kernel<T, Q8_EPI_NONE>, gemm_mxfp4_kernel<T, Q8_EPI_BIAS>, gemm_mxfp4_kernel<T, Q8_EPI_RES>,
                   gemm_mxfp4_kernel<T, Q8_EPI_SWIGLU>>(p, epi, "v3d_gemm_mxfp4", st);
}

}  // namespace v3d

using namespace v3d;

extern "C" int v3d_quantize_mxfp4_rows(const void* w, int64_t ldw, int64_t rows, int cols, int dtype, void* q, int64_t ldq, void* e,
                                       int64_t lde, void* stream) {
  V3D_REQUIRE(w && q && e, "v3d_quantize_mxfp4_rows: null pointer");
  V3D_REQUIRE(rows >= 0 && cols > 0 && cols % 128 == 0, "v3d_quantize_mxfp4_rows: cols=%d must be a multiple of 128", cols);
  V3D_REQUIRE(ldw % 8 == 0 && ldw >= cols && ldq % 4 == 0 && ldq >= cols / 2 && lde >= cols / 32, "v3d_quantize_mxfp4_rows: leading dimensions");
  V3D_REQUIRE(aligned16(w) && (reinterpret_cast<uintptr_t>(q) & 3) == 0, "v3d_quantize_mxfp4_rows: alignment");
  if (rows == 0) return V3D_OK;
  const int64_t threads = rows * (cols / 8);
  V3D_REQUIRE((threads + 255) / 256 < (1ll << 31), "v3d_quantize_mxfp4_rows: matrix too large");
  const unsigned blocks = (unsigned)((threads + 255) / 256);
  if (dtype == V3D_BF16) hipLaunchKernelGGL(quantize_mxfp4_kernel<bf16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w, ldw, rows, cols, (uint8_t*)q, ldq, (uint8_t*)e, lde);
  else if (dtype == V3D_F16) hipLaunchKernelGGL(quantize_mxfp4_kernel<f16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const f16_t*)w, ldw, rows, cols, (uint8_t*)q, ldq, (uint8_t*)e, lde);
  else { set_error("v3d_quantize_mxfp4_rows: dtype must be f16 or bf16"); return V3D_E_INVALID; }
  return check_launch("v3d_quantize_mxfp4_rows");
}

extern "C" int v3d_gemm_mxfp4(const void* A, int64_t lda, const float* scale_a, const void* Wq, int64_t ldw, const void* We, int64_t lde,
                              const void* bias, const void* res, int64_t ldr, void* out, int64_t ldo, int M, int N, int K, int out_dtype,
                              int epilogue, void* stream) {
  const Q8GemmArgs p{(const uint8_t*)A, (const uint8_t*)Wq, (const uint8_t*)We, scale_a, nullptr, bias, res, out, M, N, K, lda, ldw, lde, ldr, ldo, 0, 0};
  if (int rc = q8_validate("v3d_gemm_mxfp4", p, We != nullptr, ldw >= K / 2 && lde >= K / 32, out_dtype, epilogue)) return rc;
  hipStream_t st = (hipStream_t)stream;
  return out_dtype == V3D_BF16 ? launch_mxfp4<bf16_t>(p, epilogue, st) : launch_mxfp4<f16_t>(p, epilogue, st);
}

extern "C" int v3d_linear_decode_mxfp4_rows(const void* x, int64_t ldx, int M, const void* Wq, int64_t ldw, const void* We, int64_t lde,
                                            const void* bias, const void* res, int64_t ldr, void* out, int64_t ldo, int N, int K, int dtype,
                                            int epilogue, void* stream) {
  const char* who = "v3d_linear_decode_mxfp4_rows";
  // one row: VALU form; 2..32 rows: matrix-core form when the shape allows (a row's bits then depend neither on the other rows
  // nor on M); other shapes: VALU form with up to 4 rows
  const bool mfma_ok = K % 256 == 0 && lde % 8 == 0 && (reinterpret_cast<uintptr_t>(We) & 7) == 0 &&
                       (epilogue == V3D_DEC_SWIGLU ? N % 128 == 0 : N % 16 == 0);
  if (int rc = dec_check_rows(who, x && Wq && We && out, dtype, K % 128 == 0 && ldw % 16 == 0 && ldw >= K / 2 && lde >= K / 32, mfma_ok,
                              aligned16(x) && aligned16(Wq), false, ldx, M, N, K, epilogue, bias, res))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  return dec_dispatch(dtype, epilogue, who, [&](auto t, auto e) {
    using T = decltype(t);
    constexpr int E = decltype(e)::value;
    if (mfma_ok && M >= 2) {
      dec_pick<1, 2>(M <= 16 ? 1 : 2, [&](auto b) {
        hipLaunchKernelGGL((linear_decode_mxfp4_mfma_kernel<T, E, decltype(b)::value>), dim3((E == V3D_DEC_SWIGLU ? N / 2 : N) / 16), dim3(512), 0, st,
                           (const T*)x, ldx, M, (const uint8_t*)Wq, ldw, (const uint8_t*)We, lde, (const T*)bias, (const T*)res, ldr, (T*)out, ldo,
                           N, K);
      });
    } else {
      dec_pick<1, 2, 3, 4>(M, [&](auto m) {
        hipLaunchKernelGGL((linear_decode_mxfp4_kernel<T, E, decltype(m)::value>), dim3(N / 4), dim3(256), 0, st, (const T*)x, ldx, (const uint8_t*)Wq,
                           ldw, (const uint8_t*)We, lde, (const T*)bias, (const T*)res, ldr, (T*)out, ldo, N, K);
      });
    }
  });
}
