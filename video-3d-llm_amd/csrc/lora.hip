// LoRA rank products on the MFMA units (gfx950): the two products of an adapted Linear in which one dimension is the rank.
// For y = x W^T + s (x A^T) B^T with A [r, K], B [N, r] (peft's LoraLayer; llava/train/train_3d.py:168-173 lora_r 64, lora_alpha 16):
//
//   v3d_lora_down   out[M, R] = T(scale * X[M, K] . P[R, K]^T)          u = x A^T, and du = s dy B against the transposed copy of B
//   v3d_lora_wgrad  G[R, K]   = scale * U[M, R]^T . X[M, K]             dA = du^T x, and dB^T = s u^T dy; the sum runs over the M token rows
//
// R (the rank, or the stacked rank of fused q|k|v / gate|up rows) is 16 .. 384 in steps of 16, K a multiple of 64, M anything.
//
// down.   One workgroup (4 waves) owns 32 rows of X and ALL R columns, so X - the only large operand - is read once, and M = 6794 gives
//         213 workgroups.  Per 64-wide K step the 32 x 64 piece of X and the R x 64 piece of P go through registers into LDS (144-byte
//         rows: the ds_read_b128 of 16 rows then touches 16 different 16-byte slots); the loads of step t + 1 are issued before the MFMAs
//         of step t.  Both operands are K-contiguous, which is the 16 x 16 x 32 operand order (lane l: row l & 15, k = 8 (l >> 4) + j).
//         Wave w owns the 16-column blocks w, w + 4, ...; every output has ONE accumulator and k runs ascending through it.
// wgrad.  Both operands are stored with the summed index (the token row) as their ROW, the wrong way round for an MFMA operand; they are
//         staged as stored ([32 rows][R] and [32 rows][64]) and read back through the hardware transpose (ds_read_b64_tr_b16: two reads
//         give the 8 consecutive rows of one column a lane needs), so no transposed copy is made in HBM.  The grid is (K / 64) x chunks:
//         a workgroup sums rows [c chunk, (c + 1) chunk) for 64 columns of X and all R rows of G (wave w: columns 16 w .. 16 w + 15, up
//         to 24 accumulator tiles) and stores its f32 partial slab [R][64] into workspace[c] with plain stores.  A second launch adds the
//         slabs in chunk order, scales once and rounds once.  No atomics, no counters, nothing passed between workgroups inside a launch:
//         two calls give the same bits.  Rows past M are never read (the staging pass clamps the address and stores zeros instead).
#include "v3d_common.h"

namespace v3d {

using lora_bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using lora_f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using lora_f32x4 = __attribute__((ext_vector_type(4))) float;
using lora_s16x4 = __attribute__((ext_vector_type(4))) short;
using lora_s16x8 = __attribute__((ext_vector_type(8))) short;

template <typename T> struct LoraMfma;
template <> struct LoraMfma<bf16_t> {
  using frag = lora_bf16x8;
  static __device__ __forceinline__ lora_f32x4 run(frag a, frag b, lora_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct LoraMfma<f16_t> {
  using frag = lora_f16x8;
  static __device__ __forceinline__ lora_f32x4 run(frag a, frag b, lora_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

constexpr int LORA_BM = 32;        // rows of X per workgroup (down) and per step of the sum (wgrad)
constexpr int LORA_BK = 64;        // K step (down) and columns of X per workgroup (wgrad)
constexpr int LORA_ROW = 72;       // LDS row of a 64-wide piece, in elements: 128 bytes of data + 16 of padding
constexpr int LORA_MAX_R = 384;
constexpr int LORA_WG_TARGET = 512;   // workgroups the wgrad grid aims at (two per compute unit)

// ----------------------------------------------------------------------------------------------------------------------- down

template <typename T, int CF>          // CF 16-column blocks per wave: R <= 64 CF
__global__ __launch_bounds__(256) void lora_down_kernel(const T* __restrict__ X, int64_t ldx, const T* __restrict__ P, int64_t ldp, float scale,
                                                        T* __restrict__ out, int64_t ldo, int M, int R, int K) {
  using MF = LoraMfma<T>;
  using frag = typename MF::frag;
  constexpr int RP = 64 * CF;          // rows of the P piece in LDS (rows past R repeat row R - 1; their columns are never stored)
  __shared__ __attribute__((aligned(16))) uint16_t smem[(LORA_BM + RP) * LORA_ROW];
  uint16_t* sx = smem;
  uint16_t* sp = smem + LORA_BM * LORA_ROW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * LORA_BM;
  const int sr = tid >> 3, sc = (tid & 7) * 8;           // this thread's 16-byte chunk of a 32-row x 64-column piece
  int64_t xr = m0 + sr;
  if (xr > M - 1) xr = M - 1;                            // rows past M: row M - 1 again (never stored)
  const T* xsrc = X + xr * ldx + sc;
  const T* psrc[2 * CF];
#pragma unroll
  for (int i = 0; i < 2 * CF; ++i) {
    int pr = sr + 32 * i;
    if (pr > R - 1) pr = R - 1;
    psrc[i] = P + (int64_t)pr * ldp + sc;
  }
  lora_f32x4 acc[CF][2];
#pragma unroll
  for (int c = 0; c < CF; ++c) acc[c][0] = acc[c][1] = lora_f32x4{0.f, 0.f, 0.f, 0.f};

  uint4 vx = *reinterpret_cast<const uint4*>(xsrc);
  uint4 vp[2 * CF];
#pragma unroll
  for (int i = 0; i < 2 * CF; ++i) vp[i] = *reinterpret_cast<const uint4*>(psrc[i]);

  const int fr = lane & 15, fk = (lane >> 4) * 8;
  for (int k0 = 0; k0 < K; k0 += LORA_BK) {
    __syncthreads();                                     // the previous step's fragment reads are done
    *reinterpret_cast<uint4*>(sx + sr * LORA_ROW + sc) = vx;
#pragma unroll
    for (int i = 0; i < 2 * CF; ++i) *reinterpret_cast<uint4*>(sp + (sr + 32 * i) * LORA_ROW + sc) = vp[i];
    __syncthreads();
    const int kn = k0 + LORA_BK < K ? k0 + LORA_BK : k0;  // the next step's loads fly under this step's MFMAs (the last step repeats its own)
    vx = *reinterpret_cast<const uint4*>(xsrc + kn);
#pragma unroll
    for (int i = 0; i < 2 * CF; ++i) vp[i] = *reinterpret_cast<const uint4*>(psrc[i] + kn);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const frag a0 = *reinterpret_cast<const frag*>(sx + fr * LORA_ROW + ks * 32 + fk);
      const frag a1 = *reinterpret_cast<const frag*>(sx + (fr + 16) * LORA_ROW + ks * 32 + fk);
#pragma unroll
      for (int c = 0; c < CF; ++c) {
        const frag b = *reinterpret_cast<const frag*>(sp + ((wave + 4 * c) * 16 + fr) * LORA_ROW + ks * 32 + fk);
        acc[c][0] = MF::run(a0, b, acc[c][0]);
        acc[c][1] = MF::run(a1, b, acc[c][1]);
      }
    }
  }
  // accumulator element j of lane l: row 4 (l >> 4) + j, column l & 15
#pragma unroll
  for (int c = 0; c < CF; ++c) {
    const int col = (wave + 4 * c) * 16 + fr;
    if (col >= R) continue;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t row = m0 + 16 * h + 4 * (lane >> 4) + j;
        if (row < M) out[row * ldo + col] = from_f32<T>(scale * acc[c][h][j]);
      }
  }
}

// ----------------------------------------------------------------------------------------------------------------------- wgrad

// One 16 x 32 operand whose 32 summed indices are ROWS of the LDS image: lane l (group g = l >> 4, i = l & 15) gets column c0 + i of rows
// 8 g .. 8 g + 7 in its elements 0 .. 7.  Lane 4 q + p of a group supplies the address of row q, columns 4 p .. 4 p + 3 of the 4-row block.
template <typename F>
__device__ __forceinline__ F lora_tr_frag(const uint16_t* image, int row_elems, int c0, int lane) {
  using lds_ptr = __attribute__((address_space(3))) lora_s16x4*;
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const uint16_t* a = image + (8 * g + q) * row_elems + c0 + 4 * p;
  const lora_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)a);
  const lora_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(a + 4 * row_elems));
  const lora_s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(F, v);
}

template <typename T, int RB>          // RB 16-row blocks of G: R <= 16 RB
__global__ __launch_bounds__(256) void lora_wgrad_partial_kernel(const T* __restrict__ U, int64_t ldu, const T* __restrict__ X, int64_t ldx,
                                                                 float* __restrict__ slabs, int M, int R, int K, int chunk) {
  using MF = LoraMfma<T>;
  using frag = typename MF::frag;
  constexpr int UROW = 16 * RB + 8;    // LDS row of the U piece, in elements
  constexpr int UCH = 2 * RB;          // its 16-byte chunks per row
  constexpr int UPT = RB / 4;          // chunks per thread (32 rows x UCH chunks over 256 threads)
  __shared__ __attribute__((aligned(16))) uint16_t smem[LORA_BM * (UROW + LORA_ROW)];
  uint16_t* su = smem;
  uint16_t* sx = smem + LORA_BM * UROW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * LORA_BK;
  const int r_begin = blockIdx.y * chunk;
  const int r_end = r_begin + chunk < M ? r_begin + chunk : M;
  const int sr = tid >> 3, sc = (tid & 7) * 8;
  int ur[UPT], uc[UPT];
  bool ucol_ok[UPT];
#pragma unroll
  for (int i = 0; i < UPT; ++i) {
    const int idx = tid + 256 * i;
    ur[i] = idx / UCH;
    uc[i] = (idx % UCH) * 8;
    ucol_ok[i] = uc[i] < R;            // columns R .. 16 RB - 1 of the image are zeros, never loaded
  }
  lora_f32x4 acc[RB];
#pragma unroll
  for (int b = 0; b < RB; ++b) acc[b] = lora_f32x4{0.f, 0.f, 0.f, 0.f};
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);

  for (int r0 = r_begin; r0 < r_end; r0 += LORA_BM) {
    // rows at or past r_end: the address is clamped to the last row of the chunk and zeros are stored instead of what came back
    int xrow = r0 + sr;
    const bool xok = xrow < r_end;
    if (!xok) xrow = r_end - 1;
    uint4 vx = *reinterpret_cast<const uint4*>(X + (int64_t)xrow * ldx + n0 + sc);
    if (!xok) vx = zero;
    uint4 vu[UPT];
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      int row = r0 + ur[i];
      const bool ok = row < r_end && ucol_ok[i];
      if (row > r_end - 1) row = r_end - 1;
      const int col = ucol_ok[i] ? uc[i] : 0;
      vu[i] = *reinterpret_cast<const uint4*>(U + (int64_t)row * ldu + col);
      if (!ok) vu[i] = zero;
    }
    __syncthreads();                                     // the previous step's fragment reads are done
    *reinterpret_cast<uint4*>(sx + sr * LORA_ROW + sc) = vx;
#pragma unroll
    for (int i = 0; i < UPT; ++i) *reinterpret_cast<uint4*>(su + ur[i] * UROW + uc[i]) = vu[i];
    __syncthreads();
    const frag b = lora_tr_frag<frag>(sx, LORA_ROW, 16 * wave, lane);
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const frag a = lora_tr_frag<frag>(su, UROW, 16 * rb, lane);
      acc[rb] = MF::run(a, b, acc[rb]);
    }
  }
  float* slab = slabs + (int64_t)blockIdx.y * R * K;
  const int col = n0 + 16 * wave + (lane & 15);
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = 16 * rb + 4 * (lane >> 4) + j;
      if (row < R) slab[(int64_t)row * K + col] = acc[rb][j];
    }
}

template <typename TO> __device__ __forceinline__ void lora_store4(TO* dst, const float* v);
template <> __device__ __forceinline__ void lora_store4<float>(float* dst, const float* v) {
  *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void lora_store4<f16_t>(f16_t* dst, const float* v) {
  *reinterpret_cast<uint2*>(dst) = make_uint2(pack2<f16_t>(v[0], v[1]), pack2<f16_t>(v[2], v[3]));
}
template <> __device__ __forceinline__ void lora_store4<bf16_t>(bf16_t* dst, const float* v) {
  *reinterpret_cast<uint2*>(dst) = make_uint2(pack2<bf16_t>(v[0], v[1]), pack2<bf16_t>(v[2], v[3]));
}

// G[r, k .. k + 3] = TO(scale * (slab 0 + slab 1 + ... in chunk order)); one thread per four columns
template <typename TO>
__global__ __launch_bounds__(256) void lora_wgrad_sum_kernel(const float* __restrict__ slabs, int n_chunks, float scale, TO* __restrict__ G,
                                                             int64_t ldg, int R, int K) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int kq = K / 4;
  if (i >= (int64_t)R * kq) return;
  const int r = (int)(i / kq), k = (int)(i % kq) * 4;
  const int64_t slab_elems = (int64_t)R * K;
  const float* src = slabs + (int64_t)r * K + k;
  float4 s = *reinterpret_cast<const float4*>(src);
  for (int c = 1; c < n_chunks; ++c) {
    const float4 t = *reinterpret_cast<const float4*>(src + c * slab_elems);
    s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
  }
  const float v[4] = {scale * s.x, scale * s.y, scale * s.z, scale * s.w};
  lora_store4<TO>(G + (int64_t)r * ldg + k, v);
}

// rows of the sum per workgroup: K / 64 column slabs times the chunks give about LORA_WG_TARGET workgroups; a multiple of the 32-row step
static int64_t lora_chunks_wanted(int K) {
  const int64_t kt = K / LORA_BK;
  return (LORA_WG_TARGET + kt - 1) / kt;
}
static bool lora_shape_ok(int64_t M, int R, int K) {
  return M >= 1 && M < (1ll << 31) && R >= 16 && R <= LORA_MAX_R && R % 16 == 0 && K >= LORA_BK && K % LORA_BK == 0;
}
// rows * ld < 2^31 without forming the product (ld is the caller's: rows >= 1 here)
static bool lora_span_ok(int64_t rows, int64_t ld) { return ld < ((1ll << 31) + rows - 1) / rows; }
static int64_t lora_chunk_rows(int64_t M, int K) {
  const int64_t want = lora_chunks_wanted(K);
  const int64_t c = (M + want - 1) / want;
  return (c + LORA_BM - 1) / LORA_BM * LORA_BM;
}

}  // namespace v3d

using namespace v3d;

#define V3D_LORA_16(dtype, ...)                                               \
  switch (dtype) {                                                            \
    case V3D_F16: { using T = v3d::f16_t; __VA_ARGS__; } break;               \
    case V3D_BF16: { using T = v3d::bf16_t; __VA_ARGS__; } break;             \
    default: v3d::set_error("16-bit dtypes only (got code %d)", (int)(dtype)); return V3D_E_INVALID; \
  }

extern "C" int v3d_lora_down(const void* X, int64_t ldx, const void* P, int64_t ldp, float scale, void* out, int64_t ldo, int64_t M, int R,
                             int K, int dtype, void* stream) {
  V3D_REQUIRE(X && P && out, "v3d_lora_down: null pointer");
  V3D_REQUIRE(dtype == V3D_F16 || dtype == V3D_BF16, "v3d_lora_down: 16-bit dtypes only (got code %d)", dtype);
  V3D_REQUIRE(M >= 1 && M < (1ll << 31), "v3d_lora_down: M=%lld", (long long)M);
  V3D_REQUIRE(R % 16 == 0 && R >= 16, "v3d_lora_down: R=%d must be a multiple of 16", R);
  V3D_REQUIRE(R <= LORA_MAX_R, "v3d_lora_down: R=%d, the kernel covers ranks up to %d", R, LORA_MAX_R);
  V3D_REQUIRE(K >= LORA_BK && K % LORA_BK == 0, "v3d_lora_down: K=%d must be a multiple of %d", K, LORA_BK);
  V3D_REQUIRE(ldx >= K && ldx % 8 == 0 && ldp >= K && ldp % 8 == 0 && ldo >= R && ldo % 8 == 0,
              "v3d_lora_down: row strides must cover their rows and be multiples of 8 (ldx=%lld ldp=%lld ldo=%lld)", (long long)ldx,
              (long long)ldp, (long long)ldo);
  V3D_REQUIRE(aligned16(X) && aligned16(P) && aligned16(out), "v3d_lora_down: pointers must be 16-byte aligned");
  V3D_REQUIRE(lora_span_ok(M, ldx) && lora_span_ok(R, ldp) && lora_span_ok(M, ldo), "v3d_lora_down: an operand spans 2^31 elements or more");
  const dim3 grid((unsigned)((M + LORA_BM - 1) / LORA_BM));
  hipStream_t st = (hipStream_t)stream;
#define V3D_LORA_DOWN(CF)                                                                                                                  \
  hipLaunchKernelGGL((lora_down_kernel<T, CF>), grid, dim3(256), 0, st, (const T*)X, ldx, (const T*)P, ldp, scale, (T*)out, ldo, (int)M, R, K)
  V3D_LORA_16(dtype, {
    if (R <= 64) V3D_LORA_DOWN(1);
    else if (R <= 128) V3D_LORA_DOWN(2);
    else if (R <= 192) V3D_LORA_DOWN(3);
    else if (R <= 256) V3D_LORA_DOWN(4);
    else V3D_LORA_DOWN(6);
  });
#undef V3D_LORA_DOWN
  return check_launch("v3d_lora_down");
}

extern "C" int64_t v3d_lora_wgrad_chunk(int64_t M, int R, int K) {
  if (!lora_shape_ok(M, R, K)) return 0;
  return lora_chunk_rows(M, K);
}

extern "C" int64_t v3d_lora_wgrad_workspace_bytes(int64_t M, int R, int K) {
  if (!lora_shape_ok(M, R, K)) return 0;
  const int64_t want = lora_chunks_wanted(K), most = (M + LORA_BM - 1) / LORA_BM;     // never fewer slabs than the launch uses
  return (want < most ? want : most) * (int64_t)R * K * 4;
}

extern "C" int v3d_lora_wgrad(const void* U, int64_t ldu, const void* X, int64_t ldx, float scale, void* G, int64_t ldg, int g_dtype, int64_t M,
                              int R, int K, int dtype, float* workspace, void* stream) {
  V3D_REQUIRE(U && X && G, "v3d_lora_wgrad: null pointer");
  V3D_REQUIRE(workspace, "v3d_lora_wgrad: null workspace (v3d_lora_wgrad_workspace_bytes(M, R, K) bytes, from the caller)");
  V3D_REQUIRE(dtype == V3D_F16 || dtype == V3D_BF16, "v3d_lora_wgrad: 16-bit operands only (got code %d)", dtype);
  V3D_REQUIRE(g_dtype == V3D_F32 || g_dtype == V3D_F16 || g_dtype == V3D_BF16, "v3d_lora_wgrad: unknown output dtype %d", g_dtype);
  V3D_REQUIRE(M >= 1 && M < (1ll << 31), "v3d_lora_wgrad: M=%lld", (long long)M);
  V3D_REQUIRE(R % 16 == 0 && R >= 16, "v3d_lora_wgrad: R=%d must be a multiple of 16", R);
  V3D_REQUIRE(R <= LORA_MAX_R, "v3d_lora_wgrad: R=%d, the kernel covers ranks up to %d", R, LORA_MAX_R);
  V3D_REQUIRE(K >= LORA_BK && K % LORA_BK == 0, "v3d_lora_wgrad: K=%d must be a multiple of %d", K, LORA_BK);
  V3D_REQUIRE(ldu >= R && ldu % 8 == 0 && ldx >= K && ldx % 8 == 0 && ldg >= K && ldg % 8 == 0,
              "v3d_lora_wgrad: row strides must cover their rows and be multiples of 8 (ldu=%lld ldx=%lld ldg=%lld)", (long long)ldu,
              (long long)ldx, (long long)ldg);
  V3D_REQUIRE(aligned16(U) && aligned16(X) && aligned16(G) && aligned16(workspace), "v3d_lora_wgrad: pointers must be 16-byte aligned");
  V3D_REQUIRE(lora_span_ok(M, ldu) && lora_span_ok(M, ldx) && lora_span_ok(R, ldg), "v3d_lora_wgrad: an operand spans 2^31 elements or more");
  const int64_t chunk = lora_chunk_rows(M, K);
  const int64_t n_chunks = (M + chunk - 1) / chunk;
  V3D_REQUIRE(n_chunks * (int64_t)R * K < (1ll << 31), "v3d_lora_wgrad: the partial slabs span 2^31 elements or more");
  const dim3 grid((unsigned)(K / LORA_BK), (unsigned)n_chunks);
  hipStream_t st = (hipStream_t)stream;
#define V3D_LORA_WGRAD(RB)                                                                                                                 \
  hipLaunchKernelGGL((lora_wgrad_partial_kernel<T, RB>), grid, dim3(256), 0, st, (const T*)U, ldu, (const T*)X, ldx, workspace, (int)M, R, K, \
                     (int)chunk)
  V3D_LORA_16(dtype, {
    if (R <= 64) V3D_LORA_WGRAD(4);
    else if (R <= 128) V3D_LORA_WGRAD(8);
    else if (R <= 192) V3D_LORA_WGRAD(12);
    else if (R <= 256) V3D_LORA_WGRAD(16);
    else V3D_LORA_WGRAD(24);
  });
#undef V3D_LORA_WGRAD
  if (int e = check_launch("v3d_lora_wgrad")) return e;
  const dim3 sgrid((unsigned)(((int64_t)R * (K / 4) + 255) / 256));
  switch (g_dtype) {
    case V3D_F32: hipLaunchKernelGGL(lora_wgrad_sum_kernel<float>, sgrid, dim3(256), 0, st, workspace, (int)n_chunks, scale, (float*)G, ldg, R, K); break;
    case V3D_F16: hipLaunchKernelGGL(lora_wgrad_sum_kernel<f16_t>, sgrid, dim3(256), 0, st, workspace, (int)n_chunks, scale, (f16_t*)G, ldg, R, K); break;
    default: hipLaunchKernelGGL(lora_wgrad_sum_kernel<bf16_t>, sgrid, dim3(256), 0, st, workspace, (int)n_chunks, scale, (bf16_t*)G, ldg, R, K); break;
  }
  return check_launch("v3d_lora_wgrad");
}
