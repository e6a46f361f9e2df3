// The prefill GEMM tile shared by gemm_fp8_kernel (gemm_fp8.hip) and gemm_mxfp4_kernel (gemm_fp4.hip): "q8" = an e4m3 activation
// tile against a weight tile of 8 bits or fewer per element, on v_mfma_scale_f32_16x16x128_f8f6f4.  Device code for the two .hip
// files only (plus their common launch and argument checks); gemm.hip keeps its own copies of the small helpers.
//
// Structure = gemm256x256_kernel (gemm.hip): 256 x 256 tile, K-step 128, 8 waves of 128 x 64, 16-byte LDS-DMA staging into a
// 2-deep ring, four phases of 8 MFMAs with the A fragments of phase p+1 in flight under phase p, B fragments read once per K-step,
// one barrier per K-step, and a wave-private epilogue that turns the C tile around 32 rows at a time.  The activation tile always
// has 128-byte rows with the bf16 kernel's XOR swizzle; what a weight format changes is in its trait (WfE4m3, WfMxfp4) below.
#pragma once
#include "v3d_common.h"

namespace v3d {

using q8_v8i = __attribute__((ext_vector_type(8))) int;
using q8_v4i = __attribute__((ext_vector_type(4))) int;
using q8_f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int Q8_BK = 128;                               // k elements per K-step (= bytes of an activation row)
constexpr int Q8_BN = 256;
constexpr int Q8_ATILE = 256 * Q8_BK;                    // e4m3 activations: 32 KiB
constexpr int Q8_MT = 8;                                 // 16-row m-tiles per wave; the fragment reads hard-code the offsets of 8
constexpr int Q8_WROWS = Q8_MT * 16, Q8_BM = 2 * Q8_WROWS;

enum { Q8_EPI_NONE = 0, Q8_EPI_BIAS = 1, Q8_EPI_RES = 5, Q8_EPI_SWIGLU = 6 };

struct Q8GemmArgs {                                      // a field that a format does not use is null / 0
  const uint8_t* A; const uint8_t* W; const uint8_t* E; const float* sa; const float* sw;
  const void* bias; const void* res; void* out;
  int M, N, K;
  int64_t lda, ldw, lde, ldr, ldo;
  int tiles_m, tiles_n;
};

// Weight formats.  WROW = bytes of a weight row per K-step (CSH = log2 of its 16-byte chunks), BREG = ds_read_b128 per B fragment,
// swz = XOR swizzle of a row's chunks, a_chunk / w_chunk = the h-th 16-byte chunk of the activation / weight fragment of lane
// group g = lane >> 4 (the operand layouts are in the two files' headers), CBSZ = the MFMA's first-operand format.
struct WfE4m3 {                                          // [N, K] bytes + one f32 scale per output column (epilogue)
  static constexpr int WROW = 128, CSH = 3, BREG = 2, CBSZ = 0;
  static constexpr bool COL_SCALE = true, BLOCK_EXP = false;
  static __device__ __forceinline__ int swz(int row) { return (row >> 1) & 7; }
  static __device__ __forceinline__ int a_chunk(int g, int h) { return 2 * g + h; }
  static __device__ __forceinline__ int w_chunk(int g, int h) { return 2 * g + h; }
};
struct WfMxfp4 {                                         // [N, K/2] bytes + one E8M0 byte per 32 k (MFMA scale operand); the 16 rows
  static constexpr int WROW = 64, CSH = 2, BREG = 1, CBSZ = 4;      // that read one chunk together spread over all banks
  static constexpr bool COL_SCALE = false, BLOCK_EXP = true;
  static __device__ __forceinline__ int swz(int row) { return (row >> 2) & 3; }
  static __device__ __forceinline__ int a_chunk(int g, int h) { return g + 4 * h; }
  static __device__ __forceinline__ int w_chunk(int g, int) { return g; }
};
template <class WF> constexpr int q8_lds_bytes = 2 * (Q8_ATILE + 256 * WF::WROW);       // 128 KiB (e4m3), 96 KiB (MXFP4)

__device__ __forceinline__ float q8_silu(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x)); }

__device__ __forceinline__ void q8_glds16(const void* gsrc, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

__device__ __forceinline__ void q8_tile_of_block(int bid, int nblocks, int tiles_m, int tiles_n, int& tm, int& tn) {
  const int q = nblocks >> 3, r = nblocks & 7, xcd = bid & 7;
  const int L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  constexpr int GROUP_M = 8;
  const int per_group = GROUP_M * tiles_n;
  const int g = L / per_group, in_g = L - g * per_group;
  const int first_m = g * GROUP_M;
  const int gsz = (tiles_m - first_m) < GROUP_M ? (tiles_m - first_m) : GROUP_M;
  tm = first_m + in_g % gsz;
  tn = in_g / gsz;
}

// weight row of the [N, K] matrix behind row `row` of the 256-row tile.  SwiGLU (tile columns = two groups of [gate64 | up64]):
// wave column row >> 6 gets the gate columns and the MATCHING up columns of one 32-wide output block, so silu(gate) * up is formed
// in registers (as gemm256pp_kernel).  A macro on purpose: only with the expression in place does the compiler split `row` into
// its wave-uniform and per-lane parts and keep the uniform part in scalar registers (a function costs ~15 vector instructions).
#define Q8_WEIGHT_ROW(EPI, row) \
  ((EPI) == Q8_EPI_SWIGLU ? 128 * ((row) >> 7) + (((row) & 32) ? 64 : 0) + 32 * (((row) >> 6) & 1) + ((row) & 31) : (row))

template <int N>
__device__ __forceinline__ q8_v8i q8_frag(const q8_v4i (&f)[N]) {      // the MFMA's 8-register operand; registers 4..7 of an fp4 one are ignored
  if constexpr (N == 2) return q8_v8i{f[0][0], f[0][1], f[0][2], f[0][3], f[1][0], f[1][1], f[1][2], f[1][3]};
  else return __builtin_shufflevector(f[0], f[0], 0, 1, 2, 3, -1, -1, -1, -1);
}

template <bool COL_SCALE>
__device__ __forceinline__ float q8_deq(float acc, float sa, const float& sw) {
  if constexpr (COL_SCALE) return acc * (sa * sw);
  else return acc * sa;
}

// epilogue: dequantise (sa[m], and sw[n] where the format has column scales - block exponents are already inside the accumulators),
// then as gemm256pp_kernel: each wave turns its 128 x 64 part of the C tile around in a private 8 KiB of LDS, 32 rows at a time - no
// workgroup barrier, whole row segments out; SwiGLU formed in registers first
template <typename T, int EPI, bool COL_SCALE>
__device__ __forceinline__ void q8_epilogue(q8_f32x4 (&acc)[4][Q8_MT], const Q8GemmArgs& p, char* smem, int lane, int wave, int m0, int n0, int tn) {
  const int wm = wave >> 2, wn = wave & 3;
  const T* bias = (const T*)p.bias;
  T* out = (T*)p.out;
  int ln = lane;
  asm volatile("" : "+v"(ln));
  const int l15 = ln & 15, l4 = ln >> 4;
  char* const reg = smem + wave * 8192;
  if constexpr (EPI == Q8_EPI_SWIGLU) {
    constexpr int CP = 80;
    const int rrow = ln >> 2, rch = ln & 3;
    const int gcol = n0 + 128 * (wn >> 1) + 32 * (wn & 1) + 4 * l4;       // + 16 n2 (+ 64 for up): W rows behind acc[n2] / acc[2 + n2]
    float swg[2][4], swu[2][4];
    if constexpr (COL_SCALE) {
#pragma unroll
      for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
        for (int r = 0; r < 4; ++r) { swg[n2][r] = p.sw[gcol + 16 * n2 + r]; swu[n2][r] = p.sw[gcol + 64 + 16 * n2 + r]; }
    }
    T* const obase = out + tn * 128 + (wn >> 1) * 64 + (wn & 1) * 32 + rch * 8;
#pragma unroll
    for (int q = 0; q < Q8_MT / 2; ++q) {
#pragma unroll
      for (int m2 = 0; m2 < 2; ++m2) {
        const int mi = 2 * q + m2;
        int gmc = m0 + wm * Q8_WROWS + 16 * mi + l15;
        gmc = gmc < p.M ? gmc : p.M - 1;
        const float sa = p.sa[gmc];
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2) {
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r)
            v[r] = round_to<T>(q8_silu(round_to<T>(q8_deq<COL_SCALE>(acc[n2][mi][r], sa, swg[n2][r])))) *
                   round_to<T>(q8_deq<COL_SCALE>(acc[2 + n2][mi][r], sa, swu[n2][r]));
          uint2 pk;
          pk.x = pack2<T>(v[0], v[1]); pk.y = pack2<T>(v[2], v[3]);
          *reinterpret_cast<uint2*>(reg + (m2 * 16 + l15) * CP + (16 * n2 + 4 * l4) * 2) = pk;
        }
      }
      uint4 cq[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) cq[j] = *reinterpret_cast<const uint4*>(reg + (rrow + 16 * j) * CP + rch * 16);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int gm = m0 + wm * Q8_WROWS + 32 * q + rrow + 16 * j;
        if (gm < p.M) *reinterpret_cast<uint4*>(obase + (int64_t)gm * p.ldo) = cq[j];
      }
    }
  } else {
    constexpr int CP = 144;
    const int rrow = ln >> 3, rch = ln & 7;
    const int colr = n0 + wn * 64 + rch * 8;
    float swv[4][4], bv[4][4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = n0 + wn * 64 + 16 * ni + 4 * l4 + r;
        if constexpr (COL_SCALE) swv[ni][r] = p.sw[c];
        bv[ni][r] = bias != nullptr ? to_f32(bias[c]) : 0.f;
      }
#pragma unroll
    for (int q = 0; q < Q8_MT / 2; ++q) {
      uint4 rr[4];
      if constexpr (EPI == Q8_EPI_RES) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          int gc = m0 + wm * Q8_WROWS + 32 * q + rrow + 8 * j;
          gc = gc < p.M ? gc : p.M - 1;
          rr[j] = *reinterpret_cast<const uint4*>((const T*)p.res + (int64_t)gc * p.ldr + colr);
        }
      }
#pragma unroll
      for (int m2 = 0; m2 < 2; ++m2) {
        const int mi = 2 * q + m2;
        int gmc = m0 + wm * Q8_WROWS + 16 * mi + l15;
        gmc = gmc < p.M ? gmc : p.M - 1;
        const float sa = p.sa[gmc];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = q8_deq<COL_SCALE>(acc[ni][mi][r], sa, swv[ni][r]) + bv[ni][r];
          uint2 pk;
          pk.x = pack2<T>(v[0], v[1]); pk.y = pack2<T>(v[2], v[3]);
          *reinterpret_cast<uint2*>(reg + (m2 * 16 + l15) * CP + (16 * ni + 4 * l4) * 2) = pk;
        }
      }
      uint4 cq[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) cq[j] = *reinterpret_cast<const uint4*>(reg + (rrow + 8 * j) * CP + rch * 16);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint4 c = cq[j];
        const int gm = m0 + wm * Q8_WROWS + 32 * q + rrow + 8 * j;
        if constexpr (EPI == Q8_EPI_RES) {
          float v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = vec_get<T>(c, e) + vec_get<T>(rr[j], e);
          c = vec_pack<T>(v);
        }
        if (gm < p.M) *reinterpret_cast<uint4*>(out + (int64_t)gm * p.ldo + colr) = c;
      }
    }
  }
}

// One 256 x 256 output tile: the whole body of both __global__ entry points.
template <typename T, int EPI, class WF>
__device__ __forceinline__ void q8_gemm_tile(const Q8GemmArgs& p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int MG = Q8_MT / 4;                          // m-tiles per phase (4 phases)
  constexpr int APW = Q8_BM / 8 / 8;                     // activation DMAs per wave (8 rows x 8 chunks each)
  constexpr int WRD = 64 >> WF::CSH, WPW = 32 / WRD;     // rows per weight DMA, weight DMAs per wave (32 rows)
  constexpr int STAGE = Q8_ATILE + 256 * WF::WROW;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  int tm, tn;
  q8_tile_of_block(blockIdx.x, gridDim.x, p.tiles_m, p.tiles_n, tm, tn);
  const int m0 = tm * Q8_BM, n0 = tn * Q8_BN;

  unsigned a_off[APW], w_off[WPW];
#pragma unroll
  for (int i = 0; i < APW; ++i) {
    const int row = wave * (APW * 8) + i * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ ((row >> 1) & 7);
    int gm = m0 + row;
    gm = gm < p.M ? gm : p.M - 1;
    a_off[i] = (unsigned)(gm * (int)p.lda + chunk * 16);
  }
#pragma unroll
  for (int i = 0; i < WPW; ++i) {
    const int row = wave * 32 + i * WRD + (lane >> WF::CSH);
    const int chunk = (lane & ((1 << WF::CSH) - 1)) ^ WF::swz(row);
    w_off[i] = (unsigned)((n0 + Q8_WEIGHT_ROW(EPI, row)) * (int)p.ldw + chunk * 16);
  }
  auto stage = [&](int buf, int kt) {
    char* ba = smem + buf * STAGE + (wave * APW * 8) * Q8_BK;
    char* bw = smem + buf * STAGE + Q8_ATILE + (wave * 32) * WF::WROW;
    const char* Ak = (const char*)p.A + (size_t)kt * Q8_BK;
    const char* Wk = (const char*)p.W + (size_t)kt * WF::WROW;
#pragma unroll
    for (int i = 0; i < APW; ++i) q8_glds16(Ak + a_off[i], ba + i * 8 * Q8_BK);
#pragma unroll
    for (int i = 0; i < WPW; ++i) q8_glds16(Wk + w_off[i], bw + i * WRD * WF::WROW);
  };

  // fragments: lane l reads row l & 15 of a 16-row tile, chunks a_chunk / w_chunk of its lane group, XOR-swizzled as staged
  const int l15 = lane & 15, g4 = lane >> 4;
  const int frow = l15 * Q8_BK, sw = (lane >> 1) & 7;
  const unsigned fo_lo = frow + ((WF::a_chunk(g4, 0) ^ sw) << 4), fo_hi = frow + ((WF::a_chunk(g4, 1) ^ sw) << 4);
  const unsigned fw_lo = l15 * WF::WROW + ((WF::w_chunk(g4, 0) ^ WF::swz(l15)) << 4);
  const unsigned fw_hi = l15 * WF::WROW + ((WF::w_chunk(g4, 1) ^ WF::swz(l15)) << 4);
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const unsigned offA = lds0 + (wm * Q8_WROWS) * Q8_BK, offW = lds0 + Q8_ATILE + (wn * 64) * WF::WROW;

  // block exponents: the lane's E8M0 byte of n-tile ni at K-step kt is e[weight row][4 kt + g]; 127 = 2^0 without them
  const uint8_t* eptr[4];
  int sc[4] = {127, 127, 127, 127}, scn[4];
  if constexpr (WF::BLOCK_EXP) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) eptr[ni] = p.E + (int64_t)(n0 + Q8_WEIGHT_ROW(EPI, wn * 64 + 16 * ni + l15)) * p.lde + g4;
  }

  q8_f32x4 acc[4][Q8_MT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < Q8_MT; ++j) acc[i][j] = q8_f32x4{0.f, 0.f, 0.f, 0.f};

  // register sets: B fragments of the K-step (4 n-tiles), A ring of two groups of MG m-tiles; an A fragment = lo|hi v4i (two
  // ds_read_b128; the 8-register MFMA operand is assembled by the compiler), a B fragment = BREG of them.  One barrier per K-step:
  //   top: read B + A(0,1), issue the DMA of tile t+1 into the other buffer, then four phases of 8 MFMAs with
  //   the A fragments of phase p+1 in flight under phase p; the last phase also retires the DMA (vmcnt(0)).
  q8_v4i A0[MG][2], A1[MG][2], B0[4][WF::BREG];
#define Q8_DSR(dst, addr, imm) asm volatile("ds_read_b128 %0, %1 offset:" #imm : "=v"(dst) : "v"(addr))
#define Q8_RDT(f, lo, hi, imm) { Q8_DSR(f[0], lo, imm); Q8_DSR(f[1], hi, imm); }
#define Q8_RD_A(F, lo, hi, tile0)                                                                                 \
  {                                                                                                               \
    if constexpr ((tile0) == 0) { Q8_RDT(F[0], lo, hi, 0); Q8_RDT(F[1], lo, hi, 2048); }                          \
    else if constexpr ((tile0) == 2) { Q8_RDT(F[0], lo, hi, 4096); Q8_RDT(F[1], lo, hi, 6144); }                  \
    else if constexpr ((tile0) == 4) { Q8_RDT(F[0], lo, hi, 8192); Q8_RDT(F[1], lo, hi, 10240); }                 \
    else { Q8_RDT(F[0], lo, hi, 12288); Q8_RDT(F[1], lo, hi, 14336); }                                            \
  }
#define Q8_RD_B(F, lo, hi)                                                                                                       \
  {                                                                                                                              \
    if constexpr (WF::BREG == 2) { Q8_RDT(F[0], lo, hi, 0); Q8_RDT(F[1], lo, hi, 2048); Q8_RDT(F[2], lo, hi, 4096); Q8_RDT(F[3], lo, hi, 6144); } \
    else { Q8_DSR(F[0][0], lo, 0); Q8_DSR(F[1][0], lo, 1024); Q8_DSR(F[2][0], lo, 2048); Q8_DSR(F[3][0], lo, 3072); }              \
  }
#define Q8_WA(cnt, F) asm volatile("s_waitcnt " cnt : "+v"(F[0][0]), "+v"(F[0][1]), "+v"(F[1][0]), "+v"(F[1][1]) : : "memory")
#define Q8_WAB(cnt, F, G)                                                                                                        \
  {                                                                                                                              \
    if constexpr (WF::BREG == 2)                                                                                                 \
      asm volatile("s_waitcnt " cnt : "+v"(F[0][0]), "+v"(F[0][1]), "+v"(F[1][0]), "+v"(F[1][1]), "+v"(G[0][0]), "+v"(G[0][1]),  \
                   "+v"(G[1][0]), "+v"(G[1][1]), "+v"(G[2][0]), "+v"(G[2][1]), "+v"(G[3][0]), "+v"(G[3][1]) : : "memory");       \
    else                                                                                                                         \
      asm volatile("s_waitcnt " cnt : "+v"(F[0][0]), "+v"(F[0][1]), "+v"(F[1][0]), "+v"(F[1][1]), "+v"(G[0][0]), "+v"(G[1][0]),  \
                   "+v"(G[2][0]), "+v"(G[3][0]) : : "memory");                                                                   \
  }
#define Q8_MMA(FA, FB, tile0)                                                                                       \
  {                                                                                                                 \
    __builtin_amdgcn_s_setprio(1);                                                                                  \
    _Pragma("unroll") for (int i = 0; i < MG; ++i)                                                                  \
    _Pragma("unroll") for (int ni = 0; ni < 4; ++ni)                                                                \
        acc[ni][(tile0) + i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(q8_frag(FB[ni]), q8_frag(FA[i]),    \
                                                                                  acc[ni][(tile0) + i], WF::CBSZ, 0, 0, sc[ni], 0, 127); \
    __builtin_amdgcn_s_setprio(0);                                                                                  \
  }

  const int nt = p.K / Q8_BK;
  stage(0, 0);
  if constexpr (WF::BLOCK_EXP) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) sc[ni] = eptr[ni][0];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    const unsigned alo = offA + cur * STAGE + fo_lo, ahi = offA + cur * STAGE + fo_hi;
    const unsigned wlo = offW + cur * STAGE + fw_lo, whi = offW + cur * STAGE + fw_hi;
    Q8_RD_B(B0, wlo, whi);
    Q8_RD_A(A0, alo, ahi, 0);
    if (t + 1 < nt) {                                // buffer cur^1 was released by the barrier that ended step t-1
      stage(cur ^ 1, t + 1);
      if constexpr (WF::BLOCK_EXP) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) scn[ni] = eptr[ni][4 * (t + 1)];
      }
    }
    Q8_RD_A(A1, alo, ahi, 2);
    Q8_WAB("lgkmcnt(4)", A0, B0);
    Q8_MMA(A0, B0, 0);
    Q8_RD_A(A0, alo, ahi, 4);
    Q8_WA("lgkmcnt(4)", A1);
    Q8_MMA(A1, B0, 2);
    Q8_RD_A(A1, alo, ahi, 6);
    Q8_WA("lgkmcnt(4)", A0);
    Q8_MMA(A0, B0, 4);
    Q8_WA("vmcnt(0) lgkmcnt(0)", A1);               // last fragments + this wave's share of tile t+1 (and its exponents)
    Q8_MMA(A1, B0, 6);
    if constexpr (WF::BLOCK_EXP) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) sc[ni] = scn[ni];
    }
    __builtin_amdgcn_s_barrier();                    // tile t fully read by everyone, tile t+1 visible
  }
  __syncthreads();
  q8_epilogue<T, EPI, WF::COL_SCALE>(acc, p, smem, lane, wave, m0, n0, tn);
#undef Q8_DSR
#undef Q8_RDT
#undef Q8_RD_A
#undef Q8_RD_B
#undef Q8_WA
#undef Q8_WAB
#undef Q8_MMA
#undef Q8_WEIGHT_ROW
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// the argument checks common to v3d_gemm_fp8 and v3d_gemm_mxfp4; fmt_ptrs / fmt_lds = the format's own pointer and leading-dimension
// conditions, which fail under the same messages
static int q8_validate(const char* who, const Q8GemmArgs& p, bool fmt_ptrs, bool fmt_lds, int out_dtype, int epilogue) {
  V3D_REQUIRE(p.A && p.W && fmt_ptrs && p.sa && p.out, "%s: null pointer", who);
  V3D_REQUIRE(out_dtype == V3D_F16 || out_dtype == V3D_BF16, "%s: output dtype must be f16 or bf16", who);
  V3D_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0 && p.N % Q8_BN == 0 && p.K % Q8_BK == 0, "%s: N=%d must be a multiple of 256 and K=%d of 128", who, p.N, p.K);
  V3D_REQUIRE(p.lda >= p.K && fmt_lds && p.lda % 16 == 0 && p.ldw % 16 == 0 && p.ldo % 8 == 0, "%s: leading dimensions", who);
  V3D_REQUIRE(aligned16(p.A) && aligned16(p.W) && aligned16(p.out), "%s: pointers must be 16-byte aligned", who);
  V3D_REQUIRE((int64_t)p.M * p.lda < (1ll << 31) && (int64_t)p.N * p.ldw < (1ll << 31), "%s: operand larger than 2 GiB", who);
  V3D_REQUIRE(epilogue != Q8_EPI_BIAS || p.bias, "%s: bias epilogue without bias", who);
  V3D_REQUIRE(epilogue != Q8_EPI_RES || (p.res && aligned16(p.res) && p.ldr % 8 == 0), "%s: residual epilogue without residual", who);
  return V3D_OK;
}

// NONE, BIAS, RES, SWIGLU = the four instantiations of one entry point for one output type
template <int LDS, void (*NONE)(Q8GemmArgs), void (*BIAS)(Q8GemmArgs), void (*RES)(Q8GemmArgs), void (*SWIGLU)(Q8GemmArgs)>
static int q8_launch(Q8GemmArgs p, int epi, const char* who, hipStream_t st) {
  p.tiles_m = (p.M + Q8_BM - 1) / Q8_BM;
  p.tiles_n = p.N / Q8_BN;
  p.bias = epi == Q8_EPI_BIAS ? p.bias : nullptr;
  p.res = epi == Q8_EPI_RES ? p.res : nullptr;
  switch (epi) {
    case Q8_EPI_NONE: return launch_big_lds<NONE, LDS, 512>(p, p.tiles_m * p.tiles_n, who, st);
    case Q8_EPI_BIAS: return launch_big_lds<BIAS, LDS, 512>(p, p.tiles_m * p.tiles_n, who, st);
    case Q8_EPI_RES: return launch_big_lds<RES, LDS, 512>(p, p.tiles_m * p.tiles_n, who, st);
    case Q8_EPI_SWIGLU: return launch_big_lds<SWIGLU, LDS, 512>(p, p.tiles_m * p.tiles_n, who, st);
    default: set_error("%s: epilogue %d unsupported (NONE, BIAS, RES, SWIGLU)", who, epi); return V3D_E_INVALID;
  }
}

}  // namespace v3d
