// 3-D sinusoidal position encoding and the fused visual-token kernel (K5-K9).
//
//   v3d_sin3d_table_build : PositionEmbeddingSine3D for every integer voxel id, once per model
//   v3d_visual_tokens     : bilinear 27x27->14x14 pool + PE(voxel id) add + newline insertion,
//                           one HBM pass over the projector output  (the north-star kernel)
//   v3d_embed_gather      : text-token embedding rows
// (v3d_sin3d_pe, the same module for arbitrary coordinates, sits with its P-point form in pe_points.hip.)
//
// All of it is HBM-bound streaming: 16-byte loads/stores per lane, no LDS, no MFMA.
// Compiled with -ffp-contract=off; the rounding contract and the token-row body are in visual_common.h.
#include "visual_common.h"

namespace v3d {

template <typename T>
__global__ __launch_bounds__(256) void sin3d_table_kernel(const float* __restrict__ dim_t, int nf, int n_ids,
                                                          int row_elems, T* __restrict__ table,
                                                          float* __restrict__ table_f32) {
  constexpr int VEC = 16 / sizeof(T);
  const int64_t total = (int64_t)n_ids * nf;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int id = (int)(i / nf), j = (int)(i - (int64_t)id * nf);
    const float val = pe_value((float)id, dim_t[j], j);
    if (table_f32) table_f32[i] = val;
    if (table) {
      const T t = from_f32<T>(val);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int shift = (a * nf) % VEC;
        table[((size_t)a * n_ids + id) * row_elems + shift + j] = t;
      }
    }
  }
}

// ----------------------------------------------------------------------------------------
// Fused visual-token kernel: token_row_body (visual_common.h) with the PE operand read from the per-axis table,
//   PE     : x = T(x + table[axis][id][channel])
// The three voxel ids of the token are workgroup-uniform: they and the table rows they select live in SGPRs.  Beside feat and
// out the kernel reads one table row per axis (L2-resident: 3 x n_ids x ~2.4 KB).
// ----------------------------------------------------------------------------------------
template <typename T, bool PE>
struct AxisTablePE {
  static constexpr bool ON = PE;
  static constexpr int VEC = 16 / sizeof(T);
  const int32_t* ids;
  const T* table;
  int n_ids, row_elems, nf;
  const uint4* trow_[3];      // the token's table row per axis
  int tbase_[3];              // first vector of the token row that overlaps axis a
  uint4 p;                    // the lane's operand: its table vector(s), OR-ed

  __device__ __forceinline__ void token(size_t cell) {
    const int32_t* id3 = ids + cell * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      int id = id3[a];
      id = id < 0 ? 0 : (id >= n_ids ? n_ids - 1 : id);   // ids come from the clamped voxeliser; stay in bounds regardless
      trow_[a] = reinterpret_cast<const uint4*>(table + ((size_t)a * n_ids + id) * row_elems);
      tbase_[a] = (a * nf) / VEC;
    }
  }
  __device__ __forceinline__ void vector(int) {}
  __device__ __forceinline__ void operand(int k) {
    // the members are read into locals first, so that a lane's axis selects among VALUES held in SGPRs (a select among the
    // members' addresses would put the struct in memory): one load from the selected row
    const uint4* const trow[3] = {trow_[0], trow_[1], trow_[2]};
    const int tbase[3] = {tbase_[0], tbase_[1], tbase_[2]};
    const int c0 = k * VEC;
    const int a0 = c0 / nf, a1 = (c0 + VEC - 1) / nf;
    p = make_uint4(0, 0, 0, 0);
    if (a0 < 3) {
      p = trow[a0 == 0 ? 0 : (a0 == 1 ? 1 : 2)][k - tbase[a0 == 0 ? 0 : (a0 == 1 ? 1 : 2)]];
      if (a1 != a0 && a1 < 3) {
        const uint4 q = trow[a1 == 1 ? 1 : 2][k - tbase[a1 == 1 ? 1 : 2]];
        p.x |= q.x; p.y |= q.y; p.z |= q.z; p.w |= q.w;   // disjoint support: padding is zero bits
      }
    }
  }
  __device__ __forceinline__ float value(int j) const { return vec_get<T>(p, j); }
};

template <typename T, bool POOL, bool PE>
__global__ __launch_bounds__(512) void visual_tokens_kernel(const T* __restrict__ feat, const int32_t* __restrict__ ids,
                                                            const T* __restrict__ table, int n_ids, int row_elems,
                                                            const T* __restrict__ newline, T* __restrict__ out,
                                                            int64_t out_stride, int side, int n, int C, int newline_on) {
  AxisTablePE<T, PE> src;
  src.ids = ids; src.table = table; src.n_ids = n_ids; src.row_elems = row_elems; src.nf = C / 3;
  token_row_body<T, POOL>(feat, newline, out, out_stride, side, n, C, newline_on, src);
}

template <typename T>
__global__ __launch_bounds__(256) void embed_gather_kernel(const T* __restrict__ table, int64_t vocab, int C,
                                                           const int64_t* __restrict__ ids, T* __restrict__ out,
                                                           int64_t out_stride) {
  constexpr int VEC = 16 / sizeof(T);
  const int64_t row = blockIdx.x;
  int64_t id = ids[row];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const uint4* src = reinterpret_cast<const uint4*>(table + id * C);
  uint4* dst = reinterpret_cast<uint4*>(out + row * out_stride);
  for (int k = threadIdx.x; k < C / VEC; k += blockDim.x) dst[k] = src[k];
}

}  // namespace v3d

using namespace v3d;

extern "C" int64_t v3d_sin3d_table_row_elems(int embedding_size, int dtype) {
  const int vec = dtype == V3D_F32 ? 4 : 8;
  return table_row_elems(embedding_size / 3, vec);
}

extern "C" int v3d_sin3d_table_build(const float* dim_t, int embedding_size, int n_ids, int dtype, void* table,
                                     float* table_f32, void* stream) {
  V3D_REQUIRE(dim_t && (table || table_f32), "v3d_sin3d_table_build: null pointer");
  V3D_REQUIRE(embedding_size >= 3 && n_ids > 0, "v3d_sin3d_table_build: bad shape E=%d n_ids=%d", embedding_size, n_ids);
  const int nf = embedding_size / 3;
  hipStream_t st = (hipStream_t)stream;
  const int row = (int)v3d_sin3d_table_row_elems(embedding_size, dtype);
  if (table) {
    const size_t esz = dtype == V3D_F32 ? 4 : 2;
    hipError_t e = hipMemsetAsync(table, 0, (size_t)3 * n_ids * row * esz, st);
    if (e != hipSuccess) { set_error("v3d_sin3d_table_build: memset: %s", hipGetErrorString(e)); return V3D_E_LAUNCH; }
  }
  int64_t blocks = ((int64_t)n_ids * nf + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  V3D_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(sin3d_table_kernel<T>, dim3((int)blocks), dim3(256), 0, st, dim_t, nf,
                                               n_ids, row, (T*)table, table_f32));
  return check_launch("v3d_sin3d_table_build");
}

extern "C" int v3d_visual_tokens(const void* feat, const int32_t* ids, const void* table, int n_ids,
                                 const void* newline, void* out, int64_t out_stride, int dtype, int V, int side, int n,
                                 int C, int flags, void* stream) {
  const bool pool = flags & V3D_VT_POOL, pe = flags & V3D_VT_PE, nl = flags & V3D_VT_NEWLINE;
  V3D_REQUIRE(!pe || (ids && table && n_ids > 0), "v3d_visual_tokens: PE needs ids and a table");
  const int vec = dtype == V3D_F32 ? 4 : 8;
  TokenRowPlan plan;
  if (int e = plan_token_rows("v3d_visual_tokens", feat, pe ? table : nullptr, newline, out, out_stride, vec, V, side, n, C, flags, &plan)) return e;
  V3D_REQUIRE(!pe || C / 3 >= vec, "v3d_visual_tokens: C=%d too narrow for the table layout", C);
  const int row = (int)v3d_sin3d_table_row_elems(C, dtype);
  hipStream_t st = (hipStream_t)stream;
#define V3D_VT_LAUNCH(P, E)                                                                                                   \
  hipLaunchKernelGGL((visual_tokens_kernel<T, P, E>), dim3((unsigned)plan.tokens), dim3(plan.threads), 0, st, (const T*)feat, \
                     ids, (const T*)table, n_ids, row, (const T*)newline, (T*)out, out_stride, side, n, C, nl ? 1 : 0)
  V3D_DISPATCH_DTYPE(dtype, {
    if (pool && pe) V3D_VT_LAUNCH(true, true);
    else if (pool) V3D_VT_LAUNCH(true, false);
    else if (pe) V3D_VT_LAUNCH(false, true);
    else V3D_VT_LAUNCH(false, false);
  });
#undef V3D_VT_LAUNCH
  return check_launch("v3d_visual_tokens");
}

extern "C" int v3d_embed_gather(const void* table, int64_t vocab, int C, const int64_t* ids, int64_t n, void* out,
                                int64_t out_stride, int dtype, void* stream) {
  V3D_REQUIRE(table && ids && out, "v3d_embed_gather: null pointer");
  V3D_REQUIRE(vocab > 0 && C > 0 && n >= 0, "v3d_embed_gather: bad shape");
  if (n == 0) return V3D_OK;
  const int vec = dtype == V3D_F32 ? 4 : 8;
  V3D_REQUIRE(C % vec == 0 && out_stride % vec == 0 && out_stride >= C, "v3d_embed_gather: C/out_stride not a multiple of %d", vec);
  V3D_REQUIRE(aligned16(table) && aligned16(out), "v3d_embed_gather: pointers must be 16-byte aligned");
  V3D_REQUIRE(n < (1ll << 31), "v3d_embed_gather: too many rows");
  V3D_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(embed_gather_kernel<T>, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream,
                                               (const T*)table, vocab, C, ids, (T*)out, out_stride));
  return check_launch("v3d_embed_gather");
}
