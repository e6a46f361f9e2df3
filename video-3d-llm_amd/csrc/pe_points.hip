// The position path's other encodings: P points per patch instead of the patch mean.
//
//   v3d_coord_points_voxel       : sample9 / sample5 / sample1 (a gather) and minmax (a 27x27 reduction) + voxel ids
//   v3d_sin3d_table_build_points : PositionEmbeddingSine3D(n_points=P) for every integer voxel id
//   v3d_sin3d_pe_points          : the same module for arbitrary coordinates, xyz [N,P,3] -> [N,E]
//   v3d_visual_tokens_points     : bilinear pool + PE(P points; table or on-the-fly trig) add + newline rows
//
// The one-point "avg-discrete-sin3d" path has its own aggregation and fused kernel (geometry.hip, visual_tokens.hip); the voxeliser,
// pe_value and the token-row body are shared with them (visual_common.h).  Compiled with -ffp-contract=off like visual_tokens.hip.
#include "visual_common.h"

namespace v3d {

constexpr int kSide = 384, kPatch = 27, kCells = 14;     // llava_arch.py:245 hard-codes 14 x 27

__host__ __device__ inline int points_of_mode(int mode) {
  return mode == V3D_PTS_SAMPLE9 ? 9 : mode == V3D_PTS_SAMPLE5 ? 5 : mode == V3D_PTS_SAMPLE1 ? 1 : mode == V3D_PTS_MINMAX ? 2 : 0;
}

template <typename T>
__device__ __forceinline__ void store_point(float x, int ch, size_t o, const Range& rg, T* pts, T* vox, int32_t* ids) {
  if (pts) pts[o] = from_f32<T>(x);
  if (vox || ids) {
    const float r = voxelise<T>(x, round_to<T>(rg.lo[ch]), round_to<T>(rg.hi[ch]), rg.voxel);
    if (vox) vox[o] = from_f32<T>(r);
    if (ids) ids[o] = (int32_t)r;
  }
}

// ----------------------------------------------------------------------------------------
// sample_n_points (llava_arch.py:241-257): pixel (27*py + 4 + 9*ri, 27*px + 4 + 9*ci) of every patch, point
// index 3*ri + ci; sample5 keeps points 0,2,4,6,8, sample1 point 4.  One lane = one output element: the frame
// itself is never streamed.
// ----------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void coord_sample_kernel(const T* __restrict__ coords, int64_t total, int P, int mode,
                                                           Range rg, T* __restrict__ pts, T* __restrict__ vox,
                                                           int32_t* __restrict__ ids) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % 3);
    int64_t r = i / 3;
    const int k = (int)(r % P);
    r /= P;
    const int px = (int)(r % kCells);
    r /= kCells;
    const int py = (int)(r % kCells);
    const int64_t v = r / kCells;
    const int point = mode == V3D_PTS_SAMPLE9 ? k : (mode == V3D_PTS_SAMPLE5 ? 2 * k : 4);
    const int row = kPatch * py + 4 + 9 * (point / 3), col = kPatch * px + 4 + 9 * (point % 3);
    const float x = to_f32(coords[((v * kSide + row) * kSide + col) * 3 + ch]);
    store_point<T>(x, ch, (size_t)i, rg, pts, vox, ids);
  }
}

// ----------------------------------------------------------------------------------------
// minmax_coordinate_in_patch (llava_arch.py:225-239): point 0 = -max_pool2d(-x), point 1 = max_pool2d(x) over each
// 27x27 patch.  A NaN in the window gives NaN (ATen's max-pool keeps it); min and max of finite values are exact in
// every dtype.  One workgroup = one (frame, patch-row) strip of 27 image rows: lane i owns 16-byte column i of every
// row (coalesced, each byte of the strip read once), folds its 27 vectors in registers, leaves per-column results
// in LDS, and lanes 0..41 fold the 27 columns of their (patch, channel).
// ----------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(320) void coord_minmax_kernel(const T* __restrict__ coords, Range rg, T* __restrict__ pts,
                                                           T* __restrict__ vox, int32_t* __restrict__ ids) {
  constexpr int VEC = 16 / sizeof(T);
  constexpr int ROW = kSide * 3;             // 1152 elements; the 6 dropped columns ride along and are never folded
  constexpr int VECS = ROW / VEC;
  __shared__ float smin[ROW], smax[ROW];
  const int v = blockIdx.y, py = blockIdx.x, tid = threadIdx.x;
  const uint4* strip = reinterpret_cast<const uint4*>(coords + ((size_t)v * kSide + (size_t)py * kPatch) * ROW);
  const float nan = __uint_as_float(0x7fc00000u);

  for (int i = tid; i < VECS; i += blockDim.x) {
    float mn[VEC], mx[VEC];
    bool bad[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { mn[j] = __uint_as_float(0x7f800000u); mx[j] = __uint_as_float(0xff800000u); bad[j] = false; }
#pragma unroll 9
    for (int r = 0; r < kPatch; ++r) {
      const uint4 raw = strip[(size_t)r * VECS + i];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float x = vec_get<T>(raw, j);
        bad[j] = bad[j] || (x != x);
        mn[j] = fminf(mn[j], x);        // fminf / fmaxf return the other operand for a NaN; `bad` carries it
        mx[j] = fmaxf(mx[j], x);
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      smin[i * VEC + j] = bad[j] ? nan : mn[j];
      smax[i * VEC + j] = bad[j] ? nan : mx[j];
    }
  }
  __syncthreads();
  if (tid < kCells * 3) {
    const int px = tid / 3, ch = tid - px * 3;
    float mn = __uint_as_float(0x7f800000u), mx = __uint_as_float(0xff800000u);
    bool bad = false;
    for (int iw = 0; iw < kPatch; ++iw) {
      const float a = smin[(px * kPatch + iw) * 3 + ch], b = smax[(px * kPatch + iw) * 3 + ch];
      bad = bad || (a != a);
      mn = fminf(mn, a);
      mx = fmaxf(mx, b);
    }
    const size_t o = ((((size_t)v * kCells + py) * kCells + px) * 2) * 3 + ch;
    store_point<T>(bad ? nan : mn, ch, o, rg, pts, vox, ids);
    store_point<T>(bad ? nan : mx, ch, o + 3, rg, pts, vox, ids);
  }
}

// ----------------------------------------------------------------------------------------
// PE with P points (position_encoding.py:17-49): nf = E / (3P); channel c < 3*P*nf belongs to segment q = c / nf
// (point q / 3, axis q % 3) and feature j = c % nf; channels past 3*P*nf are zero.
//
// Table layout.  The fused kernel reads 16-byte vectors of channels, and a segment starts at channel q*nf, which is
// (q*nf) % VEC elements past a vector boundary.  One copy of the [n_ids, nf] table per DISTINCT shift (at most VEC
// copies), each row holding the nf values at its shift with zero bits around them: a lane's vector is then one
// aligned load per segment it overlaps (at most two, since nf >= VEC), OR-ed together.
// ----------------------------------------------------------------------------------------
struct PointsLayout {
  int n_copies;
  int row_elems;
  uint32_t shift_of_copy;     // 4 bits per copy
  uint32_t copy_of_shift;     // 4 bits per shift
};

__host__ inline PointsLayout points_layout(int nf, int P, int vec) {
  PointsLayout l = {0, table_row_elems(nf, vec), 0u, 0u};
  bool seen[8] = {false, false, false, false, false, false, false, false};
  for (int q = 0; q < 3 * P; ++q) {
    const int s = (int)(((int64_t)q * nf) % vec);
    if (seen[s]) continue;
    seen[s] = true;
    l.shift_of_copy |= (uint32_t)s << (4 * l.n_copies);
    l.copy_of_shift |= (uint32_t)l.n_copies << (4 * s);
    ++l.n_copies;
  }
  return l;
}

template <typename T>
__global__ __launch_bounds__(256) void sin3d_table_points_kernel(const float* __restrict__ dim_t, int nf, int n_ids,
                                                                 PointsLayout lay, T* __restrict__ table) {
  const int64_t total = (int64_t)n_ids * nf;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int id = (int)(i / nf), j = (int)(i - (int64_t)id * nf);
    const T t = from_f32<T>(pe_value((float)id, dim_t[j], j));
    for (int c = 0; c < lay.n_copies; ++c) {
      const int shift = (int)((lay.shift_of_copy >> (4 * c)) & 15u);
      table[((size_t)c * n_ids + id) * lay.row_elems + shift + j] = t;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void sin3d_pe_points_kernel(const T* __restrict__ xyz, int64_t N, int P,
                                                              const float* __restrict__ dim_t, int E, int nf,
                                                              T* __restrict__ out) {
  const int64_t total = N * E;
  const int segs = 3 * P;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t tok = i / E;
    const int c = (int)(i - tok * E);
    const int q = c / nf;
    float val = 0.0f;
    if (q < segs) {
      const int j = c - q * nf;
      val = pe_value(to_f32(xyz[tok * segs + q]), dim_t[j], j);
    }
    out[i] = from_f32<T>(val);
  }
}

// ----------------------------------------------------------------------------------------
// The fused visual-token kernel with P points: token_row_body (visual_common.h) with this PE operand of a lane:
//
//   table : segments q0, q1 of the lane's first and last channel, id = ids[token][q] (4-byte loads from the token's
//           12*P bytes, which every lane of the workgroup shares), one aligned 16-byte load from id0's row of the
//           copy with q0's shift; a second one when the vector runs into segment q1 = q0 + 1
//   CONT  : x = pts[token][q] per channel, T(pe_value(x, dim_t[j], j)) on the fly (the reference's rule for a
//           type without `discrete`; also `avg-sin3d` with P = 1)
// ----------------------------------------------------------------------------------------
template <typename T>
struct PointsArgs {
  const T* feat;
  const int32_t* ids;       // [V, n*n, P, 3]  (table source)
  const T* pts;             // [V, n*n, P, 3]  (CONT source)
  const T* table;           // [n_copies][n_ids][row_elems]
  const float* dim_t;       // [nf]            (CONT source)
  const T* newline;
  T* out;
  int64_t out_stride;
  PointsLayout lay;
  int n_ids, P, nf, side, n, C, newline_on;
};

// the 16-byte vector k of the token row as segment q's table row holds it (zero bits outside q's channels)
template <typename T>
__device__ __forceinline__ uint4 points_table_vec(const PointsArgs<T>& a, int id, int q, int k) {
  constexpr int VEC = 16 / sizeof(T);
  id = id < 0 ? 0 : (id >= a.n_ids ? a.n_ids - 1 : id);     // ids come from the clamped voxeliser; stay in bounds regardless
  const int start = q * a.nf;
  const int copy = (int)((a.lay.copy_of_shift >> (4 * (start % VEC))) & 15u);
  const uint4* row = reinterpret_cast<const uint4*>(a.table + ((size_t)copy * a.n_ids + id) * a.lay.row_elems);
  return row[k - start / VEC];
}

template <typename T, bool CONT>
struct PointsPE {
  static constexpr bool ON = true;
  static constexpr int VEC = 16 / sizeof(T);
  const PointsArgs<T>& a;
  size_t tbase;             // this token's ids / points
  int id0, id1;
  uint4 p;                  // table source: the lane's table vector(s), OR-ed
  int c0, q0, edge;         // CONT source: first channel and segment of the lane's vector, channels of it that belong to q0,
  float xa, xb;             //              and the coordinates of segments q0 and q0 + 1

  __device__ __forceinline__ void token(size_t cell) { tbase = cell * (3 * a.P); }
  __device__ __forceinline__ void vector(int k) {
    const int segs = 3 * a.P, c0 = k * VEC;
    const int q0 = c0 / a.nf, q1 = (c0 + VEC - 1) / a.nf;
    // The lane's ids are asked for BEFORE the feature rows: vector loads return in order, so a table load that waits for its id
    // would otherwise wait for the four feature loads as well, and the kernel's longest chain would grow by one memory round trip.
    id0 = id1 = 0;
    if (!CONT) {
      id0 = a.ids[tbase + (q0 < segs ? q0 : segs - 1)];
      id1 = a.ids[tbase + (q1 < segs ? q1 : segs - 1)];
    }
  }
  __device__ __forceinline__ void operand(int k) {
    const int segs = 3 * a.P, nf = a.nf;
    c0 = k * VEC;
    q0 = c0 / nf;
    if (CONT) {
      // the vector overlaps segments q0 and (at most) q0 + 1, nf being >= VEC
      edge = (q0 + 1) * nf - c0;                                  // channels of this vector that belong to q0
      xa = q0 < segs ? to_f32(a.pts[tbase + q0]) : 0.0f;
      xb = (q0 + 1 < segs && edge < VEC) ? to_f32(a.pts[tbase + q0 + 1]) : 0.0f;
    } else {
      const int q1 = (c0 + VEC - 1) / nf;
      p = make_uint4(0, 0, 0, 0);
      if (q0 < segs) {
        p = points_table_vec(a, id0, q0, k);
        if (q1 != q0 && q1 < segs) {
          const uint4 q = points_table_vec(a, id1, q1, k);
          p.x |= q.x; p.y |= q.y; p.z |= q.z; p.w |= q.w;        // disjoint support: padding is zero bits
        }
      }
    }
  }
  __device__ __forceinline__ float value(int j) const {
    if (!CONT) return vec_get<T>(p, j);
    const bool first = j < edge;
    const int q = first ? q0 : q0 + 1;
    const int f = first ? c0 - q0 * a.nf + j : j - edge;
    return q < 3 * a.P ? round_to<T>(pe_value(first ? xa : xb, a.dim_t[f], f)) : 0.0f;
  }
};

template <typename T, bool POOL, bool CONT>
__global__ __launch_bounds__(512) void visual_tokens_points_kernel(PointsArgs<T> a) {
  PointsPE<T, CONT> src{a};
  token_row_body<T, POOL>(a.feat, a.newline, a.out, a.out_stride, a.side, a.n, a.C, a.newline_on, src);
}

}  // namespace v3d

using namespace v3d;

extern "C" int v3d_coord_points_voxel(const void* coords, int dtype, int V, int S, int patch, int mode,
                                      const float* min_xyz_host, const float* max_xyz_host, float voxel_size, void* pts,
                                      void* vox, int32_t* ids, void* stream) {
  V3D_REQUIRE(coords && (pts || vox || ids), "v3d_coord_points_voxel: null pointer");
  const int P = points_of_mode(mode);
  V3D_REQUIRE(P > 0, "v3d_coord_points_voxel: unknown mode %d", mode);
  V3D_REQUIRE(V > 0, "v3d_coord_points_voxel: bad shape V=%d", V);
  V3D_REQUIRE(S == kSide && patch == kPatch,
              "v3d_coord_points_voxel: S=%d patch=%d: the sampled-point and min/max encodings are defined for S = 384, patch = 27 only "
              "(the reference hard-codes a 14 x 27 grid)", S, patch);
  Range rg;
  if (int e = fill_range(rg, min_xyz_host, max_xyz_host, voxel_size, "v3d_coord_points_voxel")) return e;
  hipStream_t st = (hipStream_t)stream;
  if (mode == V3D_PTS_MINMAX) {
    V3D_REQUIRE(aligned16(coords), "v3d_coord_points_voxel: coords must be 16-byte aligned");
    const int vecs = kSide * 3 / (dtype == V3D_F32 ? 4 : 8);
    const int threads = ((vecs + 63) / 64) * 64;     // 320 (f32) or 192 (16-bit): one lane per 16-byte column
    V3D_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(coord_minmax_kernel<T>, dim3(kCells, V), dim3(threads), 0, st, (const T*)coords,
                                                 rg, (T*)pts, (T*)vox, ids));
  } else {
    const int64_t total = (int64_t)V * kCells * kCells * P * 3;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    V3D_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(coord_sample_kernel<T>, dim3((int)blocks), dim3(256), 0, st, (const T*)coords,
                                                 total, P, mode, rg, (T*)pts, (T*)vox, ids));
  }
  return check_launch("v3d_coord_points_voxel");
}

static int check_points_shape(const char* who, int E, int P, int dtype, int* nf_out, int* vec_out) {
  V3D_REQUIRE(dtype == V3D_F32 || dtype == V3D_F16 || dtype == V3D_BF16, "%s: unknown dtype code %d", who, dtype);
  V3D_REQUIRE(P >= 1 && P <= 9, "%s: n_points=%d (the reference has 1, 2, 5 and 9)", who, P);
  const int vec = dtype == V3D_F32 ? 4 : 8;
  V3D_REQUIRE(E >= 3 * P, "%s: E=%d too narrow for %d points", who, E, P);
  const int nf = E / (3 * P);
  V3D_REQUIRE(nf >= vec, "%s: E=%d with %d points leaves %d features per axis, the table layout needs at least %d", who, E, P, nf, vec);
  *nf_out = nf;
  *vec_out = vec;
  return V3D_OK;
}

extern "C" int v3d_sin3d_table_points_layout(int embedding_size, int n_points, int dtype, int64_t* row_elems_host,
                                             int32_t* shifts_host) {
  int nf, vec;
  if (int e = check_points_shape("v3d_sin3d_table_points_layout", embedding_size, n_points, dtype, &nf, &vec)) return e;
  const PointsLayout l = points_layout(nf, n_points, vec);
  if (row_elems_host) *row_elems_host = l.row_elems;
  if (shifts_host)
    for (int c = 0; c < l.n_copies; ++c) shifts_host[c] = (int32_t)((l.shift_of_copy >> (4 * c)) & 15u);
  return l.n_copies;
}

extern "C" int v3d_sin3d_table_build_points(const float* dim_t, int embedding_size, int n_points, int n_ids, int dtype,
                                            void* table, void* stream) {
  V3D_REQUIRE(dim_t && table, "v3d_sin3d_table_build_points: null pointer");
  V3D_REQUIRE(n_ids > 0, "v3d_sin3d_table_build_points: bad shape n_ids=%d", n_ids);
  int nf, vec;
  if (int e = check_points_shape("v3d_sin3d_table_build_points", embedding_size, n_points, dtype, &nf, &vec)) return e;
  const PointsLayout l = points_layout(nf, n_points, vec);
  hipStream_t st = (hipStream_t)stream;
  const size_t esz = dtype == V3D_F32 ? 4 : 2;
  hipError_t e = hipMemsetAsync(table, 0, (size_t)l.n_copies * n_ids * l.row_elems * esz, st);
  if (e != hipSuccess) { set_error("v3d_sin3d_table_build_points: memset: %s", hipGetErrorString(e)); return V3D_E_LAUNCH; }
  int64_t blocks = ((int64_t)n_ids * nf + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  V3D_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(sin3d_table_points_kernel<T>, dim3((int)blocks), dim3(256), 0, st, dim_t, nf, n_ids,
                                               l, (T*)table));
  return check_launch("v3d_sin3d_table_build_points");
}

// both forms of PositionEmbeddingSine3D.forward on arbitrary coordinates: the one-point module is the P-point kernel with P = 1
static int launch_sin3d_pe(const char* who, const void* xyz, int dtype, int64_t N, int P, const float* dim_t, int E, void* out, void* stream) {
  int64_t blocks = (N * E + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  V3D_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(sin3d_pe_points_kernel<T>, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream,
                                               (const T*)xyz, N, P, dim_t, E, E / (3 * P), (T*)out));
  return check_launch(who);
}

extern "C" int v3d_sin3d_pe(const void* xyz, int dtype, int64_t N, const float* dim_t, int embedding_size, void* out,
                            void* stream) {
  V3D_REQUIRE(xyz && dim_t && out, "v3d_sin3d_pe: null pointer");
  V3D_REQUIRE(N >= 0 && embedding_size >= 3, "v3d_sin3d_pe: bad shape");
  if (N == 0) return V3D_OK;
  return launch_sin3d_pe("v3d_sin3d_pe", xyz, dtype, N, 1, dim_t, embedding_size, out, stream);
}

extern "C" int v3d_sin3d_pe_points(const void* xyz, int dtype, int64_t N, int n_points, const float* dim_t,
                                   int embedding_size, void* out, void* stream) {
  V3D_REQUIRE(xyz && dim_t && out, "v3d_sin3d_pe_points: null pointer");
  V3D_REQUIRE(N >= 0 && n_points >= 1 && embedding_size >= 3 * n_points, "v3d_sin3d_pe_points: bad shape N=%lld P=%d E=%d",
              (long long)N, n_points, embedding_size);
  if (N == 0) return V3D_OK;
  return launch_sin3d_pe("v3d_sin3d_pe_points", xyz, dtype, N, n_points, dim_t, embedding_size, out, stream);
}

extern "C" int v3d_visual_tokens_points(const void* feat, const int32_t* ids, const void* pts, const void* table, int n_ids,
                                        const float* dim_t, int n_points, const void* newline, void* out, int64_t out_stride,
                                        int dtype, int V, int side, int n, int C, int flags, void* stream) {
  const bool pool = flags & V3D_VT_POOL, pe = flags & V3D_VT_PE, nl = flags & V3D_VT_NEWLINE, cont = flags & V3D_VT_CONTINUOUS;
  V3D_REQUIRE(pe, "v3d_visual_tokens_points: the PE flag is required (v3d_visual_tokens pools without one)");
  V3D_REQUIRE(cont ? (pts && dim_t) : (ids && table && n_ids > 0),
              "v3d_visual_tokens_points: PE needs pts and dim_t (CONTINUOUS) or ids and a table");
  int nf, vec;
  if (int e = check_points_shape("v3d_visual_tokens_points", C, n_points, dtype, &nf, &vec)) return e;
  TokenRowPlan plan;
  if (int e = plan_token_rows("v3d_visual_tokens_points", feat, cont ? nullptr : table, newline, out, out_stride, vec, V, side, n, C, flags, &plan))
    return e;
  hipStream_t st = (hipStream_t)stream;
  V3D_DISPATCH_DTYPE(dtype, {
    PointsArgs<T> a;
    a.feat = (const T*)feat; a.ids = ids; a.pts = (const T*)pts; a.table = (const T*)table; a.dim_t = dim_t;
    a.newline = (const T*)newline; a.out = (T*)out; a.out_stride = out_stride;
    a.lay = points_layout(nf, n_points, vec);
    a.n_ids = n_ids; a.P = n_points; a.nf = nf; a.side = side; a.n = n; a.C = C; a.newline_on = nl ? 1 : 0;
    if (pool && cont) hipLaunchKernelGGL((visual_tokens_points_kernel<T, true, true>), dim3((unsigned)plan.tokens), dim3(plan.threads), 0, st, a);
    else if (pool) hipLaunchKernelGGL((visual_tokens_points_kernel<T, true, false>), dim3((unsigned)plan.tokens), dim3(plan.threads), 0, st, a);
    else if (cont) hipLaunchKernelGGL((visual_tokens_points_kernel<T, false, true>), dim3((unsigned)plan.tokens), dim3(plan.threads), 0, st, a);
    else hipLaunchKernelGGL((visual_tokens_points_kernel<T, false, false>), dim3((unsigned)plan.tokens), dim3(plan.threads), 0, st, a);
  });
  return check_launch("v3d_visual_tokens_points");
}
