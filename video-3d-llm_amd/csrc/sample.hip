// Sampling on the device (do_sample): temperature, top-k, top-p, one seeded categorical draw per row.  The rule is DESIGN
// section 2, "Sampling, stated once"; its shared parts are sample_rule.h.
//
// A 16-bit logit has at most 65536 values and tokens of one value have one probability, so the kept set is "every token above a
// cut value, and the first n_cut tokens (by index) of the cut value".  Three short launches over L2-resident logits:
//   sample_threshold_kernel  one workgroup per row: the cut by bisection over the ordered 16-bit key.  Each probe is one pass over
//                 the row that yields count(key >= c) - an integer - and mass(key >= c) = sum exp(z - z_max), summed in ONE fixed
//                 order (thread t owns tokens t, t + 1024, ...; a butterfly over the wave; the 16 waves in order), so a probe is
//                 reproducible and monotone in c.  No float atomics.  16 probes find the top-k value, 16 more the top-p value;
//                 inside the cut value the counts follow in closed form (top_k - count above; the j with S + j * e < top_p * Z).
//                 When only some tokens of the cut value stay, one more pass counts them per chunk (integer LDS atomics) and
//                 leaves the exclusive prefix, which gives every such token its rank among equals.
//                 Skipped when top_k is off and top_p == 1.
//   sample_draw_kernel       per (row, chunk): the Gumbel key of every kept token (one Philox call per four tokens), the largest
//                 (key, ~index) of the chunk.
//   sample_merge_kernel      per row: the largest of its chunks' pairs -> out_index, the size of the kept set -> kept.
// A row's result depends on its logits, seed, step and stream only: the geometry of the threshold pass is fixed, ranks are
// integers, and the keys of one row are distinct 64-bit words whose maximum does not depend on how the row was cut into chunks.
#include "v3d_common.h"
#include "sample_rule.h"

namespace v3d {

constexpr int ST_THREADS = 1024;                   // threshold: one workgroup per row
constexpr int ST_U = 8;                            // a thread's loads in flight per trip of a pass (one 2-byte load per token: rows start anywhere)
constexpr int SD_THREADS = 256;                    // draw
constexpr int SD_E = 4;                            // consecutive tokens of a thread = one Philox call
constexpr int SD_TILE = SD_THREADS * SD_E;         // 1024
constexpr int SD_CHUNK = 4 * SD_TILE;              // 4096 tokens per workgroup, longer once a row would need more than SD_MAX_CHUNKS
constexpr int SD_MAX_CHUNKS = 256;

struct SampleRowCut { int32_t cut, n_cut, n_eq, kept; };    // tokens with key > cut stay, and n_cut of the n_eq tokens with key == cut

struct SamplePlan {
  int chunk, n_chunks;
  int64_t off_eq, off_part, total;
};

static SamplePlan sample_plan(int M, int V) {
  SamplePlan p;
  int nc = (V + SD_CHUNK - 1) / SD_CHUNK;
  nc = nc < SD_MAX_CHUNKS ? nc : SD_MAX_CHUNKS;
  p.chunk = (int)((((int64_t)V + nc - 1) / nc + SD_TILE - 1) / SD_TILE * SD_TILE);
  p.n_chunks = (int)(((int64_t)V + p.chunk - 1) / p.chunk);
  p.off_eq = ((int64_t)M * sizeof(SampleRowCut) + 255) / 256 * 256;
  p.off_part = p.off_eq + ((int64_t)M * p.n_chunks * 4 + 255) / 256 * 256;
  p.total = p.off_part + (int64_t)M * p.n_chunks * 8;
  return p;
}

// the ordered 16-bit key: monotone in the value, -0 and +0 one key (NaN is outside the contract)
__device__ __forceinline__ int sample_ord(uint16_t v) {
  if (v == 0x8000u) v = 0;
  return (v & 0x8000u) ? (int)(~v & 0xffffu) : (int)(v | 0x8000u);
}
template <typename T> __device__ __forceinline__ float sample_ord_value(int ord) {
  T t;
  t.v = (ord & 0x8000) ? (uint16_t)(ord & 0x7fff) : (uint16_t)(~ord & 0xffff);
  return to_f32(t);
}

__device__ __forceinline__ uint64_t sample_pack(float key, uint32_t index) {
  uint32_t u = __float_as_uint(key);
  if (u == 0x80000000u) u = 0;
  const uint32_t ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);        // never 0 for a non-NaN
  return ((uint64_t)ord << 32) | (uint64_t)(0xffffffffu - index);          // 0 = "no token"
}

// count and mass of the whole workgroup, the same bits in every thread
__device__ __forceinline__ void st_reduce(int& cnt, float& mass, int* sc, float* sm) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    cnt += __shfl_xor(cnt, off);
    mass += __shfl_xor(mass, off);
  }
  if ((threadIdx.x & 63) == 0) { sc[threadIdx.x >> 6] = cnt; sm[threadIdx.x >> 6] = mass; }
  __syncthreads();
  int c = 0;
  float m = 0.f;
#pragma unroll
  for (int w = 0; w < ST_THREADS / 64; ++w) { c += sc[w]; m += sm[w]; }
  __syncthreads();
  cnt = c;
  mass = m;
}

// one probe: count and (with_mass) mass of the tokens whose key is >= c
template <typename T>
__device__ __forceinline__ void st_probe(const T* __restrict__ row, int V, int c, float temp, float zmax, bool with_mass, int* sc, float* sm, int& cnt, float& mass) {
  int n = 0;
  float s = 0.f;
  for (int i0 = threadIdx.x; i0 < V; i0 += ST_THREADS * ST_U) {             // ST_U loads in flight, then the sums in index order
    T x[ST_U];
#pragma unroll
    for (int u = 0; u < ST_U; ++u) {
      const int i = i0 + u * ST_THREADS;
      x[u].v = 0;
      if (i < V) x[u] = row[i];
    }
#pragma unroll
    for (int u = 0; u < ST_U; ++u) {
      if (i0 + u * ST_THREADS < V && sample_ord(x[u].v) >= c) {
        ++n;
        if (with_mass) s += expf(sample_scaled(to_f32(x[u]), temp) - zmax);
      }
    }
  }
  st_reduce(n, s, sc, sm);
  cnt = n;
  mass = s;
}

template <typename T>
__global__ __launch_bounds__(ST_THREADS) void sample_threshold_kernel(const T* __restrict__ x, int64_t ldx, int V, float temp, int top_k, float top_p, int chunk,
                                                                     int n_chunks, SampleRowCut* __restrict__ cuts, int32_t* __restrict__ eq_prefix) {
  __shared__ int sc[ST_THREADS / 64];
  __shared__ float sm[ST_THREADS / 64];
  __shared__ int s_eq[SD_MAX_CHUNKS];
  const int b = blockIdx.x;
  const T* row = x + (int64_t)b * ldx;
  // the largest key of the row
  int omax = 0;
  for (int i0 = threadIdx.x; i0 < V; i0 += ST_THREADS * ST_U) {
#pragma unroll
    for (int u = 0; u < ST_U; ++u) {
      const int i = i0 + u * ST_THREADS;
      if (i < V) omax = max(omax, sample_ord(row[i].v));
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) omax = max(omax, __shfl_xor(omax, off));
  if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = omax;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < ST_THREADS / 64; ++w) omax = max(omax, sc[w]);
  __syncthreads();
  const float zmax = sample_scaled(sample_ord_value<T>(omax), temp);
  const int k = sample_top_k(top_k, V);
  const bool use_k = k < V, use_p = top_p < 1.f;
  int lo = 0, hi = omax + 1, cnt_lo = V, cnt_hi = 0;                       // count(key >= lo) >= k > count(key >= hi)
  float mass_hi = 0.f;
  int cut = 0, n_cut = 0, n_eq = 0, kept = V;
  float Z = 0.f;
  if (use_k) {
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      int c;
      float m;
      st_probe(row, V, mid, temp, zmax, use_p, sc, sm, c, m);
      if (c >= k) { lo = mid; cnt_lo = c; } else { hi = mid; cnt_hi = c; mass_hi = m; }
    }
    cut = lo;
    n_eq = cnt_lo - cnt_hi;
    n_cut = k - cnt_hi;                                                    // 1 .. n_eq
    kept = k;
    Z = mass_hi + (float)n_cut * expf(sample_scaled(sample_ord_value<T>(cut), temp) - zmax);
  } else {
    int c;
    st_probe(row, V, 0, temp, zmax, true, sc, sm, c, Z);
  }
  if (use_p) {
    const float tZ = top_p * Z;
    int plo = lo, phi = omax + 1, cnt_plo = cnt_lo, cnt_phi = 0;           // mass(key >= phi) < tZ, and phi is the smallest such key above lo
    float S = 0.f;
    while (phi - plo > 1) {
      const int mid = (plo + phi) >> 1;
      int c;
      float m;
      st_probe(row, V, mid, temp, zmax, true, sc, sm, c, m);
      if (m < tZ) { phi = mid; cnt_phi = c; S = m; } else { plo = mid; cnt_plo = c; }
    }
    const int cp = phi - 1;
    const int neq = cnt_plo - cnt_phi;
    const float e = expf(sample_scaled(sample_ord_value<T>(cp), temp) - zmax);
    // how many j in [0, neq) have S + j * e < tZ  (j = 0 does: S < tZ)
    int j = neq;
    if (e > 0.f && neq > 0) {
      const float q = (tZ - S) / e;
      j = q >= (float)neq ? neq : (int)ceilf(q);
      j = j < 1 ? 1 : (j > neq ? neq : j);
      for (int it = 0; it < 8 && j > 1 && !(S + (float)(j - 1) * e < tZ); ++it) --j;
      for (int it = 0; it < 8 && j < neq && (S + (float)j * e < tZ); ++it) ++j;
    }
    if (use_k && cp == cut && j > n_cut) j = n_cut;
    cut = cp;
    n_cut = j;
    n_eq = neq;
    kept = cnt_phi + j;
  }
  if (n_cut < n_eq) {                                                      // rank among equals: the cut value's count per chunk, in index order
    for (int i = threadIdx.x; i < n_chunks; i += ST_THREADS) s_eq[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < V; i += ST_THREADS)
      if (sample_ord(row[i].v) == cut) atomicAdd(&s_eq[i / chunk], 1);
    __syncthreads();
    if (threadIdx.x == 0) {
      int run = 0;
      for (int c = 0; c < n_chunks; ++c) {
        eq_prefix[(int64_t)b * n_chunks + c] = run;
        run += s_eq[c];
      }
    }
  }
  if (threadIdx.x == 0) {
    SampleRowCut r;
    r.cut = cut; r.n_cut = n_cut; r.n_eq = n_eq; r.kept = kept;
    cuts[b] = r;
  }
}

// cuts == nullptr: every token is kept
template <typename T>
__global__ __launch_bounds__(SD_THREADS) void sample_draw_kernel(const T* __restrict__ x, int64_t ldx, int V, float temp, uint64_t seed, uint32_t step,
                                                                const int32_t* __restrict__ streams, int chunk, const SampleRowCut* __restrict__ cuts,
                                                                const int32_t* __restrict__ eq_prefix, uint64_t* __restrict__ part) {
  __shared__ int s_wave[SD_THREADS / 64];
  __shared__ uint64_t s_best[SD_THREADS / 64];
  const int c = blockIdx.x, b = blockIdx.y, nc = gridDim.x;
  const T* row = x + (int64_t)b * ldx;
  const uint32_t stream = streams ? (uint32_t)streams[b] : (uint32_t)b;
  int cut = -1, n_cut = 0;
  bool rank = false;
  if (cuts) {
    const SampleRowCut r = cuts[b];
    cut = r.cut;
    n_cut = r.n_cut;
    rank = r.n_cut < r.n_eq;
  }
  int eq_base = rank ? eq_prefix[(int64_t)b * nc + c] : 0;                 // tokens of the cut value before this tile
  const int lo = c * chunk, hi = min(V, lo + chunk);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t best = 0;
  for (int base = lo; base < hi; base += SD_TILE) {
    const int i0 = base + SD_E * threadIdx.x;
    float val[SD_E];
    int ord[SD_E];
    int my_eq = 0;
#pragma unroll
    for (int e = 0; e < SD_E; ++e) {
      const bool in = i0 + e < hi;
      T t;
      t.v = 0;
      if (in) t = row[i0 + e];
      val[e] = to_f32(t);
      ord[e] = in ? sample_ord(t.v) : -2;                                  // below every cut, equal to none
      my_eq += ord[e] == cut ? 1 : 0;
    }
    int before = 0;                                                        // tokens of the cut value before this thread's first
    if (rank) {                                                            // (uniform over the workgroup)
      int inc = my_eq;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
      }
      if (lane == 63) s_wave[wave] = inc;
      __syncthreads();
      int prior = 0, total = 0;
#pragma unroll
      for (int w = 0; w < SD_THREADS / 64; ++w) {
        prior += w < wave ? s_wave[w] : 0;
        total += s_wave[w];
      }
      __syncthreads();
      before = eq_base + prior + inc - my_eq;
      eq_base += total;
    }
    bool keep[SD_E];
    bool any = false;
#pragma unroll
    for (int e = 0; e < SD_E; ++e) {
      keep[e] = ord[e] > cut;
      if (ord[e] == cut) {
        keep[e] = !rank || before < n_cut;
        ++before;
      }
      any = any || keep[e];
    }
    if (any) {
      const Philox4 w = sample_words((uint32_t)i0 >> 2, step, stream, seed);
#pragma unroll
      for (int e = 0; e < SD_E; ++e) {
        if (keep[e]) {
          const uint64_t k = sample_pack(sample_key(val[e], temp, w.w[e]), (uint32_t)(i0 + e));
          best = k > best ? k : best;
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = __shfl_xor((unsigned long long)best, off);
    best = o > best ? o : best;
  }
  if (lane == 0) s_best[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < SD_THREADS / 64; ++w) best = s_best[w] > best ? s_best[w] : best;
    part[(int64_t)b * nc + c] = best;
  }
}

__global__ __launch_bounds__(64) void sample_merge_kernel(const uint64_t* __restrict__ part, int nc, int V, const SampleRowCut* __restrict__ cuts,
                                                         int64_t* __restrict__ out_index, int32_t* __restrict__ kept) {
  const int b = blockIdx.x;
  uint64_t best = 0;
  for (int i = threadIdx.x; i < nc; i += 64) {
    const uint64_t k = part[(int64_t)b * nc + i];
    best = k > best ? k : best;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = __shfl_xor((unsigned long long)best, off);
    best = o > best ? o : best;
  }
  if (threadIdx.x == 0) {
    const uint32_t idx = 0xffffffffu - (uint32_t)best;
    out_index[b] = best && idx < (uint32_t)V ? (int64_t)idx : 0;           // (the kept set is never empty: best != 0)
    if (kept) kept[b] = cuts ? cuts[b].kept : V;
  }
}

}  // namespace v3d

using namespace v3d;

extern "C" int64_t v3d_sample_workspace_bytes(int M, int V) {
  if (!sample_args_ok(M, V, 1.f, 0, 1.f)) return 0;
  return sample_plan(M, V).total;
}

extern "C" int v3d_sample_chunk(int M, int V) {
  if (!sample_args_ok(M, V, 1.f, 0, 1.f)) return 0;
  return sample_plan(M, V).chunk;
}

extern "C" int v3d_sample_rows(const void* logits, int64_t ldx, int M, int V, int dtype, float temperature, int top_k, float top_p, uint64_t seed,
                               int step, const int32_t* streams, int64_t* out_index, int32_t* kept, void* workspace, int64_t workspace_bytes,
                               void* stream) {
  V3D_REQUIRE(logits && out_index && workspace, "v3d_sample_rows: null pointer");
  V3D_REQUIRE(sample_args_ok(M, V, temperature, top_k, top_p),
              "v3d_sample_rows: needs 1 <= M <= %d rows, M * V < 2^31, a finite temperature > 0, top_k >= 0, 0 < top_p <= 1 (M=%d V=%d T=%g top_k=%d top_p=%g)",
              SAMPLE_MAX_M, M, V, (double)temperature, top_k, (double)top_p);
  V3D_REQUIRE(step >= 0, "v3d_sample_rows: step < 0");
  V3D_REQUIRE(dtype == V3D_F16 || dtype == V3D_BF16, "v3d_sample_rows: 16-bit logits only");
  V3D_REQUIRE(M == 1 || ldx >= V, "v3d_sample_rows: ldx < V");
  const SamplePlan p = sample_plan(M, V);
  V3D_REQUIRE(workspace_bytes >= p.total && aligned16(workspace), "v3d_sample_rows: workspace too small or misaligned (%lld bytes needed)", (long long)p.total);
  SampleRowCut* cuts = (SampleRowCut*)workspace;
  int32_t* eq_prefix = (int32_t*)((char*)workspace + p.off_eq);
  uint64_t* part = (uint64_t*)((char*)workspace + p.off_part);
  hipStream_t st = (hipStream_t)stream;
  const bool cutting = sample_top_k(top_k, V) < V || top_p < 1.f;
  const SampleRowCut* use = cutting ? cuts : nullptr;
  const dim3 grid(p.n_chunks, M);
  if (dtype == V3D_F16) {
    if (cutting)
      hipLaunchKernelGGL(sample_threshold_kernel<f16_t>, dim3(M), dim3(ST_THREADS), 0, st, (const f16_t*)logits, ldx, V, temperature, top_k, top_p, p.chunk,
                         p.n_chunks, cuts, eq_prefix);
    hipLaunchKernelGGL(sample_draw_kernel<f16_t>, grid, dim3(SD_THREADS), 0, st, (const f16_t*)logits, ldx, V, temperature, seed, (uint32_t)step, streams,
                       p.chunk, use, eq_prefix, part);
  } else {
    if (cutting)
      hipLaunchKernelGGL(sample_threshold_kernel<bf16_t>, dim3(M), dim3(ST_THREADS), 0, st, (const bf16_t*)logits, ldx, V, temperature, top_k, top_p, p.chunk,
                         p.n_chunks, cuts, eq_prefix);
    hipLaunchKernelGGL(sample_draw_kernel<bf16_t>, grid, dim3(SD_THREADS), 0, st, (const bf16_t*)logits, ldx, V, temperature, seed, (uint32_t)step, streams,
                       p.chunk, use, eq_prefix, part);
  }
  hipLaunchKernelGGL(sample_merge_kernel, dim3(M), dim3(64), 0, st, part, p.n_chunks, V, use, out_index, kept);
  return check_launch("v3d_sample_rows");
}
