// Beam search on the device (a23, num_beams > 1): top-K over beams x vocab, the beam bookkeeping, the K/V reorder.
//
// v3d_beam_topk   score[b, v] = running[b] + (x[b, v] - lse_b) in f32, the K largest (score, flat = b * V + v) pairs, equal scores
//                 in ascending flat order.  Every candidate is ONE 64-bit key, [ordered score bits | ~flat]: the larger key is the
//                 better candidate, keys are distinct, and the tie rule rides in the low word through every stage - a selection
//                 never depends on the slot a value happened to land in.  Three short launches over L2-resident logits:
//                 per (row, chunk) max / sum-of-exponentials; per (row, chunk) the chunk's K largest keys (the row's lse is
//                 re-formed from the partials by every workgroup, in one fixed order); one workgroup merges the lists.
//                 (The lse has to be known BEFORE a chunk selects: selecting on the raw logit and scoring afterwards is not the
//                 same rule - two logits may round to one f32 score, and then the lower flat index wins, not the larger logit.)
// v3d_beam_step   one workgroup: thread 0 takes the decisions (beam_step.h, the body the host twin compiles too), all threads
//                 move the sequences.
// v3d_beam_kv_gather  every layer's rows [S, S + n) of slice src_base + parents[b] -> slice dst_base + b, one launch, 16-byte
//                 loads and stores; the two slice sets are disjoint, so no read can see a write of the same launch.
// All three return at once when the search's done word is set: the steps queued behind the host's late read are harmless.
#include "v3d_common.h"
#include "beam_step.h"

namespace v3d {

constexpr int BT_THREADS = 256;
constexpr int BT_E = 16;                          // keys a thread holds per tile
constexpr int BT_TILE = BT_THREADS * BT_E;        // 4096
constexpr int BT_MAX_LISTS = 256;                 // (row, chunk) pairs per call at most (M > 256 / chunks: longer chunks)

struct BeamTopkPlan {
  int chunk, n_chunks;
  int64_t off_lists, total;
};

static BeamTopkPlan beam_topk_plan(int M, int V, int K) {
  BeamTopkPlan p;
  int nc = (V + BT_TILE - 1) / BT_TILE;
  const int cap = BT_MAX_LISTS / M > 1 ? BT_MAX_LISTS / M : 1;
  nc = nc < cap ? nc : cap;
  p.chunk = ((V + nc - 1) / nc + 7) / 8 * 8;
  p.n_chunks = (V + p.chunk - 1) / p.chunk;
  p.off_lists = ((int64_t)M * p.n_chunks * 8 + 255) / 256 * 256;          // float2 partials first
  p.total = p.off_lists + (int64_t)M * p.n_chunks * K * 8;
  return p;
}

__device__ __forceinline__ uint64_t beam_key(float score, uint32_t flat) {
  uint32_t u = __float_as_uint(score);
  if (u == 0x80000000u) u = 0;                                            // -0 and +0 are one score
  const uint32_t ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);        // monotone in the float order; never 0 for a non-NaN
  return ((uint64_t)ord << 32) | (uint64_t)(0xffffffffu - flat);          // 0 = "no candidate"
}
__device__ __forceinline__ float beam_key_score(uint64_t key) {
  const uint32_t ord = (uint32_t)(key >> 32);
  return __uint_as_float((ord & 0x80000000u) ? (ord & 0x7fffffffu) : ~ord);
}
__device__ __forceinline__ int32_t beam_key_flat(uint64_t key) { return (int32_t)(0xffffffffu - (uint32_t)key); }

__device__ __forceinline__ float beam_wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ float beam_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// launch 1: (max, sum exp(x - max)) of chunk c of row b
template <typename T>
__global__ __launch_bounds__(BT_THREADS) void beam_lse_part_kernel(const T* __restrict__ x, int64_t ldx, int V, int chunk, const float* __restrict__ running,
                                                                  const int32_t* __restrict__ done, float2* __restrict__ part) {
  __shared__ float sm[4];
  if (done && *done) return;
  const int c = blockIdx.x, b = blockIdx.y;
  if (running[b] <= BEAM_NEG) return;                                     // a dead beam: its row is never read
  const T* row = x + (int64_t)b * ldx;
  const int lo = c * chunk, hi = min(V, lo + chunk);
  float m = -INFINITY;
  for (int i = lo + threadIdx.x; i < hi; i += BT_THREADS) m = fmaxf(m, to_f32(row[i]));
  m = beam_wave_max(m);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
  __syncthreads();
  float s = 0.f;
  for (int i = lo + threadIdx.x; i < hi; i += BT_THREADS) s += expf(to_f32(row[i]) - m);
  s = beam_wave_sum(s);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[(int64_t)b * gridDim.x + c] = make_float2(m, (sm[0] + sm[1]) + (sm[2] + sm[3]));
}

// K rounds of "largest key of the workgroup": keys[BT_E] are this tile's, keys[BT_E] slot BT_E the list entry carried over from
// the tiles before.  The winner of round r goes to list[r] and leaves its owner's registers.  sm: 8 words, two round buffers.
__device__ __forceinline__ void beam_topk_rounds(uint64_t (&keys)[BT_E + 1], int K, uint64_t* __restrict__ list, uint64_t* __restrict__ sm) {
  uint64_t lm = 0;
#pragma unroll
  for (int i = 0; i <= BT_E; ++i) lm = keys[i] > lm ? keys[i] : lm;
  const int wave = threadIdx.x >> 6;
  for (int r = 0; r < K; ++r) {
    uint64_t w = lm;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint64_t o = __shfl_xor((unsigned long long)w, off);
      w = o > w ? o : w;
    }
    uint64_t* buf = sm + (r & 1) * 4;
    if ((threadIdx.x & 63) == 0) buf[wave] = w;
    __syncthreads();
    uint64_t g = buf[0];
    g = buf[1] > g ? buf[1] : g;
    g = buf[2] > g ? buf[2] : g;
    g = buf[3] > g ? buf[3] : g;
    if (threadIdx.x == 0) list[r] = g;
    if (g != 0 && lm == g) {                                              // keys are distinct: exactly one owner
      lm = 0;
#pragma unroll
      for (int i = 0; i <= BT_E; ++i) {
        if (keys[i] == g) keys[i] = 0;
        lm = keys[i] > lm ? keys[i] : lm;
      }
    }
  }
  __syncthreads();                                                        // list[] complete and visible
}

// launch 2: the K largest keys of chunk c of row b -> lists[(b * n_chunks + c) * K ..]
template <typename T>
__global__ __launch_bounds__(BT_THREADS) void beam_topk_part_kernel(const T* __restrict__ x, int64_t ldx, int V, int chunk, int K,
                                                                   const float* __restrict__ running, const int32_t* __restrict__ done,
                                                                   const float2* __restrict__ part, uint64_t* __restrict__ lists) {
  __shared__ uint64_t list[BEAM_MAX_K];
  __shared__ uint64_t sm[8];
  __shared__ float s_lse;
  if (done && *done) return;
  const int c = blockIdx.x, b = blockIdx.y, nc = gridDim.x;
  uint64_t* out = lists + ((int64_t)b * nc + c) * K;
  const float run = running[b];
  if (run <= BEAM_NEG) {                                                  // a dead beam can never win: an empty list
    if (threadIdx.x < K) out[threadIdx.x] = 0;
    return;
  }
  if (threadIdx.x < 64) {                                                 // the row's lse from its partials, one fixed order for every workgroup
    const float2* pr = part + (int64_t)b * nc;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < nc; i += 64) m = fmaxf(m, pr[i].x);
    m = beam_wave_max(m);
    float s = 0.f;
    for (int i = threadIdx.x; i < nc; i += 64) s += pr[i].y * expf(pr[i].x - m);
    s = beam_wave_sum(s);
    if (threadIdx.x == 0) s_lse = m + logf(s);
  }
  if (threadIdx.x < K) list[threadIdx.x] = 0;
  __syncthreads();
  const float lse = s_lse;
  const T* row = x + (int64_t)b * ldx;
  const int lo = c * chunk, hi = min(V, lo + chunk);
  for (int base = lo; base < hi; base += BT_TILE) {
    uint64_t keys[BT_E + 1];
#pragma unroll
    for (int i = 0; i < BT_E; ++i) {
      const int v = base + i * BT_THREADS + threadIdx.x;
      keys[i] = v < hi ? beam_key(run + (to_f32(row[v]) - lse), (uint32_t)b * (uint32_t)V + (uint32_t)v) : 0;
    }
    keys[BT_E] = threadIdx.x < K ? list[threadIdx.x] : 0;
    __syncthreads();                                                      // everyone has read list[] before round 0 rewrites it
    beam_topk_rounds(keys, K, list, sm);
  }
  if (threadIdx.x < K) out[threadIdx.x] = list[threadIdx.x];
}

// launch 3: the K largest of all lists, decoded
__global__ __launch_bounds__(BT_THREADS) void beam_topk_merge_kernel(const uint64_t* __restrict__ lists, int64_t n_keys, int K, const int32_t* __restrict__ done,
                                                                    float* __restrict__ cand_score, int32_t* __restrict__ cand_flat) {
  __shared__ uint64_t list[BEAM_MAX_K];
  __shared__ uint64_t sm[8];
  if (done && *done) return;
  if (threadIdx.x < K) list[threadIdx.x] = 0;
  __syncthreads();
  for (int64_t base = 0; base < n_keys; base += BT_TILE) {
    uint64_t keys[BT_E + 1];
#pragma unroll
    for (int i = 0; i < BT_E; ++i) {
      const int64_t j = base + i * BT_THREADS + threadIdx.x;
      keys[i] = j < n_keys ? lists[j] : 0;
    }
    keys[BT_E] = threadIdx.x < K ? list[threadIdx.x] : 0;
    __syncthreads();
    beam_topk_rounds(keys, K, list, sm);
  }
  if (threadIdx.x < K) {
    const uint64_t k = list[threadIdx.x];
    cand_score[threadIdx.x] = k ? beam_key_score(k) : -INFINITY;          // (k == 0 cannot happen: K <= V and beam 0 is never dead)
    cand_flat[threadIdx.x] = k ? beam_key_flat(k) : 0;
  }
}

__global__ __launch_bounds__(BT_THREADS) void beam_step_kernel(int32_t* __restrict__ state, int B, int K, int V, int L, int t, const float* __restrict__ cand_score,
                                                              const int32_t* __restrict__ cand_flat, const int64_t* __restrict__ eos, int n_eos,
                                                              const float* __restrict__ div, int64_t* __restrict__ next_tokens, int32_t* __restrict__ parents,
                                                              float* __restrict__ trace_score, int32_t* __restrict__ trace_flat) {
  __shared__ int ran;
  const BeamView s = beam_view(state, B, L);
  if (threadIdx.x == 0)
    ran = beam_step_decide(s, B, K, V, L, t, cand_score, cand_flat, eos, n_eos, div, next_tokens, parents, trace_score, trace_flat) ? 1 : 0;
  __syncthreads();                                                        // (also orders thread 0's global writes before the moves of this workgroup)
  if (!ran) return;
  beam_step_move(s, B, V, L, t, cand_flat, threadIdx.x, BT_THREADS);
}

// grid (x: 16-byte vectors of the n rows, y: beam, z: layer)
__global__ __launch_bounds__(256) void beam_kv_gather_kernel(void* const* __restrict__ layers, int64_t slice_stride, int64_t row_stride, int vec_per_row, int S, int n,
                                                            int src_base, int dst_base, int B, const int32_t* __restrict__ parents, const int32_t* __restrict__ done) {
  if (done && *done) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n * vec_per_row) return;
  const int b = blockIdx.y;
  const int p = parents[b];
  if (p < 0 || p >= B) return;                                            // never index outside the source set
  const int r = i / vec_per_row, c = i - r * vec_per_row;
  uint16_t* base = (uint16_t*)layers[blockIdx.z];
  const uint4* src = reinterpret_cast<const uint4*>(base + (int64_t)(src_base + p) * slice_stride + (int64_t)(S + r) * row_stride) + c;
  uint4* dst = reinterpret_cast<uint4*>(base + (int64_t)(dst_base + b) * slice_stride + (int64_t)(S + r) * row_stride) + c;
  *dst = *src;
}

}  // namespace v3d

using namespace v3d;

static bool beam_topk_shape_ok(int M, int V, int K) { return M >= 1 && M <= BEAM_MAX_B && K >= 1 && K <= BEAM_MAX_K && V >= K && (int64_t)M * V < (1ll << 31); }

extern "C" int64_t v3d_beam_topk_workspace_bytes(int M, int V, int K) {
  if (!beam_topk_shape_ok(M, V, K)) return 0;
  return beam_topk_plan(M, V, K).total;
}

extern "C" int v3d_beam_topk_chunk(int M, int V) {
  if (!beam_topk_shape_ok(M, V, 1)) return 0;
  return beam_topk_plan(M, V, 1).chunk;
}

extern "C" int v3d_beam_topk(const void* logits, int64_t ldx, int M, int V, int dtype, const float* running, int K, float* cand_score,
                             int32_t* cand_flat, const int32_t* done, void* workspace, int64_t workspace_bytes, void* stream) {
  V3D_REQUIRE(logits && running && cand_score && cand_flat && workspace, "v3d_beam_topk: null pointer");
  V3D_REQUIRE(beam_topk_shape_ok(M, V, K), "v3d_beam_topk: needs 1 <= M <= %d rows, 1 <= K <= %d, K <= V, M * V < 2^31 (M=%d V=%d K=%d)", BEAM_MAX_B,
              BEAM_MAX_K, M, V, K);
  V3D_REQUIRE(dtype == V3D_F16 || dtype == V3D_BF16, "v3d_beam_topk: 16-bit logits only");
  V3D_REQUIRE(M == 1 || ldx >= V, "v3d_beam_topk: ldx < V");
  const BeamTopkPlan p = beam_topk_plan(M, V, K);
  V3D_REQUIRE(workspace_bytes >= p.total && aligned16(workspace), "v3d_beam_topk: workspace too small or misaligned (%lld bytes needed)", (long long)p.total);
  float2* part = (float2*)workspace;
  uint64_t* lists = (uint64_t*)((char*)workspace + p.off_lists);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(p.n_chunks, M);
  if (dtype == V3D_F16) {
    hipLaunchKernelGGL(beam_lse_part_kernel<f16_t>, grid, dim3(BT_THREADS), 0, st, (const f16_t*)logits, ldx, V, p.chunk, running, done, part);
    hipLaunchKernelGGL(beam_topk_part_kernel<f16_t>, grid, dim3(BT_THREADS), 0, st, (const f16_t*)logits, ldx, V, p.chunk, K, running, done, part, lists);
  } else {
    hipLaunchKernelGGL(beam_lse_part_kernel<bf16_t>, grid, dim3(BT_THREADS), 0, st, (const bf16_t*)logits, ldx, V, p.chunk, running, done, part);
    hipLaunchKernelGGL(beam_topk_part_kernel<bf16_t>, grid, dim3(BT_THREADS), 0, st, (const bf16_t*)logits, ldx, V, p.chunk, K, running, done, part, lists);
  }
  hipLaunchKernelGGL(beam_topk_merge_kernel, dim3(1), dim3(BT_THREADS), 0, st, lists, (int64_t)M * p.n_chunks * K, K, done, cand_score, cand_flat);
  return check_launch("v3d_beam_topk");
}

extern "C" int64_t v3d_beam_state_bytes(int B, int max_new_tokens) {
  if (B < 1 || B > BEAM_MAX_B || max_new_tokens < 1) return 0;
  return beam_state_words(B, max_new_tokens) * 4;
}

extern "C" int v3d_beam_step(const float* cand_score, const int32_t* cand_flat, int K, int B, int V, int max_new_tokens, int step,
                             const int64_t* eos_ids, int n_eos, const float* div, void* state, int64_t* next_tokens, int32_t* parents,
                             float* trace_score, int32_t* trace_flat, void* stream) {
  V3D_REQUIRE(cand_score && cand_flat && div && state && next_tokens && parents && trace_score && trace_flat && (eos_ids || n_eos == 0),
              "v3d_beam_step: null pointer");
  V3D_REQUIRE(beam_step_args_ok(B, K, V, max_new_tokens, step, n_eos),
              "v3d_beam_step: needs 1 <= B <= %d, B <= K <= %d, 0 <= step < max_new_tokens, at most %d EOS ids (B=%d K=%d V=%d step=%d of %d, %d EOS ids)",
              BEAM_MAX_B, BEAM_MAX_K, BEAM_MAX_EOS, B, K, V, step, max_new_tokens, n_eos);
  hipLaunchKernelGGL(beam_step_kernel, dim3(1), dim3(BT_THREADS), 0, (hipStream_t)stream, (int32_t*)state, B, K, V, max_new_tokens, step, cand_score, cand_flat,
                     eos_ids, n_eos, div, next_tokens, parents, trace_score, trace_flat);
  return check_launch("v3d_beam_step");
}

extern "C" int v3d_beam_kv_gather(void* const* layer_ptrs, int n_layers, int64_t slice_stride, int64_t row_stride, int width, int n_slices, int64_t slice_rows,
                                  int S, int n, int src_base, int dst_base, int B, const int32_t* parents, const int32_t* done, void* stream) {
  V3D_REQUIRE(layer_ptrs && parents, "v3d_beam_kv_gather: null pointer");
  V3D_REQUIRE(n_layers >= 1 && n_layers <= 65535 && B >= 1 && B <= BEAM_MAX_B && width > 0 && width % 8 == 0 && row_stride >= width && row_stride % 8 == 0 &&
                  slice_stride % 8 == 0 && slice_stride >= slice_rows * row_stride,
              "v3d_beam_kv_gather: bad shape (16-bit rows in 16-byte vectors: width, row and slice strides multiples of 8 elements)");
  V3D_REQUIRE(S >= 0 && n >= 0 && (int64_t)S + n <= slice_rows, "v3d_beam_kv_gather: rows [%d, %d) outside the %lld rows of a slice", S, S + n, (long long)slice_rows);
  V3D_REQUIRE(src_base >= 0 && dst_base >= 0 && src_base + B <= n_slices && dst_base + B <= n_slices && (src_base + B <= dst_base || dst_base + B <= src_base),
              "v3d_beam_kv_gather: the source and destination slice sets must be disjoint and inside the %d slices", n_slices);
  if (n == 0) return V3D_OK;
  const int vec = width / 8;
  V3D_REQUIRE((int64_t)n * vec < (1ll << 30), "v3d_beam_kv_gather: too many rows");
  hipLaunchKernelGGL(beam_kv_gather_kernel, dim3((unsigned)(((int64_t)n * vec + 255) / 256), B, n_layers), dim3(256), 0, (hipStream_t)stream, layer_ptrs,
                     slice_stride, row_stride, vec, S, n, src_base, dst_base, B, parents, done);
  return check_launch("v3d_beam_kv_gather");
}
