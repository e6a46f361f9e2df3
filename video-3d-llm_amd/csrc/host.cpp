// Host side of the C ABI: error reporting and the host-only helpers (frame sampling,
// greedy max-coverage frame selection, the beam-search step's twin, the sampler's twin, the logits processors' twin, the GEMM planner).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "v3d.h"
#include "beam_step.h"
#include "sample_rule.h"
#include "logits_rule.h"
#include "gemm_plan.h"

namespace v3d {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

}  // namespace v3d

extern "C" int v3d_abi_version(void) { return V3D_ABI_VERSION; }
extern "C" const char* v3d_last_error(void) { return v3d::g_err; }

// a1  llava/video_utils.py:187  np.linspace(0, total-1, n, dtype=int)
// numpy: y = arange(n) * (delta/div) + start in f64, y[-1] = stop, floor, cast.
extern "C" int v3d_uniform_frame_indices_host(int total_frames, int n, int32_t* out_host) {
  if (!out_host || total_frames <= 0 || n <= 0) {
    v3d::set_error("v3d_uniform_frame_indices_host: bad arguments total=%d n=%d", total_frames, n);
    return V3D_E_INVALID;
  }
  const double delta = (double)(total_frames - 1);
  const int div = n - 1;
  for (int i = 0; i < n; ++i) {
    double y;
    if (div > 0) {
      const double step = delta / div;
      y = step == 0.0 ? ((double)i / div) * delta : (double)i * step;
    } else {
      y = (double)i * delta;
    }
    out_host[i] = (int32_t)std::floor(y);
  }
  if (n > 1) out_host[n - 1] = total_frames - 1;
  return V3D_OK;
}

// a3  scripts/3d/preprocessing/max_coverage_sampling.py:44-94
static inline uint64_t pack_key(const int32_t* k) {
  // 21 bits per axis, biased: voxel keys of indoor scenes are within +-2^20
  return ((uint64_t)(uint32_t)(k[0] + (1 << 20)) << 42) | ((uint64_t)(uint32_t)(k[1] + (1 << 20)) << 21) |
         (uint64_t)(uint32_t)(k[2] + (1 << 20));
}

extern "C" int v3d_greedy_cover_host(const int32_t* keys_host, int n_frames, int64_t pts_per_frame,
                                     const int32_t* scene_host, int64_t m, int max_frames, int32_t* sel_host,
                                     int64_t* gain_host, int64_t* num_all_host, int64_t* num_sel_host) {
  if (!keys_host || (!scene_host && m > 0) || !sel_host || !gain_host || n_frames <= 0 || pts_per_frame <= 0 || m < 0 ||
      max_frames <= 0) {      // (an empty scene - m == 0, scene pointer unused - is legal, as for the device entry)
    v3d::set_error("v3d_greedy_cover_host: bad arguments");
    return V3D_E_INVALID;
  }
  for (int64_t i = 0; i < (int64_t)n_frames * pts_per_frame * 3; ++i)
    if (keys_host[i] < -(1 << 20) || keys_host[i] >= (1 << 20)) {
      v3d::set_error("v3d_greedy_cover_host: voxel key %d out of the +-2^20 range", keys_host[i]);
      return V3D_E_INVALID;
    }
  // scene voxel set -> sorted unique packed keys; a voxel's rank is its dense index
  std::vector<uint64_t> scene((size_t)m);
  for (int64_t i = 0; i < m; ++i) {
    const int32_t* k = scene_host + i * 3;
    if (k[0] < -(1 << 20) || k[0] >= (1 << 20) || k[1] < -(1 << 20) || k[1] >= (1 << 20) || k[2] < -(1 << 20) ||
        k[2] >= (1 << 20)) {
      v3d::set_error("v3d_greedy_cover_host: scene voxel out of range");
      return V3D_E_INVALID;
    }
    scene[(size_t)i] = pack_key(k);
  }
  std::sort(scene.begin(), scene.end());
  scene.erase(std::unique(scene.begin(), scene.end()), scene.end());
  const size_t ms = scene.size();

  // per frame: dense indices of its unique in-scene voxels (`set(frame) & pc_voxel`, :74)
  std::vector<std::vector<uint32_t>> frame_idx((size_t)n_frames);
  std::vector<uint64_t> tmp((size_t)pts_per_frame);
  std::vector<uint8_t> seen(ms, 0);  // union over frames, for num_all_voxels (:96)
  for (int f = 0; f < n_frames; ++f) {
    const int32_t* k = keys_host + (size_t)f * pts_per_frame * 3;
    for (int64_t p = 0; p < pts_per_frame; ++p) tmp[(size_t)p] = pack_key(k + p * 3);
    std::sort(tmp.begin(), tmp.end());
    const size_t nu = std::unique(tmp.begin(), tmp.end()) - tmp.begin();
    auto& out = frame_idx[(size_t)f];
    size_t j = 0;
    for (size_t i = 0; i < nu && j < ms; ++i) {   // merge of two sorted lists
      while (j < ms && scene[j] < tmp[i]) ++j;
      if (j < ms && scene[j] == tmp[i]) { out.push_back((uint32_t)j); seen[j] = 1; }
    }
  }
  int64_t num_all = 0;
  for (size_t i = 0; i < ms; ++i) num_all += seen[i];

  std::vector<uint8_t> used(ms, 0), taken((size_t)n_frames, 0);
  int picks = 0;
  int64_t num_sel = 0;
  const int limit = std::min(n_frames, max_frames);
  while (picks < limit) {
    int64_t best = -1;
    int best_f = -1;
    for (int f = 0; f < n_frames; ++f) {
      if (taken[(size_t)f]) continue;
      int64_t gain = 0;
      for (uint32_t i : frame_idx[(size_t)f]) gain += !used[i];
      if (gain > best) { best = gain; best_f = f; }   // strict '>' : first (lowest position) wins ties
    }
    for (uint32_t i : frame_idx[(size_t)best_f])
      if (!used[i]) { used[i] = 1; ++num_sel; }
    taken[(size_t)best_f] = 1;
    sel_host[picks] = best_f;
    gain_host[picks] = best;
    ++picks;
  }
  if (num_all_host) *num_all_host = num_all;
  if (num_sel_host) *num_sel_host = num_sel;
  return picks;
}

// a23, num_beams > 1: the twin of v3d_beam_step - the same body (beam_step.h) over host memory
extern "C" int v3d_beam_step_host(const float* cand_score, const int32_t* cand_flat, int K, int B, int V, int max_new_tokens, int step,
                                  const int64_t* eos_ids, int n_eos, const float* div, void* state, int64_t* next_tokens, int32_t* parents,
                                  float* trace_score, int32_t* trace_flat) {
  if (!cand_score || !cand_flat || !div || !state || !next_tokens || !parents || !trace_score || !trace_flat || (!eos_ids && n_eos != 0)) {
    v3d::set_error("v3d_beam_step_host: null pointer");
    return V3D_E_INVALID;
  }
  if (!v3d::beam_step_args_ok(B, K, V, max_new_tokens, step, n_eos)) {
    v3d::set_error("v3d_beam_step_host: bad shape (B=%d K=%d V=%d step=%d of %d, %d EOS ids)", B, K, V, step, max_new_tokens, n_eos);
    return V3D_E_INVALID;
  }
  const v3d::BeamView s = v3d::beam_view((int32_t*)state, B, max_new_tokens);
  if (v3d::beam_step_decide(s, B, K, V, max_new_tokens, step, cand_score, cand_flat, eos_ids, n_eos, div, next_tokens, parents, trace_score, trace_flat))
    v3d::beam_step_move(s, B, V, max_new_tokens, step, cand_flat, 0, 1);
  return V3D_OK;
}

// do_sample: the twin of v3d_sample_rows over f32 logits - the rule of DESIGN section 2 "Sampling, stated once" by a plain sort.
// Philox words, u and the top-k cut are the kernel's bits (sample_rule.h); the top-p mass is summed in f64, keys use this side's logf.
extern "C" int v3d_sample_rows_host(const float* logits, int64_t ldx, int M, int V, float temperature, int top_k, float top_p, uint64_t seed,
                                    int step, const int32_t* streams, int64_t* out_index, int32_t* kept) {
  if (!logits || !out_index) {
    v3d::set_error("v3d_sample_rows_host: null pointer");
    return V3D_E_INVALID;
  }
  if (!v3d::sample_args_ok(M, V, temperature, top_k, top_p) || step < 0 || (M > 1 && ldx < V)) {
    v3d::set_error("v3d_sample_rows_host: bad arguments (M=%d V=%d ldx=%lld T=%g top_k=%d top_p=%g step=%d)", M, V, (long long)ldx, (double)temperature,
                   top_k, (double)top_p, step);
    return V3D_E_INVALID;
  }
  std::vector<int32_t> order((size_t)V);
  for (int m = 0; m < M; ++m) {
    const float* x = logits + (int64_t)m * ldx;
    const uint32_t stream = streams ? (uint32_t)streams[m] : (uint32_t)m;
    for (int i = 0; i < V; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [x](int32_t a, int32_t b) { return x[a] > x[b]; });   // value descending, index ascending
    int n = v3d::sample_top_k(top_k, V);
    if (top_p < 1.f) {
      const float zmax = v3d::sample_scaled(x[order[0]], temperature);
      double Z = 0.0;
      for (int r = 0; r < n; ++r) Z += std::exp((double)(v3d::sample_scaled(x[order[(size_t)r]], temperature) - zmax));
      double before = 0.0;
      int keep = 0;
      for (int r = 0; r < n; ++r) {
        if (!(r == 0 || before / Z < (double)top_p)) break;
        ++keep;
        before += std::exp((double)(v3d::sample_scaled(x[order[(size_t)r]], temperature) - zmax));
      }
      n = keep;
    }
    float best = 0.f;
    int32_t best_i = -1;
    for (int r = 0; r < n; ++r) {
      const int32_t i = order[(size_t)r];
      const v3d::Philox4 w = v3d::sample_words((uint32_t)i >> 2, (uint32_t)step, stream, seed);
      const float key = v3d::sample_key(x[i], temperature, w.w[i & 3]);
      if (best_i < 0 || key > best || (key == best && i < best_i)) { best = key; best_i = i; }
    }
    out_index[m] = best_i;
    if (kept) kept[m] = n;
  }
  return V3D_OK;
}

// The twin of v3d_logits_process_rows over f32 logits that hold 16-bit values ("Logits processors, stated once"):
// the kernel's arithmetic (logits_rule.h) in the kernel's order - every gather of the penalty before any of its stores, then the
// n-gram bans, then the EOS bans.
extern "C" int v3d_logits_process_rows_host(float* logits, int64_t ldx, int M, int V, int dtype, const int64_t* history, int64_t ld_step, int n_prev,
                                            float penalty, int ngram, int min_new, const int64_t* eos_ids, int n_eos) {
  if (!logits || (!history && n_prev > 0) || (!eos_ids && n_eos > 0)) {
    v3d::set_error("v3d_logits_process_rows_host: null pointer");
    return V3D_E_INVALID;
  }
  if (n_prev > v3d::LOGITS_MAX_HISTORY) {
    v3d::set_error("v3d_logits_process_rows_host: a history of %d tokens exceeds LOGITS_MAX_HISTORY = %d", n_prev, v3d::LOGITS_MAX_HISTORY);
    return V3D_E_INVALID;
  }
  if (!v3d::logits_args_ok(M, V, ld_step, n_prev, penalty, ngram, min_new, n_eos) || (dtype != V3D_F16 && dtype != V3D_BF16) || (M > 1 && ldx < V)) {
    v3d::set_error("v3d_logits_process_rows_host: bad arguments (M=%d V=%d ldx=%lld dtype=%d ld_step=%lld n_prev=%d penalty=%g ngram=%d min_new=%d n_eos=%d)", M, V,
                   (long long)ldx, dtype, (long long)ld_step, n_prev, (double)penalty, ngram, min_new, n_eos);
    return V3D_E_INVALID;
  }
  const bool bf = dtype == V3D_BF16;
  const int L = n_prev;
  const float ninf = v3d::logits_widen(v3d::logits_neg_inf(bf), bf);
  std::vector<uint16_t> staged((size_t)L);
  for (int m = 0; m < M; ++m) {
    float* row = logits + (int64_t)m * ldx;
    const int64_t* h = history + m;
    if (penalty != 1.f) {
      for (int j = 0; j < L; ++j) {
        const int64_t v = h[(int64_t)j * ld_step];
        if (v3d::logits_id_ok(v, V)) staged[(size_t)j] = v3d::logits_penalised(v3d::logits_round16(row[v], bf), penalty, bf);
      }
      for (int j = 0; j < L; ++j) {
        const int64_t v = h[(int64_t)j * ld_step];
        if (v3d::logits_id_ok(v, V)) row[v] = v3d::logits_widen(staged[(size_t)j], bf);
      }
    }
    if (ngram > 0 && L + 1 >= ngram) {
      for (int i = 0; i <= L - ngram; ++i) {
        if (!v3d::logits_ngram_match(h, ld_step, L, ngram, i)) continue;
        const int64_t v = h[(int64_t)(i + ngram - 1) * ld_step];
        if (v3d::logits_id_ok(v, V)) row[v] = ninf;
      }
    }
    if (L < min_new) {
      for (int e = 0; e < n_eos; ++e)
        if (v3d::logits_id_ok(eos_ids[e], V)) row[eos_ids[e]] = ninf;
    }
  }
  return V3D_OK;
}

extern "C" int v3d_philox4x32_10_host(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
  if (!counter || !key || !out) {
    v3d::set_error("v3d_philox4x32_10_host: null pointer");
    return V3D_E_INVALID;
  }
  const v3d::Philox4 w = v3d::philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1]);
  for (int i = 0; i < 4; ++i) out[i] = w.w[i];
  return V3D_OK;
}

// The plan v3d_gemm makes for a shape on a chip of `slots` CUs at the default switches (gemm_plan.h): kernel 0 = skinny,
// 1 = 128 x 128, 2 = 256 x 256, 3 = 192 x 256; dp / split: the split-K tail's whole-tile rounds and K-chunks (-1 / 1: no tail)
extern "C" int v3d_gemm_plan_host(int M, int N, int K, int slots, int* kernel, int* tiles, int* dp, int* split) {
  if (!(M > 0 && N > 0 && K > 0 && N % v3d::BN == 0 && K % v3d::BK == 0 && slots > 0)) {
    v3d::set_error("v3d_gemm_plan_host: bad shape");
    return V3D_E_INVALID;
  }
  if (!(kernel && tiles && dp && split)) {
    v3d::set_error("v3d_gemm_plan_host: null pointer");
    return V3D_E_INVALID;
  }
  if (M <= 8) { *kernel = 0; *tiles = 0; *dp = -1; *split = 1; return V3D_OK; }
  const v3d::GemmPlan g = v3d::gemm_plan(M, N, K, slots, 0, true, 1);
  *kernel = g.kernel; *tiles = g.tiles; *dp = g.sk > 0 ? g.dp : -1; *split = g.sk > 0 ? g.split : 1;
  return V3D_OK;
}
