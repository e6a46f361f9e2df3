// One beam-search step ("Beam search, stated once"): the body shared by the kernel v3d_beam_step (beam.hip)
// and its host twin v3d_beam_step_host (host.cpp).  Plain C++ with no library call, so that both compile the same arithmetic:
// f32 additions and IEEE divisions only (no reciprocal, nothing a compiler may contract).
//
// The rule is GenerationMixin._beam_search of transformers 5.x for batch 1, do_sample=False, num_return_sequences=1,
// early_stopping=False, no logits processors, stopping by EOS ids and max_new_tokens; ties between equal f32 scores go to the
// LOWER position (flat index among candidates, position in [finished | candidates] in the merge) - torch.topk leaves them open.
//
// State: one block of 4-byte words (beam_state_words), laid out by beam_view:
//   hdr[BEAM_H_DONE]        int32 word, 0 or 1 (not a count): the search has ended; every later step is a no-op
//   hdr[BEAM_H_IMPROVABLE]  the sticky early-stop heuristic flag, starts at 1
//   hdr[BEAM_H_STEPS]       steps executed so far (T); the live sequence buffers are run_seq[T & 1] / fin_seq[T & 1]
//   run_score f32[B] (init 0, -1e9, ...), fin_score f32[B] (init -1e9), fin_flag[B], fin_len[B], run_src[B], fin_src[B] (the
//   step's plan: which candidate / merged entry each new row comes from), run_seq[2][B][L], fin_seq[2][B][L] (int32 token ids).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define V3D_HD __host__ __device__
#else
#define V3D_HD
#endif

namespace v3d {

constexpr int BEAM_MAX_B = 16;       // two sets of 16 K/V slices (Engine._answer_state)
constexpr int BEAM_MAX_K = 64;
constexpr int BEAM_MAX_EOS = 8;
constexpr float BEAM_NEG = -1.0e9f;
enum { BEAM_H_DONE = 0, BEAM_H_IMPROVABLE = 1, BEAM_H_STEPS = 2, BEAM_H_WORDS = 4 };

struct BeamView {
  int32_t* hdr;
  float* run_score;
  float* fin_score;
  int32_t* fin_flag;
  int32_t* fin_len;
  int32_t* run_src;
  int32_t* fin_src;
  int32_t* run_seq[2];
  int32_t* fin_seq[2];
};

V3D_HD inline int64_t beam_state_words(int B, int L) { return BEAM_H_WORDS + 6 * (int64_t)B + 4 * (int64_t)B * L; }

V3D_HD inline BeamView beam_view(int32_t* s, int B, int L) {
  BeamView v;
  v.hdr = s;
  int32_t* p = s + BEAM_H_WORDS;
  v.run_score = reinterpret_cast<float*>(p); p += B;
  v.fin_score = reinterpret_cast<float*>(p); p += B;
  v.fin_flag = p; p += B;
  v.fin_len = p; p += B;
  v.run_src = p; p += B;
  v.fin_src = p; p += B;
  const int64_t n = (int64_t)B * L;
  v.run_seq[0] = p; v.run_seq[1] = p + n; v.fin_seq[0] = p + 2 * n; v.fin_seq[1] = p + 3 * n;
  return v;
}

// a candidate's flat index, forced into [0, B * V) so that a corrupt one can never index outside the state
V3D_HD inline int32_t beam_flat(int32_t f, int B, int V) {
  const int64_t hi = (int64_t)B * V - 1;
  return f < 0 ? 0 : ((int64_t)f > hi ? (int32_t)hi : f);
}

// The decisions of step t (serial; B <= 16, K <= 64): next running beams, finished merge, heuristic, done.  Writes the plan
// (run_src / fin_src), the scores and flags, next_tokens / parents and trace row t.  Returns false when the search had ended.
V3D_HD inline bool beam_step_decide(const BeamView& s, int B, int K, int V, int L, int t, const float* cand_score, const int32_t* cand_flat,
                                    const int64_t* eos, int n_eos, const float* div, int64_t* next_tokens, int32_t* parents,
                                    float* trace_score, int32_t* trace_flat) {
  if (s.hdr[BEAM_H_DONE]) return false;
  const int n = t + 1;                                     // tokens generated after this step
  const bool improvable = s.hdr[BEAM_H_IMPROVABLE] != 0;   // as of the previous step
  const float d = div[n];
  float adj[BEAM_MAX_K];                                   // running-beam key: stopping candidates pushed down by -1e9
  float fsc[BEAM_MAX_K];                                   // finished key: normalised score, -1e9 per reason it is not eligible
  bool stop[BEAM_MAX_K], used[BEAM_MAX_K + BEAM_MAX_B];
  bool all_stop = true;
  for (int k = 0; k < K; ++k) {
    const int32_t f = beam_flat(cand_flat[k], B, V);
    const int64_t tok = f % V;
    bool st = n >= L;
    for (int e = 0; e < n_eos; ++e) st = st || tok == eos[e];
    stop[k] = st;
    all_stop = all_stop && st;
    const float sc = cand_score[k];
    trace_score[(int64_t)t * K + k] = sc;
    trace_flat[(int64_t)t * K + k] = cand_flat[k];
    adj[k] = st ? sc + BEAM_NEG : sc;
    float fs = sc / d;
    if (!improvable) fs = fs + BEAM_NEG;
    if (!(st && k < B)) fs = fs + BEAM_NEG;
    fsc[k] = fs;
    used[k] = false;
  }
  // next running beams: the B largest adj, the lower rank first among equals
  for (int b = 0; b < B; ++b) {
    int best = -1;
    for (int k = 0; k < K; ++k)
      if (!used[k] && (best < 0 || adj[k] > adj[best])) best = k;
    used[best] = true;
    const int32_t f = beam_flat(cand_flat[best], B, V);
    s.run_src[b] = best;
    s.run_score[b] = adj[best];
    parents[b] = f / V;
    next_tokens[b] = f % V;
  }
  // finished: [old finished | candidates], the B largest, the earlier position first among equals
  float old_score[BEAM_MAX_B];
  int32_t old_flag[BEAM_MAX_B], old_len[BEAM_MAX_B];
  for (int i = 0; i < B; ++i) { old_score[i] = s.fin_score[i]; old_flag[i] = s.fin_flag[i]; old_len[i] = s.fin_len[i]; }
  for (int i = 0; i < B + K; ++i) used[i] = false;
  for (int b = 0; b < B; ++b) {
    int best = -1;
    float bv = 0.f;
    for (int i = 0; i < B + K; ++i) {
      if (used[i]) continue;
      const float v = i < B ? old_score[i] : fsc[i - B];
      if (best < 0 || v > bv) { best = i; bv = v; }
    }
    used[best] = true;
    s.fin_src[b] = best;
    s.fin_score[b] = bv;
    s.fin_flag[b] = best < B ? old_flag[best] : (int32_t)(stop[best - B] && best - B < B);
    s.fin_len[b] = best < B ? old_len[best] : n;
  }
  // heuristic: can the best running beam, at this length, still beat the worst finished entry?
  float worst = s.fin_score[0];
  for (int i = 1; i < B; ++i) worst = s.fin_score[i] < worst ? s.fin_score[i] : worst;
  const float hope = s.run_score[0] / d;
  bool any = false;
  for (int i = 0; i < B; ++i) any = any || hope > (s.fin_flag[i] ? worst : BEAM_NEG);
  const bool imp = improvable && any;
  s.hdr[BEAM_H_IMPROVABLE] = imp ? 1 : 0;
  s.hdr[BEAM_H_DONE] = (!imp || all_stop) ? 1 : 0;
  s.hdr[BEAM_H_STEPS] = n;
  return true;
}

// The sequence moves of step t after beam_step_decide returned true: item `tid` of `nthreads` cooperating callers (the kernel's
// threads; the twin calls it once with (0, 1)).  Reads buffers t & 1, writes the other pair.
V3D_HD inline void beam_step_move(const BeamView& s, int B, int V, int L, int t, const int32_t* cand_flat, int tid, int nthreads) {
  const int cur = t & 1, nxt = cur ^ 1, n = t + 1;
  for (int idx = tid; idx < B * n; idx += nthreads) {
    const int b = idx / n, j = idx - b * n;
    {
      const int32_t f = beam_flat(cand_flat[s.run_src[b]], B, V);
      s.run_seq[nxt][(int64_t)b * L + j] = j < t ? s.run_seq[cur][(int64_t)(f / V) * L + j] : f % V;
    }
    const int src = s.fin_src[b];
    int32_t v;
    if (src < B) {
      v = j < s.fin_len[b] ? s.fin_seq[cur][(int64_t)src * L + j] : 0;
    } else {
      const int32_t f = beam_flat(cand_flat[src - B], B, V);
      v = j < t ? s.run_seq[cur][(int64_t)(f / V) * L + j] : f % V;
    }
    s.fin_seq[nxt][(int64_t)b * L + j] = v;
  }
}

V3D_HD inline bool beam_step_args_ok(int B, int K, int V, int L, int t, int n_eos) {
  return B >= 1 && B <= BEAM_MAX_B && K >= B && K <= BEAM_MAX_K && V >= 1 && (int64_t)B * V < (1ll << 31) && L >= 1 && t >= 0 && t < L &&
         n_eos >= 0 && n_eos <= BEAM_MAX_EOS;
}

}  // namespace v3d
