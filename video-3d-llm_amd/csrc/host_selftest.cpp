// Sanitizer self-test of the HOST half of the C ABI (csrc/host.cpp): built by `make -C video-3d-llm_amd/csrc sanitize` with
// g++ -fsanitize=address,undefined (GPU AddressSanitizer is not available on this pool; the device entry points validate their
// arguments on the host before any launch and are exercised by tests/test_abi_host.py and the -m gpu tests).
// Exercises the valid paths on ragged sizes and every argument-validation branch; exits non-zero on a wrong answer.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <tuple>
#include <vector>

#include "v3d.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "host_selftest: %s failed at line %d (%s)\n", #c, __LINE__, v3d_last_error()); return 1; } } while (0)

int main() {
  CHECK(v3d_abi_version() == V3D_ABI_VERSION);
  // a1: np.linspace(0, n-1, F, dtype=int)
  for (int total : {1, 2, 7, 31, 32, 33, 100, 517}) {
    for (int n : {1, 8, 32, 600}) {
      std::vector<int32_t> out(n, -1);
      CHECK(v3d_uniform_frame_indices_host(total, n, out.data()) == V3D_OK);
      CHECK(out[0] == 0 && (n == 1 || out[n - 1] == total - 1));
      for (int i = 1; i < n; ++i) CHECK(out[i] >= out[i - 1] && out[i] < total);
    }
  }
  int32_t one = 0;
  CHECK(v3d_uniform_frame_indices_host(0, 4, &one) == V3D_E_INVALID && std::strlen(v3d_last_error()) > 0);
  CHECK(v3d_uniform_frame_indices_host(4, 0, &one) == V3D_E_INVALID);
  CHECK(v3d_uniform_frame_indices_host(4, 4, nullptr) == V3D_E_INVALID);
  // a3: greedy max-coverage against a brute-force set implementation
  std::srand(7);
  for (int trial = 0; trial < 6; ++trial) {
    const int n_frames = 3 + trial * 5, pts = 40 + 13 * trial;
    std::vector<int32_t> keys((size_t)n_frames * pts * 3);
    for (auto& k : keys) k = std::rand() % 9 - 4;
    std::set<std::tuple<int, int, int>> scene;
    std::vector<int32_t> sc;
    for (int i = 0; i < 120; ++i) {
      const int a = std::rand() % 9 - 4, b = std::rand() % 9 - 4, c = std::rand() % 9 - 4;
      sc.push_back(a); sc.push_back(b); sc.push_back(c);          // duplicates on purpose
      scene.insert({a, b, c});
    }
    const int max_frames = 4 + trial;
    std::vector<int32_t> sel(max_frames);
    std::vector<int64_t> gain(max_frames);
    int64_t n_all = -1, n_sel = -1;
    const int picks = v3d_greedy_cover_host(keys.data(), n_frames, pts, sc.data(), (int64_t)sc.size() / 3, max_frames, sel.data(), gain.data(), &n_all, &n_sel);
    CHECK(picks >= 0 && picks <= max_frames);
    std::vector<std::set<std::tuple<int, int, int>>> fs(n_frames);
    std::set<std::tuple<int, int, int>> all;
    for (int f = 0; f < n_frames; ++f)
      for (int p = 0; p < pts; ++p) {
        const int32_t* k = &keys[((size_t)f * pts + p) * 3];
        std::tuple<int, int, int> t{k[0], k[1], k[2]};
        if (scene.count(t)) { fs[f].insert(t); all.insert(t); }
      }
    std::set<std::tuple<int, int, int>> used;
    std::vector<char> taken(n_frames, 0);
    int want_picks = 0;
    for (int step = 0; step < max_frames; ++step) {
      int best = -1; size_t best_gain = 0;
      for (int f = 0; f < n_frames; ++f) {
        if (taken[f]) continue;
        size_t g = 0;
        for (auto& t : fs[f]) g += !used.count(t);
        if (best < 0 || g > best_gain) { best = f; best_gain = g; }       // first maximum = lowest frame position
      }
      if (best < 0 || best_gain == 0) break;
      CHECK(want_picks < picks && sel[want_picks] == best && gain[want_picks] == (int64_t)best_gain);
      taken[best] = 1;
      for (auto& t : fs[best]) used.insert(t);
      ++want_picks;
    }
    CHECK(want_picks == picks && n_all == (int64_t)all.size() && n_sel == (int64_t)used.size());
  }
  int32_t k3[3] = {0, 0, 0};
  int64_t g1 = 0, na = 0, ns = 0;
  CHECK(v3d_greedy_cover_host(nullptr, 1, 1, k3, 1, 1, &one, &g1, &na, &ns) == V3D_E_INVALID);
  CHECK(v3d_greedy_cover_host(k3, 0, 1, k3, 1, 1, &one, &g1, &na, &ns) == V3D_E_INVALID);
  CHECK(v3d_greedy_cover_host(k3, 1, 1, k3, 1, 0, &one, &g1, &na, &ns) == V3D_E_INVALID);
  CHECK(v3d_greedy_cover_host(k3, 1, 1, nullptr, 0, 1, &one, &g1, &na, &ns) >= 0);      // an empty scene is legal: nothing to cover
  // a23, num_beams > 1: scripted steps through the beam step's twin (B = 2, K = 4, V = 10, 4 new tokens, EOS id 3, length_penalty 1)
  {
    const int B = 2, K = 4, V = 10, L = 4;
    const int64_t eos[1] = {3};
    const float div[L + 1] = {0.f, 1.f, 2.f, 3.f, 4.f};
    std::vector<int32_t> st(4 + 6 * B + 4 * B * L, 0);
    st[1] = 1;                                                               // improvable
    float* run = reinterpret_cast<float*>(st.data() + 4);
    float* fin = run + B;
    run[0] = 0.f; run[1] = -1e9f; fin[0] = fin[1] = -1e9f;
    const int32_t* fin_len = st.data() + 4 + 3 * B;
    const int32_t* seqs = st.data() + 4 + 6 * B;                             // run_seq[2][B][L], fin_seq[2][B][L]
    const float sc[4][K] = {{-0.5f, -1.0f, -1.5f, -2.0f}, {-0.7f, -0.9f, -1.6f, -1.8f}, {-2.5f, -2.6f, -2.7f, -2.8f}, {-2.6f, -2.7f, -2.9f, -3.0f}};
    const int32_t fl[4][K] = {{4, 3, 7, 1}, {13, 5, 3, 12}, {5, 6, 15, 16}, {1, 12, 2, 13}};
    int64_t next[B] = {-1, -1};
    int32_t par[B] = {-1, -1};
    std::vector<float> ts(L * K, 0.f);
    std::vector<int32_t> tf(L * K, 0);
    auto step = [&](int t) { return v3d_beam_step_host(sc[t], fl[t], K, B, V, L, t, eos, 1, div, st.data(), next, par, ts.data(), tf.data()); };
    CHECK(step(0) == V3D_OK);                                                // rank-1 EOS finishes with -1.0; tokens 4 and 7 run on
    CHECK(st[0] == 0 && st[2] == 1 && next[0] == 4 && next[1] == 7 && par[0] == 0 && par[1] == 0);
    CHECK(run[0] == -0.5f && run[1] == -1.5f && fin[0] == -1.0f && fin[1] == -1e9f && fin_len[0] == 1);
    CHECK(step(1) == V3D_OK);                                                // EOS at rank 0 finishes (-0.7 / 2); the EOS at rank 2 >= B must not
    CHECK(st[0] == 0 && next[0] == 5 && next[1] == 2 && par[0] == 0 && par[1] == 1);
    CHECK(fin[0] == -0.35f && fin[1] == -1.0f && fin_len[0] == 2 && fin_len[1] == 1);
    const int32_t* run2 = seqs + 0 * B * L;                                  // two steps done: buffers 0
    const int32_t* fin2 = seqs + 2 * B * L;
    CHECK(run2[0] == 4 && run2[1] == 5 && run2[L] == 7 && run2[L + 1] == 2 && fin2[0] == 7 && fin2[1] == 3 && fin2[L] == 3);
    CHECK(step(2) == V3D_OK && st[0] == 0 && next[0] == 5 && next[1] == 6 && par[0] == 0 && par[1] == 0 && fin[0] == -0.35f);
    CHECK(step(3) == V3D_OK);                                                // the length limit: every candidate stops, the search ends
    CHECK(st[0] == 1 && st[2] == 4 && fin[0] == -0.35f && fin[1] == -2.6f / 4.f && fin_len[0] == 2 && fin_len[1] == 4);
    const std::vector<int32_t> frozen = st;
    next[0] = 77;
    CHECK(step(3) == V3D_OK && st == frozen && next[0] == 77);               // done: nothing moves any more
    CHECK(tf[3 * K + 1] == 12 && ts[1 * K + 0] == -0.7f);
    CHECK(v3d_beam_step_host(sc[0], fl[0], K, 17, V, L, 0, eos, 1, div, st.data(), next, par, ts.data(), tf.data()) == V3D_E_INVALID);
    CHECK(v3d_beam_step_host(sc[0], fl[0], 1, B, V, L, 0, eos, 1, div, st.data(), next, par, ts.data(), tf.data()) == V3D_E_INVALID);
    CHECK(v3d_beam_step_host(sc[0], fl[0], K, B, V, L, L, eos, 1, div, st.data(), next, par, ts.data(), tf.data()) == V3D_E_INVALID);
    CHECK(v3d_beam_step_host(nullptr, fl[0], K, B, V, L, 0, eos, 1, div, st.data(), next, par, ts.data(), tf.data()) == V3D_E_INVALID);
  }
  // do_sample: Philox known answers, the sampler's twin on a ragged shape, its degenerate forms and its argument check
  {
    const uint32_t c0[4] = {0, 0, 0, 0}, k0[2] = {0, 0}, c1[4] = {~0u, ~0u, ~0u, ~0u}, k1[2] = {~0u, ~0u};
    const uint32_t c2[4] = {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, k2[2] = {0xa4093822u, 0x299f31d0u};
    uint32_t o[4];
    CHECK(v3d_philox4x32_10_host(c0, k0, o) == V3D_OK && o[0] == 0x6627e8d5u && o[1] == 0xe169c58du && o[2] == 0xbc57ac4cu && o[3] == 0x9b00dbd8u);
    CHECK(v3d_philox4x32_10_host(c1, k1, o) == V3D_OK && o[0] == 0x408f276du && o[1] == 0x41c83b0eu && o[2] == 0xa20bc7c6u && o[3] == 0x6d5451fdu);
    CHECK(v3d_philox4x32_10_host(c2, k2, o) == V3D_OK && o[0] == 0xd16cfe09u && o[1] == 0x94fdccebu && o[2] == 0x5001e420u && o[3] == 0x24126ea1u);
    CHECK(v3d_philox4x32_10_host(nullptr, k0, o) == V3D_E_INVALID);
    const int M = 3, V = 37, ldx = 41;
    std::vector<float> x((size_t)M * ldx);
    for (auto& v : x) v = (float)(std::rand() % 17) * 0.25f;                 // many equal values
    std::vector<int64_t> tok(M, -1), top(M, -1);
    std::vector<int32_t> kept(M, -1);
    const int32_t streams[M] = {5, 6, 7};
    for (int step = 0; step < 50; ++step) {
      CHECK(v3d_sample_rows_host(x.data(), ldx, M, V, 0.7f, 5, 0.9f, 1234567890123ull, step, streams, tok.data(), kept.data()) == V3D_OK);
      for (int m = 0; m < M; ++m) CHECK(tok[m] >= 0 && tok[m] < V && kept[m] >= 1 && kept[m] <= 5);
      CHECK(v3d_sample_rows_host(x.data(), ldx, M, V, 1.0f, 0, 1.0f, 7, step, nullptr, tok.data(), kept.data()) == V3D_OK);
      for (int m = 0; m < M; ++m) CHECK(tok[m] >= 0 && tok[m] < V && kept[m] == V);
      CHECK(v3d_sample_rows_host(x.data(), ldx, M, V, 1.0f, 1, 1.0f, 7, step, nullptr, top.data(), nullptr) == V3D_OK);
      CHECK(v3d_sample_rows_host(x.data(), ldx, M, V, 1.0f, 0, 1e-6f, 7, step, nullptr, tok.data(), kept.data()) == V3D_OK);
      for (int m = 0; m < M; ++m) {                                          // both are the first maximum of the row
        int best = 0;
        for (int i = 1; i < V; ++i) if (x[(size_t)m * ldx + i] > x[(size_t)m * ldx + best]) best = i;
        CHECK(top[m] == best && tok[m] == best && kept[m] == 1);
      }
    }
    CHECK(v3d_sample_rows_host(x.data(), ldx, M, V, 0.f, 0, 1.f, 0, 0, nullptr, tok.data(), nullptr) == V3D_E_INVALID);
    CHECK(v3d_sample_rows_host(x.data(), ldx, M, V, 1.f, -1, 1.f, 0, 0, nullptr, tok.data(), nullptr) == V3D_E_INVALID);
    CHECK(v3d_sample_rows_host(x.data(), ldx, M, V, 1.f, 0, 0.f, 0, 0, nullptr, tok.data(), nullptr) == V3D_E_INVALID);
    CHECK(v3d_sample_rows_host(x.data(), ldx, M, V, 1.f, 0, 1.5f, 0, 0, nullptr, tok.data(), nullptr) == V3D_E_INVALID);
    CHECK(v3d_sample_rows_host(x.data(), ldx, 33, V, 1.f, 0, 1.f, 0, 0, nullptr, tok.data(), nullptr) == V3D_E_INVALID);
    CHECK(v3d_sample_rows_host(x.data(), V - 1, M, V, 1.f, 0, 1.f, 0, 0, nullptr, tok.data(), nullptr) == V3D_E_INVALID);
    CHECK(v3d_sample_rows_host(nullptr, ldx, M, V, 1.f, 0, 1.f, 0, 0, nullptr, tok.data(), nullptr) == V3D_E_INVALID);
  }
  // logits processors: the twin on scripted histories (V = 12 of ld 16, two rows at a step stride of 3), every control alone and together, both
  // 16-bit formats, the pad columns, out-of-range ids, and the argument check
  {
    const int M = 2, V = 12, ldx = 16, ld = 3, L = 7;
    //                      row 0: 1 2 3 1 2 9 1   (bigram "1 2" seen twice, unigram 1 three times);  row 1: 5 5 5 77 -4 5 5 (out-of-range ids)
    const int64_t hist[L * ld] = {1, 5, -1, 2, 5, -1, 3, 5, -1, 1, 77, -1, 2, -4, -1, 9, 5, -1, 1, 5, -1};
    const int64_t eos[3] = {0, 11, 400};
    const float ninf = -HUGE_VALF;
    for (int dtype : {V3D_F16, V3D_BF16}) {
      std::vector<float> x0((size_t)M * ldx);
      for (int i = 0; i < M * ldx; ++i) x0[i] = (float)(i % 7) * 0.5f - 1.5f;          // exact in both formats; negatives, zeros, positives
      auto run = [&](std::vector<float>& x, int n_prev, float p, int n, int k, int n_eos) {
        return v3d_logits_process_rows_host(x.data(), ldx, M, V, dtype, hist, ld, n_prev, p, n, k, eos, n_eos);
      };
      std::vector<float> x = x0;
      CHECK(run(x, L, 1.f, 0, 0, 3) == V3D_OK && x == x0);                             // all off: nothing moves
      CHECK(run(x, L, 2.f, 0, 0, 0) == V3D_OK);                                        // penalty 2 (exact): once per distinct id
      for (int m = 0; m < M; ++m)
        for (int v = 0; v < ldx; ++v) {
          const bool seen = m == 0 ? (v == 1 || v == 2 || v == 3 || v == 9) : v == 5;
          const float a = x0[(size_t)m * ldx + v];
          CHECK(x[(size_t)m * ldx + v] == (seen ? (a < 0.f ? a * 2.f : a / 2.f) : a));
        }
      x = x0;
      CHECK(run(x, L, 1.f, 2, 0, 0) == V3D_OK);                                        // bigrams: row 0 ends in 1 -> 2 banned; row 1 ends in 5 -> 5 and 77 (skipped)
      for (int m = 0; m < M; ++m)
        for (int v = 0; v < ldx; ++v) CHECK(x[(size_t)m * ldx + v] == ((m == 0 && v == 2) || (m == 1 && v == 5) ? ninf : x0[(size_t)m * ldx + v]));
      x = x0;
      CHECK(run(x, L, 1.f, 3, 0, 0) == V3D_OK);                                        // trigrams: row 0 ends in "9 1" (new) -> none; row 1 ends in "5 5" -> 5
      for (int m = 0; m < M; ++m)
        for (int v = 0; v < ldx; ++v) CHECK(x[(size_t)m * ldx + v] == ((m == 1 && v == 5) ? ninf : x0[(size_t)m * ldx + v]));
      x = x0;
      CHECK(run(x, 1, 1.f, 3, 0, 0) == V3D_OK && x == x0);                             // L + 1 < n
      CHECK(run(x, L, 1.f, 0, L + 1, 3) == V3D_OK);                                    // L < k: EOS ids 0 and 11 (400 is out of range)
      for (int m = 0; m < M; ++m)
        for (int v = 0; v < ldx; ++v) CHECK(x[(size_t)m * ldx + v] == (v == 0 || v == 11 ? ninf : x0[(size_t)m * ldx + v]));
      x = x0;
      CHECK(run(x, L, 1.f, 0, L, 3) == V3D_OK && x == x0);                             // L == k: off
      CHECK(run(x, L, 1.3f, 1, L + 1, 3) == V3D_OK);                                   // all three: the bans win over the penalty
      CHECK(x[1] == ninf && x[2] == ninf && x[3] == ninf && x[9] == ninf && x[0] == ninf && x[11] == ninf && x[4] == x0[4] && x[12] == x0[12]);
      CHECK(x[ldx + 5] == ninf && x[ldx + 0] == ninf && x[ldx + 6] == x0[ldx + 6] && x[ldx + 13] == x0[ldx + 13]);
      x = x0;
      CHECK(run(x, 0, 1.3f, 2, 0, 0) == V3D_OK && x == x0);                            // an empty history
      CHECK(v3d_logits_process_rows_host(x.data(), ldx, M, V, dtype, nullptr, ld, 0, 1.3f, 2, 0, nullptr, 0) == V3D_OK && x == x0);
      CHECK(run(x, L, 0.f, 0, 0, 0) == V3D_E_INVALID && run(x, L, -1.f, 0, 0, 0) == V3D_E_INVALID && run(x, L, 1.f, -1, 0, 0) == V3D_E_INVALID);
      CHECK(run(x, L, 1.f, 0, -1, 0) == V3D_E_INVALID && run(x, -1, 1.f, 0, 0, 0) == V3D_E_INVALID && run(x, 8193, 1.f, 0, 0, 0) == V3D_E_INVALID);
      CHECK(std::strstr(v3d_last_error(), "LOGITS_MAX_HISTORY") != nullptr);
      CHECK(v3d_logits_process_rows_host(x.data(), ldx, 33, V, dtype, hist, 33, L, 1.f, 0, 0, eos, 3) == V3D_E_INVALID);
      CHECK(v3d_logits_process_rows_host(x.data(), V - 1, M, V, dtype, hist, ld, L, 1.f, 0, 0, eos, 3) == V3D_E_INVALID);
      CHECK(v3d_logits_process_rows_host(x.data(), ldx, M, V, dtype, hist, 1, L, 1.f, 0, 0, eos, 3) == V3D_E_INVALID);       // ld_step < M
      CHECK(v3d_logits_process_rows_host(x.data(), ldx, M, V, V3D_F32, hist, ld, L, 1.f, 0, 0, eos, 3) == V3D_E_INVALID);
      CHECK(v3d_logits_process_rows_host(nullptr, ldx, M, V, dtype, hist, ld, L, 1.f, 0, 0, eos, 3) == V3D_E_INVALID);
      CHECK(v3d_logits_process_rows_host(x.data(), ldx, M, V, dtype, nullptr, ld, L, 1.f, 0, 0, eos, 3) == V3D_E_INVALID);
      CHECK(v3d_logits_process_rows_host(x.data(), ldx, M, V, dtype, hist, ld, L, 1.f, 0, 1, nullptr, 3) == V3D_E_INVALID);
    }
  }
  // the GEMM planner (gemm_plan.h): the plans of the path's shapes on a 256-CU chip, then a sweep that holds every split-K plan to
  // what the kernel needs - the item list is rebuilt the way gemm256pp_kernel walks it (XCD-major id g = xcd * wx + idx, item
  // g = (chunk g / T, tile g mod T)): each K-chunk has a workgroup, each chunk-0 workgroup finds its partners by the kernel's formula
  {
    struct P { int kernel, tiles, dp, split; };
    auto plan = [](int M, int N, int K, int slots, P* p) { return v3d_gemm_plan_host(M, N, K, slots, &p->kernel, &p->tiles, &p->dp, &p->split); };
    auto is = [](const P& p, int k, int t, int d, int s) { return p.kernel == k && p.tiles == t && p.dp == d && p.split == s; };
    P p;
    CHECK(plan(6794, 37888, 3584, 256, &p) == V3D_OK && is(p, 2, 27 * 148, -1, 1));
    CHECK(plan(6794, 4608, 3584, 256, &p) == V3D_OK && is(p, 2, 27 * 18, -1, 1));
    CHECK(plan(6794, 3584, 3584, 256, &p) == V3D_OK && p.kernel == 3);
    CHECK(plan(6794, 3584, 18944, 256, &p) == V3D_OK && is(p, 2, 378, 1, 2));
    CHECK(plan(960, 3584, 18944, 256, &p) == V3D_OK && is(p, 2, 56, 0, 4));
    CHECK(plan(960, 4608, 3584, 256, &p) == V3D_OK && p.kernel == 1);
    CHECK(plan(4, 3584, 3584, 256, &p) == V3D_OK && p.kernel == 0);          // skinny (decode) path
    CHECK(plan(23328, 1152, 1152, 256, &p) == V3D_OK && p.kernel == 1);      // N % 256 != 0: only the 128 x 128 tile fits
    CHECK(plan(16, 100, 64, 256, &p) == V3D_E_INVALID && std::strstr(v3d_last_error(), "bad shape") != nullptr);
    CHECK(plan(16, 128, 64, 0, &p) == V3D_E_INVALID);
    CHECK(v3d_gemm_plan_host(16, 128, 64, 256, nullptr, &p.tiles, &p.dp, &p.split) == V3D_E_INVALID && std::strstr(v3d_last_error(), "null pointer") != nullptr);
    const int chips[6] = {8, 16, 64, 104, 256, 304};
    int seen = 0;
    for (int it = 0; it < 4000; ++it) {
      const int M = 9 + std::rand() % 29991, N = 256 * (1 + std::rand() % 159), K = 64 * (1 + std::rand() % 319), slots = chips[std::rand() % 6];
      CHECK(plan(M, N, K, slots, &p) == V3D_OK && p.kernel >= 1 && p.kernel <= 3);
      if (p.dp < 0) { CHECK(p.split == 1); continue; }
      ++seen;
      const int grid = slots & ~7, nt = K / 64, T = p.tiles - p.dp * grid, split = p.split, wx = grid / 8, gpt = nt / 2;
      CHECK(p.kernel == 2 && p.tiles == ((M + 255) / 256) * (N / 256));
      CHECK(split >= 2 && split <= 4 && T > 0 && T * split <= grid);         // no chunk without a workgroup
      CHECK(nt % 2 == 0 && gpt >= 2 * split);                                // no chunk shorter than two granules
      std::vector<int> owner((size_t)split * T, -1);                         // [chunk][tile] -> workgroup
      for (int b = 0; b < grid; ++b) {
        const int g = (b & 7) * wx + (b >> 3);
        if (g < split * T) { CHECK(owner[(size_t)g] == -1); owner[(size_t)g] = b; }
      }
      for (int j = 0; j < T; ++j) {
        const int b0 = owner[(size_t)j];
        CHECK(b0 >= 0);
        const int g0 = (b0 & 7) * wx + (b0 >> 3);
        for (int c = 1; c < split; ++c) {
          const int fg = c * T + g0, partner = (fg % wx) * 8 + fg / wx;      // the kernel's partner formula
          CHECK(partner < grid && partner == owner[(size_t)c * T + j]);
        }
      }
      for (int c = 0; c < split; ++c) CHECK(2 * ((c + 1) * gpt / split) - 2 * (c * gpt / split) >= 2);
      CHECK(2 * (split * gpt / split) == nt);
    }
    CHECK(seen > 50);
  }
  std::puts("host_selftest ok");
  return 0;
}
