// The 16-bit GEMM's planner (gemm.hip): which tile form a shape takes, and whether the ping-pong kernel ends in a split-K tail.
// Pure host arithmetic, no HIP types: gemm.hip plans its launches with it, host.cpp exports it (v3d_gemm_plan_host), and the
// sanitizer self-test walks its plans without a GPU.
#pragma once

namespace v3d {

constexpr int BM = 128, BN = 128, BK = 64;              // the 128 x 128 tile, the K-step of every tile form
constexpr int B3N = 256;                                // the width of the 256- and 192-row tiles

// Tile choice (speed only), from a time model fitted on MI355X to the path's shapes (tools/time_gemm_ab.py; microseconds):
//   a kernel takes  rounds x (fixed + K-steps x per-step),  rounds = ceil(tiles / workgroup slots of the chip)
//   256 x 256 ping-pong (256 slots): fixed 8 (epilogue, rendezvous, first DMA latency; 13 with SwiGLU), 1.26 per K-step
//   192 x 256 ping-pong (256 slots): fixed 4.5, 1.22 per K-step   (3/4 of the tile at the same step time: it only wins where
//                                    256-row tiles quantise badly against the 256 CUs, e.g. M = 6794, N = 3584, K = 3584)
//   128 x 128           (512 slots): fixed 1, 0.98 per K-step     (many small tiles: small M, or N % 256 != 0)
//   256 x 256 with the split-K tail: whole rounds as above (a launch of their own) + 5 for the second launch + one round of
//                                    (22 + step x K-steps / split + 40 for the exchange),
//                                    step 1.3 when the launch is only the tail, 1.7 behind whole rounds (measured: 6794 x 3584 x 18944
//                                    780 -> 685 us, 960 x 3584 x 18944 330 -> 152 us; no gain at K = 3584)
struct KernelCost { double fixed, per_step; int slots; };
constexpr KernelCost COST_PP256 = {8.0, 1.263, 256}, COST_PP192 = {4.5, 1.2225, 256};      // ping-pong
constexpr KernelCost COST_V3_256 = {9.0, 1.36, 256}, COST_V3_192 = {2.0, 1.32, 256};       // v3 (and the layout kernel's 256-wide form)
constexpr KernelCost COST_128 = {1.0, 0.98, 512};
constexpr int LAST_ROUND_SLACK_128 = 25;                // 128 x 128: a last round under 5 % full is not felt
constexpr double SK_SECOND_LAUNCH = 5.0, SK_TAIL_FIXED = 22.0, SK_EXCHANGE = 40.0;
constexpr double SK_STEP_ALONE = 1.3, SK_STEP_BEHIND_ROUNDS = 1.7;

inline int gemm_rounds(int tiles, int slots, int slack = 0) {
  const int r = (tiles + slots - 1 - slack) / slots;
  return r > 0 ? r : 1;
}
inline double kernel_time(int tiles, const KernelCost& c, double ks, int slack = 0) {
  return (double)gemm_rounds(tiles, c.slots, slack) * (c.fixed + c.per_step * ks);
}
// dp whole rounds of the 256 x 256 ping-pong kernel, then the rest of the tiles cut into sp K-chunks
inline double sk_time(int dp, int sp, double ks) {
  return dp * (COST_PP256.fixed + COST_PP256.per_step * ks) + (dp > 0 ? SK_SECOND_LAUNCH : 0.0) + SK_TAIL_FIXED +
         (dp > 0 ? SK_STEP_BEHIND_ROUNDS : SK_STEP_ALONE) * ks / sp + SK_EXCHANGE;
}

// ---- split-K tail of the ping-pong kernel ----
// Legal: grid a multiple of 8 (the XCD-major order), an even number of K-steps (granule = 2) with at least two granules per chunk,
// and the tiles left after the whole-tile rounds fit the grid at least twice.  Returns the whole-tile rounds (or -1) and the split.
inline int sk_plan(int n_tiles, int grid, int nt, int* split) {
  *split = 1;
  if (grid < 8 || (grid & 7) || (nt & 1)) return -1;
  const int dp = n_tiles / grid, rest = n_tiles - dp * grid;      // (dp = 0: fewer tiles than workgroups - the whole launch is the tail)
  if (rest == 0) return -1;                  // whole rounds only
  int sp = grid / rest;
  sp = sp > 4 ? 4 : sp;
  if (sp < 2 || (nt >> 1) < 2 * sp) return -1;
  *split = sp;
  return dp;
}
// a forced tile decides for itself: whole rounds on `grid` workgroups vs whole rounds + split tail (no margin, no other tile forms)
inline bool sk_pays(int n_tiles, int grid, int nt) {
  int sp = 1;
  const int dp = sk_plan(n_tiles, grid, nt, &sp);
  if (dp < 0) return false;
  const double ks = (double)nt;
  return sk_time(dp, sp, ks) < (double)gemm_rounds(n_tiles, grid) * (COST_PP256.fixed + COST_PP256.per_step * ks);
}

struct GemmPlan { int kernel; int sk; int dp; int split; int tiles; };    // kernel: 1 = 128 x 128, 2 = 256 x 256, 3 = 192 x 256 (2, 3: ping-pong or v3)
inline GemmPlan gemm_plan(int M, int N, int K, int slots, int var, bool pp_on, int sk_mode) {
  GemmPlan g = {1, 0, -1, 1, ((M + BM - 1) / BM) * (N / BN)};
  if (N % B3N != 0 || var == 1) return g;
  const double ks = (double)(K / BK);
  const int tiles256 = ((M + 255) / 256) * (N / B3N), tiles192 = ((M + 191) / 192) * (N / B3N);
  const bool pp = pp_on && K >= 2 * BK;
  double t256 = kernel_time(tiles256, pp ? COST_PP256 : COST_V3_256, ks);
  const double t192 = kernel_time(tiles192, pp ? COST_PP192 : COST_V3_192, ks);
  const double t1 = kernel_time(g.tiles, COST_128, ks, LAST_ROUND_SLACK_128);
  int sk_use = 0, sp = 1, dp = -1;
  if (pp && sk_mode != 0) {
    dp = sk_plan(tiles256, slots & ~7, K / BK, &sp);
    if (dp >= 0) {
      const double tsk = sk_time(dp, sp, ks);
      const double best = t256 < t192 ? (t256 < t1 ? t256 : t1) : (t192 < t1 ? t192 : t1);
      if (tsk < 0.98 * best || sk_mode == 2) { t256 = tsk < t256 ? tsk : t256; sk_use = 1; }    // (a 2 % margin: the model is coarse)
    }
  }
  if (var == 4) { g.kernel = 3; g.tiles = tiles192; g.sk = -1; return g; }       // forced tiles decide the split themselves (sk = -1)
  if (var == 3) { g.kernel = 2; g.tiles = tiles256; g.sk = -1; return g; }
  if (t192 < t256 && t192 < t1) { g.kernel = 3; g.tiles = tiles192; return g; }
  if (t256 < t1) { g.kernel = 2; g.tiles = tiles256; g.sk = sk_use; if (sk_use) { g.dp = dp; g.split = sp; } return g; }
  return g;
}

// v3d_gemm_layout's tile form: the 128 x 128 kernel against the 256 x 256 v3 kernel (the schedule its 256-wide form shares)
inline bool gemm_layout_big(int M, int N, int K) {
  if (N % B3N != 0) return false;
  const double ks = (double)((K + BK - 1) / BK);
  const int tiles256 = ((M + 255) / 256) * (N / B3N), tiles128 = ((M + BM - 1) / BM) * (N / BN);
  return kernel_time(tiles256, COST_V3_256, ks) < kernel_time(tiles128, COST_128, ks, LAST_ROUND_SLACK_128);
}

}  // namespace v3d
