// Logits processors on the device: repetition_penalty, no_repeat_ngram_size, min_new_tokens, applied in place to the rows the token
// choice (v3d_argmax / v3d_argmax_rows / v3d_sample_rows) reads next.  The rule is DESIGN section 2, "Logits processors, stated once";
// its shared parts are logits_rule.h.
//
// One launch per decode step, one workgroup per row.  The work follows the history (L entries), never the row (V columns):
//   penalty  thread t owns history positions t, t + 256, ...: it gathers x[h[j]], penalises and rounds it, and stages the 16-bit result
//            in LDS slot j.  After a barrier - every gather of the row is done - the same thread stores slot j to x[h[j]].  An id that
//            occurs at several positions is read unpenalised at each of them, so all its writers store the same bits: penalised once.
//   n-gram   after a second barrier (a ban must land behind the penalty's store to the same entry) thread t tests the windows
//            i = t, t + 256, ... against the last n - 1 tokens and stores -inf to x[h[i + n - 1]] on a match.
//   EOS      while L < min_new, thread t stores -inf to x[eos[t]], x[eos[t + 256]], ...
// Plain 2-byte vector stores, no atomics; ids outside [0, V) are skipped, so nothing outside the row's V columns is written.
#include "v3d_common.h"
#include "logits_rule.h"

namespace v3d {

constexpr int LP_THREADS = 256;

template <bool BF16>
__global__ __launch_bounds__(LP_THREADS) void logits_process_kernel(uint16_t* __restrict__ x, int64_t ldx, int V, const int64_t* __restrict__ history,
                                                                    int64_t ld_step, int L, float penalty, int ngram, int min_new,
                                                                    const int64_t* __restrict__ eos_ids, int n_eos) {
  __shared__ uint16_t s_val[LOGITS_MAX_HISTORY];
  uint16_t* row = x + (int64_t)blockIdx.x * ldx;
  const int64_t* h = history + blockIdx.x;
  const int t = threadIdx.x;
  if (penalty != 1.f) {
    for (int j = t; j < L; j += LP_THREADS) {
      const int64_t v = h[(int64_t)j * ld_step];
      if (logits_id_ok(v, V)) s_val[j] = logits_penalised(row[v], penalty, BF16);
    }
    __syncthreads();
    for (int j = t; j < L; j += LP_THREADS) {
      const int64_t v = h[(int64_t)j * ld_step];
      if (logits_id_ok(v, V)) row[v] = s_val[j];
    }
    __syncthreads();
  }
  const uint16_t ninf = logits_neg_inf(BF16);
  if (ngram > 0 && L + 1 >= ngram) {
    for (int i = t; i <= L - ngram; i += LP_THREADS) {
      if (logits_ngram_match(h, ld_step, L, ngram, i)) {
        const int64_t v = h[(int64_t)(i + ngram - 1) * ld_step];
        if (logits_id_ok(v, V)) row[v] = ninf;
      }
    }
  }
  if (L < min_new) {
    for (int e = t; e < n_eos; e += LP_THREADS) {
      const int64_t v = eos_ids[e];
      if (logits_id_ok(v, V)) row[v] = ninf;
    }
  }
}

}  // namespace v3d

using namespace v3d;

extern "C" int v3d_logits_process_rows(void* logits, int64_t ldx, int M, int V, int dtype, const int64_t* history, int64_t ld_step, int n_prev,
                                       float penalty, int ngram, int min_new, const int64_t* eos_ids, int n_eos, void* stream) {
  V3D_REQUIRE(logits, "v3d_logits_process_rows: null pointer");
  V3D_REQUIRE(n_prev <= LOGITS_MAX_HISTORY, "v3d_logits_process_rows: a history of %d tokens exceeds LOGITS_MAX_HISTORY = %d", n_prev, LOGITS_MAX_HISTORY);
  V3D_REQUIRE(logits_args_ok(M, V, ld_step, n_prev, penalty, ngram, min_new, n_eos),
              "v3d_logits_process_rows: needs 1 <= M <= %d rows, V >= 1, ld_step >= M, n_prev >= 0, a finite penalty > 0, ngram >= 0, min_new >= 0, "
              "n_eos >= 0 (M=%d V=%d ld_step=%lld n_prev=%d penalty=%g ngram=%d min_new=%d n_eos=%d)",
              LOGITS_MAX_M, M, V, (long long)ld_step, n_prev, (double)penalty, ngram, min_new, n_eos);
  V3D_REQUIRE(dtype == V3D_F16 || dtype == V3D_BF16, "v3d_logits_process_rows: 16-bit logits only");
  V3D_REQUIRE(M == 1 || ldx >= V, "v3d_logits_process_rows: ldx < V");
  V3D_REQUIRE(history || n_prev == 0, "v3d_logits_process_rows: null history with n_prev > 0");
  V3D_REQUIRE(eos_ids || n_eos == 0, "v3d_logits_process_rows: null eos_ids with n_eos > 0");
  const bool any = (penalty != 1.f && n_prev > 0) || (ngram > 0 && n_prev >= ngram) ||      // (at least one window i in [0, L - n])
 (n_prev < min_new && n_eos > 0);
  if (!any) return V3D_OK;                                                   // nothing of the rule touches this step
  hipStream_t st = (hipStream_t)stream;
  if (dtype == V3D_BF16)
    hipLaunchKernelGGL(logits_process_kernel<true>, dim3(M), dim3(LP_THREADS), 0, st, (uint16_t*)logits, ldx, V, history, ld_step, n_prev, penalty, ngram,
                       min_new, eos_ids, n_eos);
  else
    hipLaunchKernelGGL(logits_process_kernel<false>, dim3(M), dim3(LP_THREADS), 0, st, (uint16_t*)logits, ldx, V, history, ld_step, n_prev, penalty, ngram,
                       min_new, eos_ids, n_eos);
  return check_launch("v3d_logits_process_rows");
}
