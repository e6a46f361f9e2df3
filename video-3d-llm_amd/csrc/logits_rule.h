// The logits processors' rule ("Logits processors, stated once"): the parts shared by the kernel of logits.hip and
// the host twin v3d_logits_process_rows_host (host.cpp).  Plain C++ and integer conversions only, so both sides produce the same bits.
//
// Row m at step L has the history h[0..L) = history[j * ld_step + m] (the tokens generated so far).  In this order:
//   repetition_penalty p   every distinct id v of h: x[v] = round16(x[v] < 0 ? x[v] * p : x[v] / p), from the unpenalised x[v], once;
//   no_repeat_ngram_size n if L + 1 >= n: every i in [0, L - n] with h[i .. i+n-1) == h[L-n+1 .. L) bans h[i+n-1] (x = -inf);
//   min_new_tokens k       while L < k every EOS id is banned.
// Ids outside [0, V) are skipped.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define V3D_HD __host__ __device__
#else
#define V3D_HD
#endif

namespace v3d {

constexpr int LOGITS_MAX_M = 32;
constexpr int LOGITS_MAX_HISTORY = 8192;           // the engine's max_pos; the kernel stages one 16-bit value per history entry in LDS

V3D_HD inline uint32_t logits_f32_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
V3D_HD inline float logits_bits_f32(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// 16-bit storage <-> f32, round to nearest even (bf16: is_bf16, else IEEE half)
V3D_HD inline float logits_widen(uint16_t h, bool is_bf16) {
  if (is_bf16) return logits_bits_f32((uint32_t)h << 16);
  const uint32_t sign = ((uint32_t)h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
  if (e == 31u) return logits_bits_f32(sign | 0x7f800000u | (m << 13));
  if (e == 0u) {                                                             // zero or subnormal: m * 2^-24, exact
    const float v = (float)m * 5.9604644775390625e-08f;
    return logits_bits_f32(logits_f32_bits(v) | sign);
  }
  return logits_bits_f32(sign | ((e + 112u) << 23) | (m << 13));
}

V3D_HD inline uint16_t logits_round16(float f, bool is_bf16) {
  const uint32_t w = logits_f32_bits(f);
  const uint32_t sign = (w >> 16) & 0x8000u, u = w & 0x7fffffffu;
  if (is_bf16) {
    if (u > 0x7f800000u) return (uint16_t)(sign | 0x7fc0u);
    return (uint16_t)((w + 0x7fffu + ((w >> 16) & 1u)) >> 16);
  }
  if (u > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
  if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                   // 65520 and above (and inf) round to inf
  if (u < 0x38800000u) {                                                     // below 2^-14: a subnormal half, q * 2^-24
    if (u <= 0x33000000u) return (uint16_t)sign;                             // up to 2^-25 (the tie goes to the even 0)
    const uint32_t shift = 126u - (u >> 23);                                 // 14 .. 24
    const uint32_t m = (u & 0x7fffffu) | 0x800000u;
    uint32_t q = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (q & 1u))) ++q;
    return (uint16_t)(sign | q);
  }
  const uint32_t r = u + 0xfffu + ((u >> 13) & 1u);
  return (uint16_t)(sign | ((r - 0x38000000u) >> 13));
}

// RepetitionPenaltyLogitsProcessor on one entry: f32 from the 16-bit logit, an IEEE multiplication or division, one rounding
V3D_HD inline uint16_t logits_penalised(uint16_t x, float p, bool is_bf16) {
  const float v = logits_widen(x, is_bf16);
  return logits_round16(v < 0.f ? v * p : v / p, is_bf16);
}

V3D_HD inline uint16_t logits_neg_inf(bool is_bf16) { return is_bf16 ? (uint16_t)0xff80u : (uint16_t)0xfc00u; }

V3D_HD inline bool logits_id_ok(int64_t v, int V) { return v >= 0 && v < (int64_t)V; }

// NoRepeatNGramLogitsProcessor: does the (n-1)-gram at i equal the last n-1 tokens?  (h strided by ld; n >= 1, 0 <= i <= L - n)
V3D_HD inline bool logits_ngram_match(const int64_t* h, int64_t ld, int L, int n, int i) {
  for (int j = 0; j < n - 1; ++j)
    if (h[(int64_t)(i + j) * ld] != h[(int64_t)(L - n + 1 + j) * ld]) return false;
  return true;
}

V3D_HD inline bool logits_args_ok(int M, int V, int64_t ld_step, int n_prev, float p, int ngram, int min_new, int n_eos) {
  return M >= 1 && M <= LOGITS_MAX_M && V >= 1 && ld_step >= M && n_prev >= 0 && n_prev <= LOGITS_MAX_HISTORY && p > 0.f &&
         p <= 3.4028234663852886e38f && ngram >= 0 && min_new >= 0 && n_eos >= 0;      // (a NaN fails every comparison)
}

}  // namespace v3d
