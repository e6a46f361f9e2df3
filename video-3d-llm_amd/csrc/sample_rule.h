// The sampling rule ("Sampling, stated once"): the parts shared by the kernels of sample.hip and the host twin
// v3d_sample_rows_host (host.cpp).  Plain C++; the integer parts (Philox words, the 24-bit uniform, the argument check) are the
// same bits on both sides, the key goes through each side's own logf / log1pf.
//
// Token i of a row (seed, step, stream) owns word i & 3 of Philox4x32-10 at counter (i >> 2, step, stream, 0), key (seed low word,
// seed high word).  n = w >> 8, u = (n + 0.5) * 2^-24 lies strictly inside (0, 1), g = -log(-log(u)), key = x / T + g; the token
// drawn is the kept one with the largest key (the lower index on equal keys): Gumbel-max, an exact draw from softmax(x / T) over
// the kept set up to the 2^-24 grid of u.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define V3D_HD __host__ __device__
#else
#define V3D_HD
#endif

namespace v3d {

constexpr int SAMPLE_MAX_M = 32;

struct Philox4 { uint32_t w[4]; };

V3D_HD inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  Philox4 o;
  o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
  return o;
}

// the four words of the tokens 4 * group .. 4 * group + 3
V3D_HD inline Philox4 sample_words(uint32_t group, uint32_t step, uint32_t stream, uint64_t seed) {
  return philox4x32_10(group, step, stream, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

V3D_HD inline uint32_t sample_u24(uint32_t w) { return w >> 8; }

// g = -log(-log(u)), u = (n + 0.5) * 2^-24.  n + 0.5 needs 25 bits once n >= 2^23, so the upper half goes through
// 1 - u = (2^24 - n - 0.5) * 2^-24, which is exact in f32 there, and log1p.
V3D_HD inline float sample_gumbel(uint32_t n) {
  float a;
  if (n < (1u << 23)) a = -logf(((float)n + 0.5f) * 5.9604644775390625e-08f);
  else a = -log1pf(-(((float)((1u << 24) - n) - 0.5f) * 5.9604644775390625e-08f));
  return -logf(a);
}

V3D_HD inline float sample_scaled(float x, float T) { return x / T; }                    // an IEEE division
V3D_HD inline float sample_key(float x, float T, uint32_t w) { return sample_scaled(x, T) + sample_gumbel(sample_u24(w)); }

// top_k as the rule uses it: 0 (off) and anything above V keep all V
V3D_HD inline int sample_top_k(int top_k, int V) { return (top_k <= 0 || top_k > V) ? V : top_k; }

V3D_HD inline bool sample_args_ok(int M, int V, float T, int top_k, float top_p) {
  return M >= 1 && M <= SAMPLE_MAX_M && V >= 1 && (int64_t)M * V < (1ll << 31) && T > 0.f && T <= 3.4028234663852886e38f && top_k >= 0 &&
         top_p > 0.f && top_p <= 1.f;                                                     // (a NaN fails every comparison)
}

}  // namespace v3d
