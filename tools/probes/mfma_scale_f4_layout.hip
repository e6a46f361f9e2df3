// Lane layout of v_mfma_scale_f32_16x16x128_f8f6f4 with an fp4 (e2m1) first operand and an fp8 (e4m3) second operand, of its
// block-scale register, and the nibble / byte_sel order of v_cvt_scalef32_pk_{bf16,f16}_fp4.  Build and run on a gfx950:
//   hipcc --offload-arch=gfx950 -O2 mfma_scale_f4_layout.hip -o mfma_scale_f4_layout && ./mfma_scale_f4_layout
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <string.h>
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));
// A: fp4, 16 bytes per lane in registers 0..3 (registers 4..7 are filled with 0xff to show that they are ignored); B: fp8, 32 bytes.
template <int OPSEL>
__global__ void k(const uint8_t* A, const uint8_t* B, float* D, const int* scale_a) {
  const int l = threadIdx.x;
  v8i a, b;
  for (int i = 0; i < 4; ++i) a[i] = ((const int*)A)[l * 4 + i];
  for (int i = 4; i < 8; ++i) a[i] = -1;
  for (int i = 0; i < 8; ++i) b[i] = ((const int*)B)[l * 8 + i];
  v4f c = {0, 0, 0, 0};
  c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 4, 0, OPSEL, scale_a[l], 0, 127);
  for (int i = 0; i < 4; ++i) D[l * 4 + i] = c[i];
}
__global__ void cvt(const uint32_t* src, const uint32_t* scale_bits, float* out) {   // out[case][sel][bf16 lo, hi, f16 lo, hi]
  typedef __bf16 b2 __attribute__((ext_vector_type(2)));
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  const int c = threadIdx.x;
  const float sc = __uint_as_float(scale_bits[c]);
  b2 p; h2 q;
#define ONE(S) p = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(src[c], sc, S); q = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(src[c], sc, S); \
  out[(c * 4 + S) * 4 + 0] = (float)p[0]; out[(c * 4 + S) * 4 + 1] = (float)p[1]; out[(c * 4 + S) * 4 + 2] = (float)q[0]; out[(c * 4 + S) * 4 + 3] = (float)q[1];
  ONE(0) ONE(1) ONE(2) ONE(3)
#undef ONE
}
static uint8_t hA[64 * 16], hB[64 * 32]; static float hD[256]; static int hS[64];
static uint8_t *dA, *dB; static float* dD; static int* dS;
static void set_nibble(int lane, int idx, int code) { uint8_t& b = hA[lane * 16 + idx / 2]; b = (idx & 1) ? (uint8_t)((b & 0x0f) | (code << 4)) : (uint8_t)((b & 0xf0) | code); }
template <int OPSEL> static void run() {
  hipMemcpy(dA, hA, sizeof hA, hipMemcpyHostToDevice); hipMemcpy(dB, hB, sizeof hB, hipMemcpyHostToDevice);
  hipMemcpy(dS, hS, sizeof hS, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(k<OPSEL>, dim3(1), dim3(64), 0, 0, dA, dB, dD, dS);
  hipMemcpy(hD, dD, sizeof hD, hipMemcpyDeviceToHost);
}
int main() {
  // e2m1 codes: 0 0, 1 0.5, 2 1, 3 1.5, 4 2, 5 3, 6 4, 7 6 (+8: negative); e4m3 1.0 = 0x38
  hipMalloc(&dA, sizeof hA); hipMalloc(&dB, sizeof hB); hipMalloc(&dD, sizeof hD); hipMalloc(&dS, sizeof hS);
  for (int i = 0; i < 64; ++i) hS[i] = 127;
  // 1: every code against ones -> 128 * value
  for (int code = 0; code < 16; ++code) {
    memset(hA, code * 0x11, sizeof hA); memset(hB, 0x38, sizeof hB);
    run<0>();
    printf("code %2d: D[0]=%g D[255]=%g  (/128 = %g)\n", code, hD[0], hD[255], hD[0] / 128);
  }
  // 2: row mapping of A: one-hot (lane, nibble 5) against ones
  for (int la : {0, 1, 15, 16, 17, 33, 63}) {
    memset(hA, 0, sizeof hA); memset(hB, 0x38, sizeof hB);
    set_nibble(la, 5, 2);
    run<0>();
    printf("A one-hot lane %d nibble 5 -> nonzero D (lane,reg):", la);
    int n = 0; for (int i = 0; i < 256; ++i) if (hD[i] != 0 && n++ < 4) printf(" (%d,%d)=%g", i / 4, i % 4, hD[i]);
    printf("  [%d nonzero]\n", n);
  }
  // 3: k mapping: A(lane, nibble index) pairs with which B(lane, byte)
  for (int na : {0, 1, 2, 15, 16, 31}) for (int la : {0, 16, 32, 48}) {
    memset(hA, 0, sizeof hA); set_nibble(la, na, 2);
    int found_lb = -1, found_bb = -1, cnt = 0;
    for (int lb = 0; lb < 64; lb += 16) for (int bb = 0; bb < 32; ++bb) {
      memset(hB, 0, sizeof hB); hB[lb * 32 + bb] = 0x38;
      run<0>();
      for (int i = 0; i < 256; ++i) if (hD[i] != 0) { found_lb = lb; found_bb = bb; ++cnt; }
    }
    printf("A(lane %d, nibble %d) pairs with B(lane %d, byte %d) [%d hits]\n", la, na, found_lb, found_bb, cnt);
  }
  // 4: scale register of A: ones against ones = 128 when every scale is 2^0
  memset(hA, 0x22, sizeof hA); memset(hB, 0x38, sizeof hB);
  for (int i = 0; i < 64; ++i) hS[i] = 127 + (i >> 4);
  run<0>();
  printf("scale 127 + (lane>>4): D[0]=%g D[5]=%g D[255]=%g  (per-lane k block: 32*(1+2+4+8) = 480)\n", hD[0], hD[5], hD[255]);
  for (int i = 0; i < 64; ++i) hS[i] = 127 + (i & 15) % 3;
  run<0>();
  printf("scale 127 + (lane&15)%%3: D rows (lane>>4)*4+reg at column 0:");
  for (int row = 0; row < 16; ++row) printf(" %g", hD[((row >> 2) * 16) * 4 + (row & 3)]);
  printf("\n");
  for (int i = 0; i < 64; ++i) hS[i] = (i == 17) ? 130 : 127;
  run<0>();
  printf("scale 130 in lane 17 only: nonzero deviations from 128:");
  { int n = 0; for (int i = 0; i < 256; ++i) if (hD[i] != 128 && n++ < 6) printf(" (%d,%d)=%g", i / 4, i % 4, hD[i]); printf("  [%d]\n", n); }
  for (int i = 0; i < 64; ++i) hS[i] = 127 | (128 << 8) | (129 << 16) | (130 << 24);
  run<0>(); printf("scale bytes {127,128,129,130}: opsel 0 -> %g", hD[0]);
  run<1>(); printf(", 1 -> %g", hD[0]);
  run<2>(); printf(", 2 -> %g", hD[0]);
  run<3>(); printf(", 3 -> %g\n", hD[0]);
  for (int e : {0, 1, 254}) {
    for (int i = 0; i < 64; ++i) hS[i] = e;
    run<0>(); printf("scale byte %d: D[0]=%g (128 * 2^%d)\n", e, hD[0], e - 127);
  }
  // 5: v_cvt_scalef32_pk_{bf16,f16}_fp4
  uint32_t hsrc[8] = {0x76543210u, 0xfedcba98u, 0x76543210u, 0x76543210u, 0x76543210u, 0x76543210u, 0x76543210u, 0x76543210u};
  uint32_t hsc[8] = {127u << 23, 127u << 23, 129u << 23, 120u << 23, 0u, 1u << 23, 254u << 23, (127u << 23) | 0x400000u};
  uint32_t *dsrc, *dsc; float *dout, hout[8 * 16];
  hipMalloc(&dsrc, sizeof hsrc); hipMalloc(&dsc, sizeof hsc); hipMalloc(&dout, sizeof hout);
  hipMemcpy(dsrc, hsrc, sizeof hsrc, hipMemcpyHostToDevice); hipMemcpy(dsc, hsc, sizeof hsc, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(cvt, dim3(1), dim3(8), 0, 0, dsrc, dsc, dout);
  hipMemcpy(hout, dout, sizeof hout, hipMemcpyDeviceToHost);
  for (int c = 0; c < 8; ++c) for (int s = 0; s < 4; ++s)
    printf("cvt src %#010x scale bits %#010x sel %d: bf16 (%g, %g)  f16 (%g, %g)\n", hsrc[c], hsc[c], s, hout[(c * 4 + s) * 4], hout[(c * 4 + s) * 4 + 1],
           hout[(c * 4 + s) * 4 + 2], hout[(c * 4 + s) * 4 + 3]);
  return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
