"""Host restatement of the MXFP4 weight format (OCP MX v1.0) as include/v3d.h states it for v3d_quantize_mxfp4_rows, in numpy
f64 (every value of the format and every f16 / bf16 input is exact there).  tests/test_mxfp4_check_cpu.py pins it against
hand-written values; the GPU tests compare the kernels with it.

  W [N, K]  ->  q [N, K/2] uint8: two e2m1 codes per byte, the even k in the low nibble; code = sign(1) | exp(2) | mant(1)
                e [N, K/32] uint8: one E8M0 exponent per 32 consecutive k of a row, value 2^(e - 127)
  per block:  amax = max |w|;  e = clamp(floor(log2(amax)) - 2 + 127, 0, 254), an all-zero block gets 127;
              code = w * 2^(127 - e) rounded to the nearest of {0, .5, 1, 1.5, 2, 3, 4, 6} (ties to the even code, saturating
              at 6); a zero magnitude carries no sign bit; 0xFF is never an exponent.
"""
import numpy as np

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=np.float64)
BLOCK = 32


def to_f64(w):
    """torch tensor (any float dtype, any device) or array -> numpy f64"""
    if hasattr(w, "detach"):
        return w.detach().double().cpu().numpy()
    return np.asarray(w, dtype=np.float64)


def block_exponents(w):
    """[N, K] -> uint8 [N, K/32]"""
    w = to_f64(w)
    n, k = w.shape
    assert k % BLOCK == 0 and np.isfinite(w).all()
    amax = np.abs(w.reshape(n, k // BLOCK, BLOCK)).max(-1)
    _, ex = np.frexp(amax)                             # amax = m * 2^ex, m in [0.5, 1): floor(log2(amax)) = ex - 1
    e = np.clip(ex.astype(np.int64) - 1 - 2 + 127, 0, 254)
    e[amax == 0] = 127
    return e.astype(np.uint8)


def round_e2m1(a):
    """magnitudes (f64, >= 0) -> index 0..7 of the nearest E2M1 value; ties go to the even index, above 6 saturates"""
    d = np.abs(a[..., None] - E2M1)                    # exact: differences of small dyadic numbers
    best = d.min(-1, keepdims=True)
    hit = d == best                                    # one hit, or two neighbours at a tie
    even = hit & (np.arange(8) % 2 == 0)
    pick = np.where(even.any(-1, keepdims=True), even, hit)
    return pick.argmax(-1)


def codes(w, e):
    """[N, K] weights and their block exponents -> uint8 codes [N, K] (one per element, not packed)"""
    w = to_f64(w)
    n, k = w.shape
    shift = 127 - np.repeat(e.astype(np.int64), BLOCK, axis=1)
    scaled = np.ldexp(w, shift)                        # exact
    idx = round_e2m1(np.abs(scaled))
    return (idx | np.where((scaled < 0) & (idx != 0), 8, 0)).astype(np.uint8)


def pack(c):
    """codes [N, K] -> bytes [N, K/2], even k in the low nibble"""
    return (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)


def unpack(q):
    """bytes [N, K/2] -> codes [N, K]"""
    q = np.asarray(q, dtype=np.uint8)
    c = np.empty((q.shape[0], q.shape[1] * 2), dtype=np.uint8)
    c[:, 0::2] = q & 15
    c[:, 1::2] = q >> 4
    return c


def quantize(w):
    """[N, K] -> (q uint8 [N, K/2], e uint8 [N, K/32])"""
    e = block_exponents(w)
    return pack(codes(w, e)), e


def dequantize(q, e):
    """(q [N, K/2], e [N, K/32]) -> f64 [N, K]"""
    if hasattr(q, "detach"):
        q = q.detach().cpu().numpy()
    if hasattr(e, "detach"):
        e = e.detach().cpu().numpy()
    c = unpack(q)
    val = E2M1[c & 7] * np.where(c & 8, -1.0, 1.0)
    return np.ldexp(val, np.repeat(np.asarray(e).astype(np.int64), BLOCK, axis=1) - 127)
