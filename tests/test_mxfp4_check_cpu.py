"""tests/mxfp4_check.py (the host restatement of the MXFP4 format the GPU tests compare the kernels with) against hand-written
values: it is the yardstick of tests/test_gpu_fp4.py, so it is pinned here and not against itself."""
import numpy as np

import mxfp4_check as MX


def _block(values, fill=0.0):
    """one row of one 32-block holding `values` first"""
    b = np.full((1, 32), fill, dtype=np.float64)
    b[0, : len(values)] = values
    return b


def test_all_sixteen_codes_dequantise_to_their_values():
    q = np.array([[0x10, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE] + [0] * 8], dtype=np.uint8)     # codes 0..15 in k order
    e = np.array([[127]], dtype=np.uint8)
    want = [0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6]
    got = MX.dequantize(q, e)
    assert got.shape == (1, 32) and got[0, :16].tolist() == want and not got[0, 16:].any()
    assert MX.dequantize(q, np.array([[130]], dtype=np.uint8))[0, :16].tolist() == [8 * v for v in want]
    assert MX.dequantize(q, np.array([[120]], dtype=np.uint8))[0, 7] == 6.0 / 128


def test_every_code_is_reached_and_keeps_its_sign():
    # amax 6 -> floor(log2) = 2 -> e = 127: the elements are their own scaled values
    vals = [6, 0.5, 1, 1.5, 2, 3, 4, 0, -0.5, -1, -1.5, -2, -3, -4, -6]
    q, e = MX.quantize(_block(vals))
    assert e.tolist() == [[127]]
    assert MX.unpack(q)[0, :15].tolist() == [7, 1, 2, 3, 4, 5, 6, 0, 9, 10, 11, 12, 13, 14, 15]


def test_ties_round_to_the_even_code():
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    q, e = MX.quantize(_block([6.0] + ties + [-t for t in ties]))
    assert e.tolist() == [[127]]
    c = MX.unpack(q)[0]
    assert c[1:8].tolist() == [0, 2, 2, 4, 4, 6, 6]            # 0, 1, 1, 2, 2, 4, 4
    assert c[8:15].tolist() == [0, 10, 10, 12, 12, 14, 14]     # -0.25 -> magnitude zero carries no sign
    # just off the ties
    q, _ = MX.quantize(_block([6.0, 0.2500001, 0.7499999, 1.2500001, 1.7499999, 2.5000001, 3.4999999, 5.0000001, -0.1]))
    assert MX.unpack(q)[0, 1:9].tolist() == [1, 1, 3, 3, 5, 5, 7, 0]


def test_saturation_at_six():
    # amax 7.5: floor(log2) = 2 -> e = 127, 7.5 and 7.9 saturate at 6 (code 7), -7 at -6
    q, e = MX.quantize(_block([7.5, 7.9, -7.0, 5.5]))
    assert e.tolist() == [[127]]
    assert MX.unpack(q)[0, :4].tolist() == [7, 7, 15, 7]


def test_power_of_two_amax():
    # amax = 2^5 exactly: e = 5 - 2 + 127 = 130, amax scales to 4.0 (code 6); one ulp (bf16) below 2^5 scales to 7.97 -> e = 129, code 7
    q, e = MX.quantize(_block([32.0, 16.0, 3.0, -1.0]))
    assert e.tolist() == [[130]]
    assert MX.unpack(q)[0, :4].tolist() == [6, 4, 1, 0]               # 4, 2, 0.375 -> 0.5, -0.125 -> 0 (no sign)
    q, e = MX.quantize(_block([31.875]))
    assert e.tolist() == [[129]] and MX.unpack(q)[0, 0] == 7
    q, e = MX.quantize(_block([2.0 ** -20, -(2.0 ** -21)]))
    assert e.tolist() == [[127 - 22]] and MX.unpack(q)[0, :2].tolist() == [6, 12]


def test_zero_block_and_exponent_clamps():
    w = np.zeros((1, 96))
    w[0, 32] = 2.0 ** -130                 # floor(log2) - 2 + 127 = -5 -> clamp 0: scaled by 2^127 -> 2^-3 -> code 0
    w[0, 33] = 2.0 ** -126                 # ... -> 2^1 = 2 -> code 4
    w[0, 64] = 2.0 ** 130                  # 130 - 2 + 127 = 255 -> clamp 254 (0xFF is never written): scaled 2^3 -> saturates, code 7
    w[0, 65] = -(2.0 ** 128)               # 2^1 -> code 4 | 8
    q, e = MX.quantize(w)
    assert e.tolist() == [[127, 0, 254]]
    c = MX.unpack(q)[0]
    assert not c[:32].any() and not q[0, :16].any()
    assert c[32:34].tolist() == [0, 4] and c[64:66].tolist() == [7, 12]
    d = MX.dequantize(q, e)[0]
    assert d[33] == 2.0 * 2.0 ** -127 and d[64] == 6.0 * 2.0 ** 127 and d[65] == -(2.0 ** 128)


def test_nibble_order_and_shapes():
    w = np.zeros((2, 64))
    w[0, 0], w[0, 1], w[0, 2] = 6.0, 1.0, -3.0          # k = 0 low nibble of byte 0, k = 1 high nibble, k = 2 low nibble of byte 1
    w[1, 63] = -6.0
    q, e = MX.quantize(w)
    assert q.shape == (2, 32) and e.shape == (2, 2) and q.dtype == np.uint8 and e.dtype == np.uint8
    assert q[0, 0] == (2 << 4 | 7) and q[0, 1] == 13 and q[1, 31] == 15 << 4
    assert MX.pack(np.array([[1, 2, 3, 4]], dtype=np.uint8)).tolist() == [[0x21, 0x43]]
    assert MX.unpack(np.array([[0x21, 0x43]], dtype=np.uint8)).tolist() == [[1, 2, 3, 4]]
    assert e.tolist() == [[127, 127], [127, 127]]
    assert np.array_equal(MX.dequantize(q, e), w)


def test_round_trip_of_representable_values_is_exact():
    rng = np.random.default_rng(0)
    c = rng.integers(0, 16, size=(4, 128)).astype(np.uint8)
    c[:, ::32] = 7                                       # every block holds a 6: its exponent is recovered exactly
    e = rng.integers(100, 150, size=(4, 4)).astype(np.uint8)
    w = MX.dequantize(MX.pack(c), e)
    q2, e2 = MX.quantize(w)
    assert np.array_equal(e2, e)
    c2 = MX.unpack(q2)
    assert np.array_equal(c2 & 7, c & 7) and np.array_equal(c2[(c & 7) != 0], c[(c & 7) != 0])
