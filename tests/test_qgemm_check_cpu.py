"""tests/qgemm_check.py proved on the CPU: the e4m3 table and the rounding chains against hand-written values, and an f32 emulation of
q8_gemm_tile's arithmetic (128 products per MFMA summed sequentially in f32 from zero, the MFMAs chained over K by one f32 add each, the
epilogue's rounding points) run through the same families and the same compare() as the device tests (tests/test_gpu_qgemm_f64.py).

(a) the clean emulation is bit for bit on the exact and gather families and within the bound on the random family at every shape of the
    device tests.  RECORDED worst ratio of the clean emulation on the random family: e4m3 0.968, MXFP4 0.924 - the output roundings of
    the RES chain, h |y|; the accumulation term is far from mattering, and the emulation passed in the same way with the derived
    C_ACC = 2 before the device's measurement raised the constant to 32 (qgemm_check's docstring);
(b) every mutation of MUTATIONS is reported by at least one family at the smallest shape of the device tests where it can occur (the
    test prints which);
(c) the old rule of tests/test_gpu_fp8.py / test_gpu_fp4.py, slack (eps |ref| + 4 eps rms(ref)), at 64 x 256 x 3584 in bf16 on Gaussian
    data (heavy channel, the project's quantisers), counted per wrong output and for the case as a whole (the test prints the table):
      one product dropped from a row     ACCEPTED as a whole with res (slack 3; 199 of 199 wrong outputs), 96 % of the wrong outputs
                                         with bias (slack 1: 198 of 206, so that case is rejected by 8 outputs);
      exponent byte of block b + 1       77 % of the wrong outputs accepted with res (2876 of 3730), 31 % with bias; with 64 rows behind
                                         every weight row some output always lands outside, so the case as a whole is rejected;
      bias added after the rounding, residual added before it, one e4m3 subnormal decoded as zero     ACCEPTED as a whole;
      k chunks swapped, sa of the next row     rejected (6 .. 21 % of the wrong outputs accepted).
"""
import numpy as np
import pytest
import torch

import mxfp4_check as MX
import qgemm_check as qc
from qgemm_check import EPI_BIAS, EPI_NONE, EPI_RES, EPI_SWIGLU

BF, HF = torch.bfloat16, torch.float16
SHAPES = [(1, 256, 128), (255, 256, 384), (256, 256, 384), (257, 256, 384), (130, 768, 256), (2305, 512, 256), (300, 256, 18944)]
LONG_K = 18944


# ------------------------------------------------------------------------------ hand-written values


def test_e4m3_table_by_hand():
    t = qc.E4M3_VALUES
    assert t[0x00] == 0 and t[0x80] == 0 and np.signbit(t[0x80].item()) and not np.signbit(t[0x00].item())
    assert t[0x01] == 2.0 ** -9 and t[0x07] == 7 * 2.0 ** -9 and t[0x08] == 2.0 ** -6 and t[0x87] == -7 * 2.0 ** -9
    assert t[0x38] == 1.0 and t[0x39] == 1.125 and t[0x40] == 2.0 and t[0xB8] == -1.0
    assert t[0x7E] == 448.0 and t[0xFE] == -448.0 and t[0x77] == 240.0
    assert torch.isnan(t[0x7F]) and torch.isnan(t[0xFF]) and int(torch.isfinite(t).sum()) == 254
    assert len(set(t[torch.isfinite(t)].tolist())) == 253                     # +0 and -0 compare equal
    # torch's own e4m3 agrees on every finite byte
    b = torch.arange(256, dtype=torch.uint8)
    fin = torch.isfinite(t)
    assert torch.equal(b.view(torch.float8_e4m3fn).double()[fin], t[fin])
    assert qc.e4m3_integers(40) == list(range(17)) + [18, 20, 22, 24, 26, 28, 30, 32, 36, 40]


def test_host_quantiser_ties_and_edges_by_hand():
    """host_quantize_e4m3 on a row whose amax is 448 (scale exactly 1): ties of the e4m3 grid go to the even code."""
    x = torch.tensor([[448.0, 2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 1.0625, 1.1875, 17.0, 19.0, -0.0, 432.0, -2.0 ** -10, 2.0 ** -11 * 3,
                       0.0, 0.0, 0.0, 0.0]], dtype=torch.float32)
    q, s = qc.host_quantize_e4m3(x)
    assert s.item() == 1.0
    want = [448.0, 0.0, 2 * 2.0 ** -9, 2 * 2.0 ** -9, 1.0, 1.25, 16.0, 20.0, -0.0, 448.0, -0.0, 2.0 ** -9, 0, 0, 0, 0]
    assert qc.decode_e4m3(q)[0].tolist() == want
    assert q[0, 0] == 0x7E and q[0, 8] == 0x80 and q[0, 10] == 0x80 and q[0, 1] == 0x00
    # the scale rule: amax / 448, floored at the smallest normal f32; 1 for a zero row
    x = torch.tensor([[1e-37, 0.0, -5e-38, 0, 0, 0, 0, 0], [0.0] * 8, [896.0, -1.0, 0, 0, 0, 0, 0, 0]], dtype=torch.bfloat16)
    q, s = qc.host_quantize_e4m3(x)
    assert s.tolist() == [2.0 ** -126, 1.0, 2.0]
    assert q[1].tolist() == [0] * 8 and q[2, :2].tolist() == [0x7E, 0xB0]
    assert int(((q & 0x7F) == 0x7F).sum()) == 0 and q[0, 1] == 0


def test_chain_by_hand():
    """One row, hand-computed: y = 1.0 * 1.125 * 2^-1 * 2^-2 per column pair, the four epilogues' rounding points."""
    N, K = 256, 128
    qa = torch.zeros(1, K, dtype=torch.uint8)
    qa[0, 5] = 0x7E                                              # 448
    w = torch.zeros(N, K, dtype=torch.uint8)
    w[:, 5] = 0x39                                               # 1.125
    w[64:128, 5] = 0x7E                                          # up columns of the first pair: 448
    c = qc.Case("e4m3", qa, torch.tensor([0.5]), w, torch.full((N,), 0.25), torch.full((N,), 0.5, dtype=BF), torch.full((1, N), 3.0, dtype=BF))
    a, wd = qc.dequant(c)
    y = 448 * 1.125 * 0.125                                      # 63.0
    assert (a @ wd.T)[0, 0] == y and (a @ wd.T)[0, 64] == 448 * 448 * 0.125
    d = qc.depth(K) * qc.C_ACC / qc.gc.C_ACC                     # compare()'s argument: gemm_check multiplies by its own C_ACC
    r = qc.gc.reference(a, wd, c.bias, c.res, EPI_BIAS, dt=BF, depth=d, lin_rel=qc.LIN_REL)
    assert r["out"][0, 0] == 63.5 and r["rounded"][0, 0] == 63.5
    assert r["bound"][0, 0] == qc.C_ACC * 129 * 2.0 ** -24 * 63.5 + (2.0 ** -8 + 3 * 2.0 ** -24) * 63.5
    r = qc.gc.reference(a, wd, c.bias, c.res, EPI_RES, dt=BF, depth=d)
    assert r["rounded"][0, 64] == 25088.0 and r["out"][0, 64] == 25091.0           # bf16 spacing 128 there: 25091 -> 25088
    assert r["rounded"][0, 0] == 66.0 and r["out"][0, 0] == 66.0
    r = qc.gc.reference(a, wd, c.bias, c.res, EPI_SWIGLU, dt=BF, depth=d)
    assert r["rounded"].shape == (1, 128) and r["lo"][0, 0] <= r["rounded"][0, 0] <= r["hi"][0, 0]
    assert r["rounded"][0, 0] == torch.tensor(63.0 * 25088.0).to(BF).double()          # silu(63) = 63 in bf16
    # MXFP4: code 0x2 = 1.0 in the low nibble (even k), exponent byte 130 = 2^3
    q4 = torch.zeros(N, K // 2, dtype=torch.uint8)
    q4[:, 2] = 0x20 | 0x0D                                       # k = 4: -3.0, k = 5: 1.0
    c4 = qc.Case("mxfp4", qa, torch.tensor([0.5]), q4, torch.full((N, K // 32), 130, dtype=torch.uint8), c.bias, c.res)
    a, wd = qc.dequant(c4)
    assert wd[0, 4] == -24.0 and wd[0, 5] == 8.0 and (a @ wd.T)[0, 0] == 448 * 0.5 * 8.0


# ------------------------------------------------------------------------------ the emulation

MUTATIONS = {
    # name: (epilogue, formats, smallest shape of the device tests where it can occur)
    "k_chunks_swapped": (EPI_NONE, qc.FORMATS, (1, 256, 128)),
    "nibbles_swapped": (EPI_NONE, ("mxfp4",), (1, 256, 128)),
    "stale_ring_buffer": (EPI_NONE, qc.FORMATS, (130, 768, 256)),
    "last_k_step_dropped": (EPI_NONE, qc.FORMATS, (130, 768, 256)),
    "exponent_of_next_block": (EPI_NONE, ("mxfp4",), (1, 256, 128)),
    "exponent_of_next_row": (EPI_NONE, ("mxfp4",), (1, 256, 128)),
    "sa_of_next_row": (EPI_NONE, qc.FORMATS, (130, 768, 256)),
    "sw_of_column_plus_16": (EPI_NONE, ("e4m3",), (1, 256, 128)),
    "swiglu_up_wrong_32_block": (EPI_SWIGLU, qc.FORMATS, (1, 256, 128)),
    "bias_after_rounding": (EPI_BIAS, qc.FORMATS, (1, 256, 128)),
    "residual_before_rounding": (EPI_RES, qc.FORMATS, (1, 256, 128)),
    "one_product_dropped": (EPI_NONE, qc.FORMATS, (1, 256, 128)),
    "subnormal_decoded_as_zero": (EPI_NONE, qc.FORMATS, (1, 256, 128)),
}


def _operands(c, mut=None, block=None):
    """Case -> (A [M, K], W [N, K]) f64 WITHOUT sa / sw (the MFMA's operands; block exponents inside W), after an operand mutation."""
    table = qc.E4M3_VALUES.clone()
    if mut == "subnormal_decoded_as_zero":
        table[0x01] = 0.0
    A = qc.decode_e4m3(c.qa, table)
    if c.fmt == "e4m3":
        W = qc.decode_e4m3(c.w, table)
    else:
        q, e = c.w.numpy(), c.wx.numpy().copy()
        if mut == "nibbles_swapped":
            q = ((q >> 4) | (q << 4)).astype(np.uint8)
        if mut == "exponent_of_next_block":                      # block b takes the byte of block b + 1: every block, or only `block`
            if block is None:
                e = np.roll(e, -1, axis=1)
            else:
                e[:, block] = e[:, block + 1]
        if mut == "exponent_of_next_row":
            e = np.roll(e, -1, axis=0)
        W = torch.from_numpy(MX.dequantize(q, e))
    K = A.shape[1]
    if mut == "k_chunks_swapped":
        A = A.clone()
        A[:, 0:16], A[:, 16:32] = A[:, 16:32].clone(), A[:, 0:16].clone()
    if mut == "stale_ring_buffer":                               # the last step sees the weights of the step before it
        W = W.clone()
        W[:, K - 128:] = W[:, K - 256: K - 128]
    if mut == "last_k_step_dropped":
        A = A.clone()
        A[:, K - 128:] = 0
    if mut == "one_product_dropped":
        A = A.clone()
        m = A.shape[0] // 2
        A[m, int((A[m] != 0).nonzero()[0])] = 0
    return A, W


def _accumulate(A, W):
    """f32 [M, N]: per K-step the 128 products summed one after the other from zero (each product is exact in f32), steps chained.
    Operands in f64: they are multiplied in f32 where both fit it, else (6 x 2^127 of the exponent walk) in f64 and the exact product
    taken to f32."""
    acc = torch.zeros(A.shape[0], W.shape[0])
    if float(W.abs().max()) < 2.0 ** 127 and float(A.abs().max()) < 2.0 ** 127:
        A, W = A.float(), W.float()
    Wt = W.T.contiguous()
    for t in range(A.shape[1] // 128):
        part = torch.zeros_like(acc)
        for k in range(128 * t, 128 * t + 128):
            part = part + (A[:, k, None] * Wt[k][None, :]).float()
        acc = acc + part
    return acc


def _silu32(x):
    return x * (1.0 / (1.0 + torch.exp2(-1.4426950408889634 * x)))


def _epilogue(acc, c, dt, epi, mut=None):
    sa, N = c.sa.float(), acc.shape[1]
    if mut == "sa_of_next_row":
        sa = torch.roll(sa, -1)
    if c.fmt == "e4m3":
        sw = c.wx.float()
        if mut == "sw_of_column_plus_16":
            sw = torch.roll(sw, -16)
        v = acc * (sa[:, None] * sw[None, :])
    else:
        v = acc * sa[:, None]
    if epi == EPI_BIAS:
        if mut == "bias_after_rounding":
            return (v.to(dt).float() + c.bias.float()).to(dt)
        return (v + c.bias.float()).to(dt)
    if epi == EPI_RES:
        if mut == "residual_before_rounding":
            return (v + c.res.float()).to(dt)
        return (v.to(dt).float() + c.res.float()).to(dt)
    if epi == EPI_SWIGLU:
        g, u = qc.gc.split_gate_up(v.to(dt).float())
        if mut == "swiglu_up_wrong_32_block":
            u = u.reshape(-1, N // 128, 2, 32).flip(2).reshape(-1, N // 2)
        return (_silu32(g).to(dt).float() * u).to(dt)
    return v.to(dt)


def emulate(c, dt, epi, mut=None):
    return _epilogue(_accumulate(*_operands(c, mut)), c, dt, epi, mut)


FAMILIES = ("gather", "gather_t", "exact", "random0", "random1")


def make(family, fmt, M, N, K, dt, epi):
    if family == "gather":
        return qc.gather_inputs(fmt, M, N, K, dt, stride=37, shift=5)
    if family == "gather_t":
        return qc.gather_inputs(fmt, M, N, K, dt, stride=37, shift=5, transposed=True)
    if family == "exact":
        return qc.exact_inputs(fmt, M, N, K, dt, epi, seed=M + K)
    return qc.random_inputs(fmt, M, N, K, dt, draw=int(family[-1]), seed=M + K)


def reports(family, r, epi):
    """Does the check of this family fail on result r?"""
    if family.startswith("random"):
        return not r["ratio"] <= 1.0
    return r["outside"] > 0 if epi == EPI_SWIGLU else r["unequal"] > 0


# ------------------------------------------------------------------------------ (a) the clean emulation passes

_WORST = {}


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("fmt", qc.FORMATS)
def test_clean_emulation_passes(fmt, M, N, K):
    fams = [f for f in FAMILIES if K != LONG_K or not f.startswith("gather")]
    for family in fams:
        base = make(family, fmt, M, N, K, BF, EPI_NONE)
        acc = _accumulate(*_operands(base))
        for dt in (BF, HF):
            for epi in qc.EPIS:
                c = make(family, fmt, M, N, K, dt, epi)
                if not (torch.equal(c.qa, base.qa) and torch.equal(c.w, base.w)):     # other codes (the Gaussian draw per dt, an exact
                    base, acc = c, _accumulate(*_operands(c))                         # case narrowed for its bias): accumulate again
                got = _epilogue(acc, c, dt, epi)
                r = qc.compare(got, c, dt, epi, exact=family == "exact")
                what = f"{fmt} {family} {M}x{N}x{K} {dt} {qc.EPI_NAMES[epi]}: {r}"
                if family.startswith("random"):
                    assert r["ratio"] <= 1.0, what
                    _WORST[fmt] = max(_WORST.get(fmt, 0.0), r["ratio"])
                else:
                    assert r["outside"] == 0 and (epi == EPI_SWIGLU or r["unequal"] == 0), what
                if family == "exact":
                    assert r["needs_rounding"] > 0.5, what


def test_exponent_walk_emulation_passes():
    for dt in (BF, HF):
        c = qc.gather_exponent_walk(256, 256, 1792, dt)
        assert set(c.wx[0].tolist()) == set(qc.WALK_EXPONENTS)
        A, W = _operands(c)
        assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(W).all())
        acc = _accumulate(A, W)
        nz = acc[acc != 0].abs()
        assert nz.min() >= 2.0 ** -126 and bool(torch.isfinite(acc).all())           # every accumulator a normal f32
        r = qc.compare(_epilogue(acc, c, dt, EPI_NONE), c, dt, EPI_NONE)
        assert r["unequal"] == 0, r
        # a wrong exponent byte (the one of the next block) is seen
        bad = _epilogue(_accumulate(*_operands(c, "exponent_of_next_block")), c, dt, EPI_NONE)
        assert qc.compare(bad, c, dt, EPI_NONE)["unequal"] > 0


def test_zz_report_clean_ratios():
    print("\nclean f32 emulation, worst ratio on the random family: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(_WORST.items())))


# ------------------------------------------------------------------------------ (b) every mutation is reported


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_mutation_is_reported(mut):
    epi, fmts, (M, N, K) = MUTATIONS[mut]
    lines = []
    for fmt in fmts:
        for dt in (BF, HF):
            caught = []
            for family in FAMILIES[:4]:
                c = make(family, fmt, M, N, K, dt, epi)
                clean = qc.compare(emulate(c, dt, epi), c, dt, epi)
                assert not reports(family, clean, epi), f"{fmt} {family}: the clean emulation is reported: {clean}"
                if reports(family, qc.compare(emulate(c, dt, epi, mut), c, dt, epi), epi):
                    caught.append(family)
            lines.append(f"{mut:28s} {fmt:5s} {str(dt)[6:]:8s} {M}x{N}x{K}: reported by {', '.join(caught) or 'NO FAMILY'}")
            assert caught, lines[-1]
    print("\n" + "\n".join(lines))


def test_gather_explain_names_the_k():
    c = make("gather", "e4m3", 1, 256, 128, BF, EPI_NONE)                           # 128 distinct bytes in a row
    got = emulate(c, BF, EPI_NONE, "k_chunks_swapped")
    text = qc.gather_explain(got, c)
    assert "(k = 5)" in text and "k = [21]" in text, text                           # row 0 reads k0 = shift = 5; the swap brought k = 21


# ------------------------------------------------------------------------------ (c) what the old rule accepts


def test_old_rule_accepts_what_the_new_check_reports():
    M, N, K, dt = 64, 256, 3584, BF
    share, whole = {}, {}
    for fmt in qc.FORMATS:
        c = qc.random_inputs(fmt, M, N, K, dt, draw=1, seed=3)
        acc = _accumulate(*_operands(c))
        for epi in (EPI_BIAS, EPI_RES):
            clean = _epilogue(acc, c, dt, epi)
            assert bool(qc.old_rule(clean, c, dt, epi).all())
            for mut in ("one_product_dropped", "exponent_of_next_block", "k_chunks_swapped", "sa_of_next_row", "bias_after_rounding",
                        "residual_before_rounding", "subnormal_decoded_as_zero"):
                if fmt not in MUTATIONS[mut][1] or (mut.startswith("bias") and epi != EPI_BIAS) or (mut.startswith("res") and epi != EPI_RES):
                    continue
                got = _epilogue(_accumulate(*_operands(c, mut, block=7)), c, dt, epi, mut)
                ok = qc.old_rule(got, c, dt, epi)
                wrong = got != clean
                key = (fmt, qc.EPI_NAMES[epi], mut)
                whole[key] = bool(ok.all())
                share[key] = (int((ok & wrong).sum()), int(wrong.sum()))
    print("\nold rule at 64 x 256 x 3584, bf16, Gaussian data: wrong outputs it accepts / wrong outputs; the case as a whole")
    for key, (acc_n, n) in share.items():
        print(f"  {key[0]:5s} {key[1]:4s} {key[2]:28s} {acc_n:6d} / {n:6d}   {'ACCEPTED' if whole[key] else 'rejected'}")
    for fmt in qc.FORMATS:
        assert whole[(fmt, "res", "one_product_dropped")]
        n_ok, n = share[(fmt, "bias", "one_product_dropped")]
        assert n > 100 and n_ok > 0.9 * n
    # a halved block moves an output by sqrt(32 / K) / 2 rms = 0.047 rms (one sigma): the floor of the old rule with its slack of 3
    n_ok, n = share[("mxfp4", "res", "exponent_of_next_block")]
    assert n > 1000 and n_ok > 0.5 * n
    for key in whole:
        if key[2] in ("bias_after_rounding", "residual_before_rounding", "subnormal_decoded_as_zero"):
            assert whole[key]
