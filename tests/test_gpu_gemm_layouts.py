"""v3d_gemm_layout (k-major operand layouts of the 16-bit MFMA GEMM) per element against the f64 reference and bound of
tests/gemm_check.py, on both tile forms (V3D_GEMM_LAYOUT_TILE = 128 / 256), both dtypes and the three layouts with a k-major operand:
  NN (a_kmajor, b_kmajor) = (0, 1)   dx = dy . W on W as stored        TN (1, 1)   dW = dy^T . x on dy, x as stored        TK (1, 0)
The k-major operands are handed to gc.reference / gc.compare as .t() views of what the kernel gets.

Every case: every operand lives in a larger buffer whose padding is NaN - a leading dimension above its minimum, and for a k-major
operand 64 NaN rows behind row K (a TN product with a K tail that read memory instead of the zero line would return NaN); the output is
a window, pre-filled with NaN, of a buffer of sentinels that must come back untouched.  Families: *exact* (integer sums, torch.equal
with the rounded f64 chain, EPI_NONE and EPI_RES), *gather* (one-hot rows: the output names the k that was read) and *random* under
gemm_check's bound.

Bound.  gemm_check's, unchanged: lin = C_ACC (K / 32 + C0) 2^-24 mag + h |y|, K / 32 taken as a real number.  The new kernels sum k
ascending in one run of ceil(K / 32) MFMAs per output - no split-K tail, so the chain is shorter than the depth K / 32 + 35 the constants
were settled for; the zero rows of a K tail add exact zeros.  No new constant.

The training switch (V3D_TRAIN_GEMM_LAYOUTS=1): linear_backward against the same bound and, on exact inputs, torch.equal with the
switch-off result; a decoder layer against the switch-off run within the tolerances tests/test_gpu_train_dense.py holds that block to
against autograd; peak memory of one call.  "136 x 384 x 192" is tokens x in-features x out-features (w [192, 384]): the other reading
gives dx 192 columns, which no tile of either path takes.

Measured on one MI355X (120 tests, 4 s): exact 1020 compared launches, 0 unequal (worst |err| / bound 0.995); gather 0 mismatches; worst |err| / bound
on random inputs 0.991 (the bound at these K is almost only the output rounding h |y|, as for v3d_gemm at short K); peak memory over one
1024^3 linear_backward 10 MiB with the switch off, 4 MiB with it on.
"""
import pytest
import torch

import gemm_check as gc
from gemm_check import EPI_NONE, EPI_RES

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
MODES = {"NN": (False, True), "TN": (True, True), "TK": (True, False)}
SENT = 7.0
GUARD_ROWS, GUARD_COLS, LD_PAD, K_GUARD = 8, 64, 8, 64
ENV_TILE = "V3D_GEMM_LAYOUT_TILE"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from v3d import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def train():
    from v3d import train as t
    return t


def stored(x, kmajor):
    """The logical operand x [rows, K] as the kernel gets it: a window of a NaN-filled buffer, ld = minimum + LD_PAD; k-major: [K, rows]
    with K_GUARD NaN rows behind it."""
    rows, K = x.shape
    if kmajor:
        buf = torch.full((K + K_GUARD, rows + LD_PAD), float("nan"), dtype=x.dtype, device=x.device)
        buf[:K, :rows] = x.t()
        return buf[:K, :rows]
    buf = torch.full((rows, K + LD_PAD), float("nan"), dtype=x.dtype, device=x.device)
    buf[:, :K] = x
    return buf[:, :K]


def logical(t, kmajor):
    return t.t() if kmajor else t


def launch(ops, a, w, mode, res=None, inplace=False):
    """a [M, K], w [N, K] logical -> (out window [M, N], the stored operands, the stored residual)."""
    akm, bkm = MODES[mode]
    M, N = a.shape[0], w.shape[0]
    sa, sb = stored(a, akm), stored(w, bkm)
    sres = None
    if res is not None:
        rbuf = torch.full((M, N + LD_PAD), float("nan"), dtype=a.dtype, device=a.device)
        rbuf[:, :N] = res
        sres = rbuf[:, :N]
    if inplace:
        out, frame = sres, None
    else:
        frame = torch.full((M + GUARD_ROWS, N + GUARD_COLS), SENT, dtype=a.dtype, device=a.device)
        out = frame[:M, :N]
        out.fill_(float("nan"))
    got = ops.gemm_layout(sa, sb, a_kmajor=akm, b_kmajor=bkm, res=sres, epilogue=EPI_RES if res is not None else EPI_NONE, out=out)
    assert got.data_ptr() == out.data_ptr()
    if frame is not None:
        assert bool((frame[M:] == SENT).all()) and bool((frame[:, N:] == SENT).all()), "guard rows / columns were written"
    if inplace:
        assert bool(torch.isnan(rbuf[:, N:]).all()), "the residual's padding was written"
    return out, sa, sb


def n_list(tile):
    return (256, 512) if tile == 256 else (128, 256, 512)


def k_list(mode):
    ks = [64, 128, 192, 320]
    if mode == "TN":
        ks += [1, 7, 65, 200, 6794 % 64 + 128]
    return ks


@pytest.mark.parametrize("epi", [EPI_NONE, EPI_RES], ids=["none", "res"])
@pytest.mark.parametrize("tile", [128, 256])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dt", list(DT))
def test_exact_inputs_bit_for_bit(ops, monkeypatch, dt, mode, tile, epi):
    monkeypatch.setenv(ENV_TILE, str(tile))
    akm, bkm = MODES[mode]
    seed, report = 0, []
    for M in (8, 136, 264):
        for N in n_list(tile):
            for K in k_list(mode):
                seed += 1
                a, w, _, r = gc.exact_inputs(M, N, K, DT[dt], seed=seed, device="cuda")
                res = r if epi == EPI_RES else None
                out, sa, sb = launch(ops, a, w, mode, res)
                c = gc.compare(out, logical(sa, akm), logical(sb, bkm), res=res, epi=epi, exact=True)
                print(f"{dt} {mode} tile {tile} epi {epi} M {M} N {N} K {K}: unequal {c['unequal']} ratio {c['ratio']:.3f}")
                if c["unequal"] or not c["ratio"] <= 1.0:
                    report.append((M, N, K, c["unequal"], c["ratio"]))
    assert not report, f"(M, N, K, unequal, ratio): {report[:12]}"


@pytest.mark.parametrize("tile", [128, 256])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dt", list(DT))
def test_in_place_residual(ops, monkeypatch, dt, mode, tile):
    monkeypatch.setenv(ENV_TILE, str(tile))
    akm, bkm = MODES[mode]
    M, N, K = 264, 512, 192 if mode != "TN" else 200
    a, w, _, r = gc.exact_inputs(M, N, K, DT[dt], seed=11, device="cuda")
    out, sa, sb = launch(ops, a, w, mode, r, inplace=True)
    c = gc.compare(out, logical(sa, akm), logical(sb, bkm), res=r, epi=EPI_RES, exact=True)
    assert c["unequal"] == 0, c


@pytest.mark.parametrize("stride,shift", [(1, 0), (7, 3)])
@pytest.mark.parametrize("transposed", [False, True], ids=["a_onehot", "b_onehot"])
@pytest.mark.parametrize("tile", [128, 256])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dt", list(DT))
def test_gather_names_the_k_that_was_read(ops, monkeypatch, dt, mode, tile, transposed, stride, shift):
    """M >= K = 192 and N >= K: with stride 1 every k of three K-steps is selected by some row of the one-hot operand."""
    monkeypatch.setenv(ENV_TILE, str(tile))
    M, N, K = 264, 256, 192
    a, w, want = gc.gather_inputs(M, N, K, DT[dt], stride=stride, shift=shift, device="cuda", transposed=transposed)
    out, _, _ = launch(ops, a, w, mode)
    assert torch.equal(out, want), gc.gather_explain(out, a, w, want, transposed=transposed)


RANDOM_SHAPES = {128: [(264, 384, 320), (520, 128, 192)], 256: [(264, 256, 320), (520, 512, 192)]}


@pytest.mark.parametrize("epi", [EPI_NONE, EPI_RES], ids=["none", "res"])
@pytest.mark.parametrize("tile", [128, 256])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dt", list(DT))
def test_random_inputs_within_the_f64_bound(ops, monkeypatch, dt, mode, tile, epi):
    monkeypatch.setenv(ENV_TILE, str(tile))
    akm, bkm = MODES[mode]
    shapes = list(RANDOM_SHAPES[tile])
    if mode == "TN":
        shapes.append((264, shapes[0][1], 6794 % 64 + 128))
    for i, (M, N, K) in enumerate(shapes):
        a, w, _, r = gc.random_inputs(M, N, K, DT[dt], seed=20 + i, device="cuda")
        res = r if epi == EPI_RES else None
        out, sa, sb = launch(ops, a, w, mode, res)
        again, _, _ = launch(ops, a, w, mode, res)
        assert torch.equal(out, again), "two launches differ"
        c = gc.compare(out, logical(sa, akm), logical(sb, bkm), res=res, epi=epi)
        print(f"{dt} {mode} tile {tile} epi {epi} {M} x {N} x {K}: ratio {c['ratio']:.3f}")
        assert c["ratio"] <= 1.0, (M, N, K, c)


def test_default_tile_choice_runs_both_forms(ops, monkeypatch):
    """No switch: the cost model picks (128 form at few tiles, 256 form at many); both answers are the exact one."""
    monkeypatch.delenv(ENV_TILE, raising=False)
    for M, N, K in ((136, 256, 128), (2056, 4096, 1024)):
        a, w, _, _ = gc.exact_inputs(M, N, K, torch.bfloat16, seed=5, device="cuda")
        out, sa, sb = launch(ops, a, w, "TN")
        assert gc.compare(out, sa.t(), sb.t(), exact=True)["unequal"] == 0
    monkeypatch.setenv(ENV_TILE, "256")
    with pytest.raises(ops.V3DError, match="V3D_GEMM_LAYOUT_TILE"):
        ops.gemm_layout(torch.zeros(64, 128, dtype=torch.bfloat16, device="cuda"), torch.zeros(64, 128, dtype=torch.bfloat16, device="cuda"),
                        a_kmajor=True, b_kmajor=True)


def test_flags_off_is_v3d_gemm(ops):
    a, w, _, _ = gc.random_inputs(136, 256, 128, torch.bfloat16, seed=3, device="cuda")
    assert torch.equal(ops.gemm_layout(a, w), ops.gemm(a, w))


# ------------------------------------------------------------------------------ the training switch

TRAIN_SHAPES = [(200, 128, 256), (136, 384, 192)]        # tokens M, in-features K, out-features N (x [M, K], w [N, K], dy [M, N])


def _backward(train, x, w, dy, res, on, monkeypatch):
    if on:
        monkeypatch.setenv("V3D_TRAIN_GEMM_LAYOUTS", "1")
    else:
        monkeypatch.delenv("V3D_TRAIN_GEMM_LAYOUTS", raising=False)
    dx, dw, _ = train.linear_backward(x, w, dy, res=res)
    torch.cuda.synchronize()
    return dx, dw


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("M,K,N", TRAIN_SHAPES)
@pytest.mark.parametrize("dt", list(DT))
def test_linear_backward_with_the_switch(train, monkeypatch, dt, M, K, N, with_res):
    monkeypatch.delenv(ENV_TILE, raising=False)
    g = torch.Generator(device="cuda").manual_seed(M + N)
    mk = lambda *s, sc=1.0: (torch.randn(*s, generator=g, device="cuda") * sc).to(DT[dt])
    x, w, dy = mk(M, K), mk(N, K, sc=K ** -0.5), mk(M, N, sc=0.5)
    res = mk(M, K) if with_res else None
    calls = []
    real = train.ops.gemm_layout
    monkeypatch.setattr(train.ops, "gemm_layout", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    dx, dw = _backward(train, x, w, dy, res, True, monkeypatch)
    assert len(calls) == 2, "the switch did not route dx and dw through gemm_layout"
    c = gc.compare(dx, dy, w.t(), res=res, epi=EPI_RES if with_res else EPI_NONE)
    assert c["ratio"] <= 1.0, ("dx", c)
    c = gc.compare(dw, dy.t(), x.t())
    assert c["ratio"] <= 1.0, ("dw", c)
    # exact inputs: the same bits as the transposing path
    amax = gc.exact_amax(max(M, N))
    ri = lambda *s: torch.randint(-amax, amax + 1, s, generator=g, device="cuda").to(DT[dt])
    x, w, dy = ri(M, K), ri(N, K), ri(M, N)
    res = (ri(M, K) * 8).to(DT[dt]) if with_res else None
    on = _backward(train, x, w, dy, res, True, monkeypatch)
    n_on = len(calls)
    off = _backward(train, x, w, dy, res, False, monkeypatch)
    assert len(calls) == n_on, "the switch-off path called gemm_layout"
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])


def test_decoder_layer_with_the_switch_matches_the_switch_off_run(train, monkeypatch):
    from test_gpu_train_dense import _close
    S, H, I, n_q, n_kv, hd = 200, 256, 512, 2, 1, 128
    g = torch.Generator().manual_seed(S)
    width = (n_q + 2 * n_kv) * hd
    mk = lambda *shape, s=1.0: (torch.randn(*shape, generator=g) * s).to(torch.bfloat16).cuda()
    p = {"ln1": (1 + 0.1 * torch.randn(H, generator=g)).to(torch.bfloat16).cuda(), "qkv": mk(width, H, s=H ** -0.5), "qkv_bias": mk(width, s=0.5),
         "o": mk(H, n_q * hd, s=(n_q * hd) ** -0.5), "ln2": (1 + 0.1 * torch.randn(H, generator=g)).to(torch.bfloat16).cuda(),
         "gate_up": mk(2 * I, H, s=H ** -0.5), "down": mk(H, I, s=I ** -0.5)}
    h, dout = mk(S, H), mk(S, H)
    rope = train.RopeTables(hd, 512, 1e6, torch.bfloat16, "cuda")
    runs = {}
    for on in (False, True):
        if on:
            monkeypatch.setenv("V3D_TRAIN_GEMM_LAYOUTS", "1")
        else:
            monkeypatch.delenv("V3D_TRAIN_GEMM_LAYOUTS", raising=False)
        out, saved = train.decoder_layer_forward(h, p, rope, n_q, n_kv, hd)
        dh, grads = train.decoder_layer_backward(dout, saved, p, rope, n_q, n_kv, hd)
        torch.cuda.synchronize()
        runs[on] = (out, dh, grads)
    assert torch.equal(runs[True][0], runs[False][0])          # the forward does not read the switch
    _close(runs[True][1], runs[False][1].float().cpu(), 1.5e-2, 4e-2, "dh")
    for k in p:
        _close(runs[True][2][k], runs[False][2][k].float().cpu(), 1.5e-2, 4e-2, "d " + k)


def test_peak_memory_of_one_linear_backward(train, monkeypatch):
    """1024 x 1024 x 1024 bf16, called on its own (no side stream): every tensor is one 2 MiB allocator block.  The transposing path
    holds w^T, dx, dy^T, x^T and dW at its peak (5 blocks: w^T lives until linear_backward returns) - that is the parent commit's
    figure and must not move; with the switch on the three transposed copies are gone (dx and dW remain)."""
    MiB = 1 << 20
    g = torch.Generator(device="cuda").manual_seed(1)
    x, w, dy = ((torch.randn(1024, 1024, generator=g, device="cuda") * 0.1).to(torch.bfloat16) for _ in range(3))
    peaks = {}
    for on in (False, True):
        _backward(train, x, w, dy, None, on, monkeypatch)      # first call outside the measurement (workspaces, attributes)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        dx, dw = _backward(train, x, w, dy, None, on, monkeypatch)
        peaks[on] = torch.cuda.max_memory_allocated() - base
        del dx, dw
    print("peak bytes over the call: off", peaks[False], "on", peaks[True])
    copies = 3 * 1024 * 1024 * 2
    assert peaks[False] == 5 * 2 * MiB
    assert peaks[True] <= peaks[False] - copies + 2 * MiB
