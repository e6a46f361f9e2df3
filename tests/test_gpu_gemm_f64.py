"""Every v3d_gemm kernel and epilogue, per element, against the f64 reference and bound of tests/gemm_check.py.

Every case: the output lives in a larger buffer pre-filled with NaN (an element never written fails), with guard rows after M and guard
columns after N (N / 2 for SwiGLU) holding a sentinel that must come back untouched; the whole [M, N] block is compared, on the
device; every case is launched twice and must repeat bit for bit.  Three input families: *random* under the bound, *exact* (integer
sums: the answer is known bit for bit, whatever the tile, the k order or the split-K tail) with torch.equal for NONE / BIAS / BIAS_RES /
RES / BIAS_RELU and the function-error interval for the GELUs and SwiGLU, *gather* (one-hot rows) with torch.equal.

Measured on one MI355X (both dtypes, 68 tests, 1090 compared launches): worst |err| / bound on random inputs 0.992 (bf16) / 0.989 (f16),
both at K = 64, EPI_NONE, where the bound is almost only the output rounding h |y| (a result that sits next to a rounding boundary
has ratio -> 1; the CPU emulation gives the same 0.992); at the product shapes 0.99 (SigLIP, K = 640 / 1152) falling to 0.72 (bf16) /
0.36 (f16) at K = 18 944.  exact: 0 unequal of every bit-for-bit case, 0 outside the interval for the GELUs and SwiGLU; gather: 0.
Wall time of the file: 7 s (the f64 references run on the device).
Activations over the 16-bit grid (test_activation_function_error): C_FUNC needed 0.24 (gelu_erf, at x = -3.9 / -5.3, the cancelling
tail: got -3.19e-7 for -2.43e-7 in bf16), 0.63 (gelu_tanh), 0.08 (silu), in the units of gemm_check.func_err; C_FUNC = 4.
"""
import ctypes

import pytest
import torch

import gemm_check as gc
from gemm_check import (EPI_BIAS, EPI_BIAS_GELU_ERF, EPI_BIAS_GELU_TANH, EPI_BIAS_RELU, EPI_BIAS_RES, EPI_NONE, EPI_RES, EPI_SWIGLU)

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
SENT = 7.0
GUARD_ROWS, GUARD_COLS = 8, 64
ENV_NAMES = ("V3D_GEMM_VARIANT", "V3D_GEMM_PP", "V3D_GEMM_PP_GRID", "V3D_GEMM_STREAMK")
ACTS = (EPI_BIAS_GELU_ERF, EPI_BIAS_GELU_TANH, EPI_SWIGLU)

# kernel name -> environment (anything not named is removed)
KERNELS = {
    "k128": {"V3D_GEMM_VARIANT": "1"},
    "v3_256": {"V3D_GEMM_VARIANT": "3", "V3D_GEMM_PP": "0"},
    "v3_192": {"V3D_GEMM_VARIANT": "4", "V3D_GEMM_PP": "0"},
    "pp_256": {"V3D_GEMM_VARIANT": "3", "V3D_GEMM_PP": "1", "V3D_GEMM_STREAMK": "0"},
    "pp_192": {"V3D_GEMM_VARIANT": "4", "V3D_GEMM_PP": "1", "V3D_GEMM_STREAMK": "0"},
    "pp_grid3": {"V3D_GEMM_VARIANT": "3", "V3D_GEMM_PP": "1", "V3D_GEMM_STREAMK": "0", "V3D_GEMM_PP_GRID": "3"},
    "default": {},
}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from v3d import ops as _ops
    return _ops


def set_env(monkeypatch, env):
    for n in ENV_NAMES:
        monkeypatch.delenv(n, raising=False)
    for n, v in env.items():
        monkeypatch.setenv(n, v)


def bits(t):
    return t.contiguous().view(torch.int16)


def launch(ops, a, w, b, r, epi, res_mod=0, inplace=False):
    """One launch into a NaN-filled, sentinel-guarded buffer -> (out view [M, n_out], the whole buffer).  inplace: the buffer's block
    starts as the residual and is passed as res and out at once (the engine's res = x, out = x)."""
    M, N = a.shape[0], w.shape[0]
    no = gc.n_out(N, epi)
    buf = torch.full((M + GUARD_ROWS, no + GUARD_COLS), float("nan"), dtype=a.dtype, device=a.device)
    buf[M:] = SENT
    buf[:, no:] = SENT
    out = buf[:M, :no]
    res = r if epi in gc.HAS_RES else None
    if inplace:
        out.copy_(r[:M, :no])
        res = out
    ops.gemm(a, w, bias=b if epi in gc.HAS_BIAS else None, res=res, epilogue=epi, out=out, res_mod=res_mod)
    torch.cuda.synchronize()
    return out, buf


def run(ops, a, w, b, r, epi, res_mod=0, inplace=False):
    """Two launches, bit-equal, guards untouched -> out."""
    M = a.shape[0]
    no = gc.n_out(w.shape[0], epi)
    out, buf = launch(ops, a, w, b, r, epi, res_mod, inplace)
    assert bool((buf[M:] == SENT).all()), "rows past M were written"
    assert bool((buf[:M, no:] == SENT).all()), "columns past N were written"
    out2, buf2 = launch(ops, a, w, b, r, epi, res_mod, inplace)
    assert torch.equal(bits(buf), bits(buf2)), "two launches of the same case differ"
    return out


def check(ops, tag, family, a, w, b, r, epi, res_mod=0, inplace=False):
    """Run and compare; random: under the bound; exact: bit for bit (interval for the activations) and under the bound as well."""
    out = run(ops, a, w, b, r, epi, res_mod, inplace)
    c = gc.compare(out, a, w, b, r, epi, res_mod, exact=family == "exact")
    print(f"GEMMCHK {family} {tag} {gc.EPI_NAMES[epi]} {str(a.dtype)[6:]} M={a.shape[0]} N={w.shape[0]} K={a.shape[1]} ratio {c['ratio']:.3f} "
          f"unequal {c['unequal']} outside {c['outside']} needs_rounding {c['needs_rounding']:.2f}")
    assert c["ratio"] <= 1.0, f"{tag} {family} {gc.EPI_NAMES[epi]}: worst |err| / bound = {c['ratio']}"
    if family == "exact":
        if epi in gc.EXACT_EPIS:
            assert c["unequal"] == 0, f"{tag} {gc.EPI_NAMES[epi]}: {c['unequal']} outputs differ from round(exact)"
        else:
            assert c["outside"] == 0, f"{tag} {gc.EPI_NAMES[epi]}: {c['outside']} outputs outside the function-error interval"
    return c


def make(family, M, N, K, dt, epi, seed=0, res_rows=None):
    if family == "random":
        return gc.random_inputs(M, N, K, dt, seed=seed, device="cuda", res_rows=res_rows)
    return gc.exact_inputs(M, N, K, dt, seed=seed, device="cuda", target=2.0 if epi in ACTS else None, res_rows=res_rows)


def check_gather(ops, M, N, K, dt, stride, shift, transposed=False):
    a, w, want = gc.gather_inputs(M, N, K, dt, stride=stride, shift=shift, device="cuda", transposed=transposed)
    out = run(ops, a, w, None, None, EPI_NONE)
    assert torch.equal(out, want), gc.gather_explain(out, a, w, want, transposed)


# ------------------------------------------------------------------------------ kernel x epilogue x dtype


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("kernel", ["k128", "v3_256", "v3_192", "pp_256", "pp_192", "pp_grid3"])
def test_every_epilogue_on_every_tile_kernel(ops, kind, kernel, monkeypatch):
    """M = 300 (a partial last tile for every tile height), N = 512, K = 320 (5 K-steps); BIAS_RES once more with res_mod."""
    set_env(monkeypatch, KERNELS[kernel])
    dt = DT[kind]
    M, N, K = 300, 512, 320
    for epi in range(8):
        for family in ("random", "exact"):
            a, w, b, r = make(family, M, N, K, dt, epi, seed=epi)
            check(ops, kernel, family, a, w, b, r, epi)
    for family in ("random", "exact"):
        a, w, b, r = make(family, M, N, K, dt, EPI_BIAS_RES, seed=11, res_rows=7)
        check(ops, kernel + "/res_mod", family, a, w, b, r, EPI_BIAS_RES, res_mod=7)
    for shift in (0, 160):                    # two launches of 300 consecutive k0: every k of every K-step is some row's k0
        check_gather(ops, M, N, K, dt, stride=1, shift=shift)
    check_gather(ops, M, N, K, dt, stride=5, shift=2, transposed=True)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("M", [1, 8])
def test_every_epilogue_on_the_gemv(ops, kind, M, monkeypatch):
    set_env(monkeypatch, {})
    dt = DT[kind]
    for N, K in ((256, 320), (384, 3584)):
        for epi in range(8):
            for family in ("random", "exact"):
                a, w, b, r = make(family, M, N, K, dt, epi, seed=epi + M)
                check(ops, "gemv", family, a, w, b, r, epi)
        a, w, b, r = make("exact", M, N, K, dt, EPI_BIAS_RES, seed=3, res_rows=3)
        check(ops, "gemv/res_mod", "exact", a, w, b, r, EPI_BIAS_RES, res_mod=3)
        check_gather(ops, M, N, K, dt, stride=77, shift=5)
        check_gather(ops, M, N, K, dt, stride=5, shift=2, transposed=True)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("M,N,grid,cut", [(300, 1024, "16", 2), (300, 1024, "24", 3), (300, 1024, "32", 4), (1025, 2048, "32", 4)])
def test_every_epilogue_on_the_split_k_tail(ops, kind, M, N, grid, cut, monkeypatch):
    """V3D_GEMM_STREAMK=2 (wherever legal) on small grids: 8 tiles on 16 / 24 / 32 workgroups are cut 2 / 3 / 4 ways (the whole launch is
    the tail); 40 tiles on 32 workgroups run one whole-tile round and a 4-way tail.  K = 1024: 16 K-steps, two granules per chunk."""
    set_env(monkeypatch, {"V3D_GEMM_VARIANT": "3", "V3D_GEMM_PP": "1", "V3D_GEMM_STREAMK": "2", "V3D_GEMM_PP_GRID": grid})
    dt = DT[kind]
    K = 1024
    tiles = ((M + 255) // 256) * (N // 256)
    g = int(grid)
    assert min(4, g // (tiles % g)) == cut          # the launcher's sk_plan for this shape
    for epi in range(8):
        for family in ("random", "exact"):
            a, w, b, r = make(family, M, N, K, dt, epi, seed=epi + cut)
            check(ops, f"pp_sk{cut}", family, a, w, b, r, epi)
    for shift in range(0, K, 256):            # every k of every chunk is some row's k0
        check_gather(ops, M, N, K, dt, stride=1, shift=shift)


# ------------------------------------------------------------------------------ edges


EDGE_M = (9, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 513)
SMALL_K = (64, 128, 192, 256)
EXACT_ROT = (EPI_NONE, EPI_BIAS, EPI_BIAS_RES, EPI_RES, EPI_BIAS_RELU)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("kernel", ["k128", "v3_256", "v3_192", "pp_256", "pp_192"])
def test_edges_of_m_with_a_short_and_a_long_k(ops, kind, kernel, monkeypatch):
    """Each M around the tile heights (128, 192, 256) with one short K (64: one K-step, which the ping-pong kernel hands to v3; 128;
    192; 256) and one long K (3584; 18 944 for three of them), N = 256 and 4608 (128 and 384 on the 128 x 128 kernel: N % 256 != 0
    forces it), epilogues in rotation; exact inputs bit for bit, random ones under the bound."""
    set_env(monkeypatch, KERNELS[kernel])
    dt = DT[kind]
    for i, M in enumerate(EDGE_M):
        ks = SMALL_K[i % 4]
        kl = 18944 if M in (9, 257, 513) else 3584
        ns = (128, 384)[i % 2] if kernel == "k128" else 256
        nl = 4608 if M in (129, 256) else 256
        for (N, K) in ((ns, ks), (nl, kl)):
            epi = EXACT_ROT[(i + (K > 256)) % 5]
            a, w, b, r = make("exact", M, N, K, dt, epi, seed=M)
            check(ops, kernel + "/edge", "exact", a, w, b, r, epi)
            epi = (i + (K > 256)) % 8
            a, w, b, r = make("random", M, N, K, dt, epi, seed=M)
            check(ops, kernel + "/edge", "random", a, w, b, r, epi)


# ------------------------------------------------------------------------------ strides and aliasing


def padded(t, pad):
    """The same values as a view into a wider buffer (row stride + pad, the pad columns NaN: reading them would show)."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, : t.shape[1]] = t
    return buf[:, : t.shape[1]]


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("kernel", ["k128", "pp_256", "v3_256", "pp_192"])
def test_all_four_leading_dimensions_and_in_place_residual(ops, kind, kernel, monkeypatch):
    """lda > K, ldw > K, ldr > N and ldo > N together (the pads hold NaN), then out aliasing res (the engine's res = x, out = x), twice
    from the same start; BIAS_RES and RES, exact inputs bit for bit and random ones under the bound."""
    set_env(monkeypatch, KERNELS[kernel])
    dt = DT[kind]
    M, N, K = 700, 512, 448
    for family in ("exact", "random"):
        for epi in (EPI_BIAS_RES, EPI_RES, EPI_BIAS_GELU_TANH):
            a, w, b, r = make(family, M, N, K, dt, epi, seed=5)
            a, w, r = padded(a, 64), padded(w, 72), padded(r, 8)
            assert a.stride(0) > K and w.stride(0) > K and r.stride(0) > N
            check(ops, kernel + "/strided", family, a, w, b, r, epi)
            if epi in gc.HAS_RES:
                check(ops, kernel + "/inplace", family, a, w, b, r, epi, inplace=True)


# ------------------------------------------------------------------------------ product shapes, default environment


def plan(M, N, K, slots=256):
    from v3d import _native
    out = [ctypes.c_int(0) for _ in range(4)]
    rc = _native.lib().v3d_gemm_plan_host(M, N, K, slots, *[ctypes.byref(o) for o in out])
    assert rc == 0
    return tuple(o.value for o in out)            # kernel (0 GEMV, 1 128 x 128, 2 256-row, 3 192-row), tiles, whole rounds before the tail, split


T_VIT, S_LLM = 23328, 6794          # 32 frames x 729 patches; the benchmark's prefill length
# name: (M, N, K, epilogue, res_mod, in place, pad of A's row stride, the plan on 256 CUs: kernel, split)
PRODUCT = {
    "siglip_patch_embed_res_mod": (T_VIT, 1152, 640, EPI_BIAS_RES, 729, False, 0, (1, 1)),
    "siglip_1152_in_place": (T_VIT, 1152, 1152, EPI_BIAS_RES, 0, True, 0, (1, 1)),
    "siglip_out_proj_in_place": (T_VIT, 1280, 1152, EPI_BIAS_RES, 0, True, 0, (2, 1)),
    "siglip_fc1_gelu_tanh": (T_VIT, 4352, 1152, EPI_BIAS_GELU_TANH, 0, False, 128, (2, 1)),
    "siglip_fc2_in_place": (T_VIT, 1280, 4352, EPI_BIAS_RES, 0, True, 64, (2, 1)),
    "projector_gelu_erf": (T_VIT, 3584, 1152, EPI_BIAS_GELU_ERF, 0, False, 128, (2, 1)),
    "qwen2_qkv": (S_LLM, 4608, 3584, EPI_BIAS, 0, False, 0, (2, 1)),
    "qwen2_o_proj": (S_LLM, 3584, 3584, EPI_RES, 0, True, 0, (3, 1)),
    "qwen2_down_proj": (S_LLM, 3584, 18944, EPI_RES, 0, True, 0, (2, 2)),
    "qwen2_gate_up": (S_LLM, 37888, 3584, EPI_SWIGLU, 0, False, 0, (2, 1)),
    "ground_head_relu": (100, 3584, 3584, EPI_BIAS_RELU, 0, False, 0, (1, 1)),
    "dw_siglip_fc1": (4352, 1280, 23424, EPI_NONE, 0, False, 0, (2, 3)),
}


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("name", list(PRODUCT))
def test_product_shapes_with_the_default_environment(ops, kind, name, monkeypatch):
    """The shapes the engine and the training step launch, as they launch them (in place, res_mod, A a strided view), with no variant
    forced; the plan of the cost model is asserted first, so a change that moves a product shape onto another kernel fails here."""
    set_env(monkeypatch, {})
    M, N, K, epi, res_mod, inplace, apad, (kernel, split) = PRODUCT[name]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    got = plan(M, N, K, 256)
    assert (got[0], got[3]) == (kernel, split), f"{name}: the cost model now plans {got}"
    if cus != 256:
        print(f"GEMMCHK note: {cus} CUs, the launch is planned as {plan(M, N, K, cus)}")
    dt = DT[kind]
    for family in ("exact", "random"):
        a, w, b, r = make(family, M, N, K, dt, epi, seed=len(name), res_rows=res_mod or None)
        if apad:
            a = padded(a, apad)
        check(ops, name, family, a, w, b, r, epi, res_mod=res_mod, inplace=inplace)


# ------------------------------------------------------------------------------ the activations' own error


def _needed(got, v, unit, dt):
    """Smallest c with got in [round(v - c unit), round(v + c unit)], per element (f64 tensors; got, round(v) normal 16-bit numbers)."""
    p = 8 if dt == torch.bfloat16 else 11
    r = gc.rnd(v, dt)
    _, ex = torch.frexp(r.abs())
    ulp = torch.exp2((ex - p).double())
    one_step = (got - r).abs() <= 1.001 * ulp                       # got is r's neighbour: the boundary between them is their mean (exact)
    need = torch.where(one_step, ((r + got) / 2 - v).abs(), (got - v).abs()) / unit
    return torch.where(got == r, torch.zeros_like(need), need)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_activation_function_error(ops, kind, monkeypatch):
    """gelu_erf, gelu_tanh and silu of gemm.hip over the whole 16-bit grid with |x| <= 16 (one-hot A, so the linear output IS the grid
    value), against the f64 functions: the smallest C_FUNC that explains every output must leave the margin of 2 that gemm_check.C_FUNC
    = 4 claims.  Outputs below the normal range of the dtype (f16) or 2^-100 (bf16) are left to the bound's absolute terms."""
    set_env(monkeypatch, {})
    dt = DT[kind]
    grid = torch.arange(65536, device="cuda").sub(32768).to(torch.int16).view(dt).reshape(256, 256)
    x = torch.where(torch.isfinite(grid) & (grid.abs() <= 16), grid, torch.zeros_like(grid))
    a = torch.eye(256, dtype=dt, device="cuda")
    zero = torch.zeros(256, dtype=dt, device="cuda")
    xd = x.double().T                                            # out[m, n] = f(x[n, m])
    floor = 2.0 ** -14 if dt == torch.float16 else 2.0 ** -100
    failed = []
    for name, epi, f in (("erf", EPI_BIAS_GELU_ERF, gc.gelu_erf), ("tanh", EPI_BIAS_GELU_TANH, gc.gelu_tanh), ("silu", EPI_SWIGLU, gc.silu)):
        w = ops.interleave_gate_up(x, torch.ones_like(x)) if epi == EPI_SWIGLU else x
        got = run(ops, a, w, zero, None, epi).double()
        v = f(xd)
        unit = (gc.func_err(xd, name) - gc.FTZ) / gc.C_FUNC
        need = _needed(got, v, unit, dt)
        need = torch.where(v.abs() >= floor, need, torch.zeros_like(need))
        worst = need.max().item()
        at = xd.flatten()[need.argmax()].item()
        i = need.argmax()
        print(f"GEMMCHK function_error {name} {kind}: C_FUNC needed {worst:.3f} at x = {at} (got {got.flatten()[i].item()!r}, f64 {v.flatten()[i].item()!r}; "
              f"{int((need > 2).sum())} grid points need more than 2)")
        failed += [f"{name}: measured {worst} at x = {at}"] if 2.0 * worst > gc.C_FUNC else []
    assert not failed, f"C_FUNC = {gc.C_FUNC} no longer leaves a margin of 2: {failed}"
