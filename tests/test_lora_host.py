"""Host half of the LoRA entry points (csrc/lora.hip), no GPU: the ABI number did not move, the library exports what include/v3d.h
declares for them, the chunk and workspace queries are pure functions of the shape, and every argument refusal returns V3D_E_INVALID
from the checks that run before any device call."""
import ctypes
import os
import re

import pytest

from v3d import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LORA = ("v3d_lora_down", "v3d_lora_wgrad", "v3d_lora_wgrad_chunk", "v3d_lora_wgrad_workspace_bytes")
BF16, F32 = 2, 0


def test_abi_is_still_7_and_exports_equal_declarations():
    lib = _native.lib()
    assert lib.v3d_abi_version() == 7 and _native.ABI_VERSION == 7
    text = open(os.path.join(ROOT, "include", "v3d.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(v3d_lora_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(LORA)
    for n in declared:
        assert hasattr(lib, n) and n in _native.SIGNATURES, n
    assert sorted(n for n in _native.SIGNATURES if n.startswith("v3d_lora_")) == sorted(LORA)


def test_chunk_and_workspace_are_pure_and_monotone():
    lib = _native.lib()
    for R, K in ((16, 128), (64, 3584), (192, 4608), (64, 18944), (64, 37888), (384, 64)):
        prev_c, prev_w = 0, 0
        for M in (1, 2, 31, 32, 33, 100, 257, 1000, 2592, 6794, 6795, 50000):
            c, w = lib.v3d_lora_wgrad_chunk(M, R, K), lib.v3d_lora_wgrad_workspace_bytes(M, R, K)
            assert (c, w) == (lib.v3d_lora_wgrad_chunk(M, R, K), lib.v3d_lora_wgrad_workspace_bytes(M, R, K))       # pure
            assert c >= 32 and c % 32 == 0
            n_chunks = -(-M // c)
            assert 1 <= n_chunks <= 512
            assert w >= n_chunks * R * K * 4 and w % (R * K * 4) == 0, "the workspace must hold every slab the launch writes"
            assert c >= prev_c and w >= prev_w, "neither decreases when M grows"
            prev_c, prev_w = c, w
        assert lib.v3d_lora_wgrad_workspace_bytes(6794, R, K) <= lib.v3d_lora_wgrad_workspace_bytes(6794, min(384, R + 16), K)   # nor with R
    # the flagship shape: 56 column slabs x 10 chunks of 704 rows
    assert lib.v3d_lora_wgrad_chunk(6794, 64, 3584) == 704
    assert lib.v3d_lora_wgrad_workspace_bytes(6794, 64, 3584) == 10 * 64 * 3584 * 4
    for bad in ((0, 64, 128), (10, 24, 128), (10, 400, 128), (10, 64, 96), (10, 0, 128), (10, 64, 0)):
        assert lib.v3d_lora_wgrad_chunk(*bad) == 0 and lib.v3d_lora_wgrad_workspace_bytes(*bad) == 0, bad


@pytest.fixture(scope="module")
def host_buffer():
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15
    return buf, p


def _down(p, **kw):
    a = dict(X=p, ldx=128, P=p, ldp=128, scale=1.0, out=p, ldo=64, M=4, R=64, K=128, dtype=BF16)
    a.update(kw)
    return _native.lib().v3d_lora_down(a["X"], a["ldx"], a["P"], a["ldp"], a["scale"], a["out"], a["ldo"], a["M"], a["R"], a["K"], a["dtype"], None)


def _wgrad(p, **kw):
    a = dict(U=p, ldu=64, X=p, ldx=128, scale=1.0, G=p, ldg=128, g_dtype=F32, M=4, R=64, K=128, dtype=BF16, ws=p)
    a.update(kw)
    return _native.lib().v3d_lora_wgrad(a["U"], a["ldu"], a["X"], a["ldx"], a["scale"], a["G"], a["ldg"], a["g_dtype"], a["M"], a["R"], a["K"],
                                        a["dtype"], a["ws"], None)


DOWN_REFUSALS = {
    "R % 16": (dict(R=24, ldo=24), "multiple of 16"),
    "R > 384": (dict(R=400, ldo=400), "up to 384"),
    "K % 64": (dict(K=96), "multiple of 64"),
    "misaligned pointer": (dict(misalign="X"), "16-byte aligned"),
    "ld not a multiple of 8": (dict(ldx=132), "multiples of 8"),
    "ld below the row": (dict(ldo=56), "multiples of 8"),
    "null pointer": (dict(P=None), "null pointer"),
    "f32 operands": (dict(dtype=F32), "16-bit"),
    "M = 0": (dict(M=0), "M=0"),
    "span": (dict(M=1 << 24, ldx=128), "2^31"),
    "span, a huge ld": (dict(M=4, ldx=1 << 62), "2^31"),
}
WGRAD_REFUSALS = {
    "R % 16": (dict(R=24, ldu=24), "multiple of 16"),
    "R > 384": (dict(R=400, ldu=400), "up to 384"),
    "K % 64": (dict(K=96), "multiple of 64"),
    "misaligned pointer": (dict(misalign="U"), "16-byte aligned"),
    "misaligned workspace": (dict(misalign="ws"), "16-byte aligned"),
    "ld not a multiple of 8": (dict(ldg=132), "multiples of 8"),
    "null workspace": (dict(ws=None), "null workspace"),
    "null pointer": (dict(G=None), "null pointer"),
    "output dtype": (dict(g_dtype=5), "output dtype"),
    "M = 0": (dict(M=0), "M=0"),
    "span": (dict(M=1 << 24), "2^31"),
    "span, a huge ld": (dict(M=4, ldg=1 << 62), "2^31"),
}


@pytest.mark.parametrize("case", sorted(DOWN_REFUSALS))
def test_down_refuses_before_any_device_call(host_buffer, case):
    _, p = host_buffer
    kw, text = DOWN_REFUSALS[case]
    kw = dict(kw)
    m = kw.pop("misalign", None)
    if m:
        kw[m] = p + 2
    assert _down(p, **kw) == -1, case                                       # V3D_E_INVALID
    assert text.encode() in _native.lib().v3d_last_error(), (case, _native.lib().v3d_last_error())


@pytest.mark.parametrize("case", sorted(WGRAD_REFUSALS))
def test_wgrad_refuses_before_any_device_call(host_buffer, case):
    _, p = host_buffer
    kw, text = WGRAD_REFUSALS[case]
    kw = dict(kw)
    m = kw.pop("misalign", None)
    if m:
        kw[m] = p + 2
    assert _wgrad(p, **kw) == -1, case
    assert text.encode() in _native.lib().v3d_last_error(), (case, _native.lib().v3d_last_error())
