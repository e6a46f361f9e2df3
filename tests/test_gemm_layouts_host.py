"""v3d_gemm_layout without a GPU: the export and its declaration, every refusal of include/v3d.h's rules (all checked before any
device call, so they answer on a machine without one), ops.gemm_layout's shape checks, and the LDS addressing of gemm_layout_kernel
as modelled in tests/gemm_layout_model.py: staging map, row read and transposed read against the 16 x 16 x 32 operand map, alignment of
the transposed reads, and the bank-conflict degrees DESIGN.md section 7 states."""
import ctypes
import os
import re

import pytest
import torch

import gemm_layout_model as model
from v3d import _native, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F16, F32 = 2, 1, 0
EPI_NONE, EPI_BIAS, EPI_RES, EPI_SWIGLU = 0, 1, 5, 6


def test_export_and_declaration():
    lib = _native.lib()
    assert hasattr(lib, "v3d_gemm_layout") and "v3d_gemm_layout" in _native.SIGNATURES
    text = open(os.path.join(ROOT, "include", "v3d.h")).read()
    m = re.search(r"int v3d_gemm_layout\(([^;]*)\);", text)
    assert m, "include/v3d.h does not declare v3d_gemm_layout"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == len(_native.SIGNATURES["v3d_gemm_layout"][1]) == 18
    assert [a.split()[-1].lstrip("*") for a in args] == ["A", "lda", "a_kmajor", "B", "ldb", "b_kmajor", "bias", "res", "ldr", "res_mod", "out", "ldo",
                                                          "M", "N", "K", "dtype", "epilogue", "stream"]
    assert lib.v3d_abi_version() == 7


def _buf():
    raw = (ctypes.c_char * 4096)()
    return raw, (ctypes.addressof(raw) + 15) & ~15


def _call(**kw):
    """One TN call that passes every check up to the launch, with the named arguments replaced."""
    raw, p = _buf()
    a = dict(A=p, lda=256, a_kmajor=1, B=p, ldb=256, b_kmajor=1, bias=None, res=None, ldr=0, res_mod=0, out=p, ldo=256, M=136, N=256, K=70,
             dtype=BF16, epilogue=EPI_NONE, stream=None)
    a.update(kw)
    lib = _native.lib()
    rc = lib.v3d_gemm_layout(a["A"], a["lda"], a["a_kmajor"], a["B"], a["ldb"], a["b_kmajor"], a["bias"], a["res"], a["ldr"], a["res_mod"], a["out"],
                             a["ldo"], a["M"], a["N"], a["K"], a["dtype"], a["epilogue"], a["stream"])
    return rc, lib.v3d_last_error().decode()


REFUSALS = [
    (dict(A=None), "A is a null"),
    (dict(B=None), "B is a null"),
    (dict(out=None), "out is a null"),
    (dict(A="+8"), "A must be 16-byte aligned"),
    (dict(B="+8"), "B must be 16-byte aligned"),
    (dict(out="+8"), "out must be 16-byte aligned"),
    (dict(a_kmajor=2), "a_kmajor"),
    (dict(dtype=F32), "dtype"),
    (dict(M=0), "bad shape"),
    (dict(N=192), "N=192"),
    (dict(lda=128), "lda=128"),                                        # k-major A: lda >= M = 136
    (dict(lda=260), "lda=260"),                                        # not a multiple of 8
    (dict(a_kmajor=0, K=128, lda=64), "lda=64"),                       # K-contiguous A: lda >= K
    (dict(ldb=128), "ldb=128"),                                        # k-major B: ldb >= N = 256
    (dict(b_kmajor=0, K=128, ldb=120), "ldb=120"),
    (dict(ldo=128), "ldo=128"),
    (dict(a_kmajor=0, lda=128), "K=70"),                               # one K-contiguous operand: K % 64
    (dict(b_kmajor=0, ldb=128), "K=70"),
    (dict(M=132), "M=132"),                                            # k-major A: M % 8
    (dict(K=1 << 23, lda=256), "A is larger than 2^31"),
    (dict(a_kmajor=0, M=1 << 22, K=512, lda=512), "A is larger than 2^31"),
    (dict(a_kmajor=0, lda=128, K=128, b_kmajor=0, N=1 << 23, ldb=256), None),      # (0, 0) is v3d_gemm: its own message
    (dict(a_kmajor=0, lda=1 << 22, K=1 << 22, M=8, ldb=1 << 24), "B is larger than 2^31"),
    (dict(epilogue=EPI_BIAS), "epilogue 1"),
    (dict(epilogue=EPI_SWIGLU), "epilogue 6"),
    (dict(epilogue=99), "epilogue 99"),
    (dict(epilogue=EPI_RES), "res"),                                   # no residual given
    (dict(epilogue=EPI_RES, res="p", ldr=128), "res"),                 # ldr < N
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_refusals_name_their_argument(i, monkeypatch):
    monkeypatch.delenv("V3D_GEMM_LAYOUT_TILE", raising=False)
    kw, text = REFUSALS[i]
    raw, p = _buf()
    kw = {k: (p + 8 if v == "+8" else p if v == "p" else v) for k, v in kw.items()}
    rc, msg = _call(**kw)
    assert rc == -1, (kw, rc, msg)
    if text is not None:
        assert msg.startswith("v3d_gemm_layout:") and text in msg, (kw, msg)
    else:
        assert msg.startswith("v3d_gemm:"), msg


def test_forced_tile_must_fit(monkeypatch):
    monkeypatch.setenv("V3D_GEMM_LAYOUT_TILE", "256")
    rc, msg = _call(N=128, ldb=128, ldo=128)
    assert rc == -1 and "V3D_GEMM_LAYOUT_TILE" in msg
    monkeypatch.setenv("V3D_GEMM_LAYOUT_TILE", "64")
    rc, msg = _call()
    assert rc == -1 and "V3D_GEMM_LAYOUT_TILE" in msg


class _Fake:
    """A tensor as ops.gemm_layout's checks see it (they run before the library is called)."""
    is_cuda = True

    def __init__(self, *shape, dtype=torch.bfloat16, inner=1):
        self.shape, self.dtype, self._inner = torch.Size(shape), dtype, inner

    def dim(self):
        return len(self.shape)

    def stride(self, i):
        return self._inner if i in (-1, len(self.shape) - 1) else self.shape[-1]


def test_ops_gemm_layout_rejects_mismatched_shapes():
    with pytest.raises(_native.V3DError, match="HBM"):
        ops.gemm_layout(torch.zeros(8, 64), torch.zeros(128, 64))
    with pytest.raises(_native.V3DError, match="K = 64 but b .* has K = 128"):
        ops.gemm_layout(_Fake(8, 64), _Fake(64, 128))                            # NT reading: b is [N = 64, K = 128]
    with pytest.raises(_native.V3DError, match="K = 200 but b .* has K = 128"):
        ops.gemm_layout(_Fake(200, 256), _Fake(128, 200), a_kmajor=True, b_kmajor=True)
    with pytest.raises(_native.V3DError, match="K = 256 but b .* has K = 200"):
        ops.gemm_layout(_Fake(200, 256), _Fake(200, 128), b_kmajor=True)         # a is K-contiguous: [M = 200, K = 256]
    with pytest.raises(_native.V3DError, match="contiguous last dimension"):
        ops.gemm_layout(_Fake(200, 256, inner=2), _Fake(200, 128), a_kmajor=True, b_kmajor=True)
    with pytest.raises(_native.V3DError, match="a is torch.bfloat16 but b is torch.float16"):
        ops.gemm_layout(_Fake(200, 256), _Fake(200, 128, dtype=torch.float16), a_kmajor=True, b_kmajor=True)


# ------------------------------------------------------------------------------ the addressing model

FORMS = [False, True]


@pytest.mark.parametrize("kmajor", [False, True], ids=["kcontig", "kmajor"])
@pytest.mark.parametrize("operand", ["A", "B"])
@pytest.mark.parametrize("big", FORMS, ids=["t128", "t256"])
def test_every_tile_element_reaches_its_mfma_lane(big, operand, kmajor):
    """The addresses do not depend on the K-step's parity: a stage is the same image at ring offset 0 or STAGE, so one image stands
    for both ring buffers; asserted by reading it at both offsets."""
    g = model.geometry(big)
    image = model.stage_image(big, kmajor)
    rows = g["np"] * 128
    assert sorted(image.values()) == sorted((r, k) for r in range(rows) for k in range(64)), "staging is not a bijection onto the tile"
    seen = set()
    for wave in range(g["waves"]):
        for frag in range(g["mt"] if operand == "A" else 4):
            for ks in range(2):
                want = model.expected_fragment(big, operand, wave, frag, ks)
                for ring in (0, 2 * g["tile"]):                                  # both ring buffers: base + the same offsets
                    shifted = {a + ring: v for a, v in image.items()}
                    assert model.fragment(big, operand, kmajor, wave, frag, ks, shifted, ring) == want, (wave, frag, ks, ring)
                seen |= set(want.values())
    assert len(seen) == rows * 64, "some (row, k) of the tile is read by no wave"


@pytest.mark.parametrize("operand", ["A", "B"])
@pytest.mark.parametrize("big", FORMS, ids=["t128", "t256"])
def test_transposed_reads_are_8_byte_aligned_and_stay_in_their_tile(big, operand):
    g = model.geometry(big)
    for wave in range(g["waves"]):
        for frag in range(g["mt"] if operand == "A" else 4):
            for ks in range(2):
                for lanes in model.read_addresses(big, operand, True, wave, frag, ks):
                    assert all(a % 8 == 0 and 0 <= a <= g["tile"] - 8 for a in lanes)


@pytest.mark.parametrize("big", FORMS, ids=["t128", "t256"])
def test_conflict_degrees_are_the_ones_design_states(big):
    """every fragment read of gemm_layout_kernel is conflict-free by the bank rule - the transposed reads of both
    operands in NN, TN and TK (a 32-lane half takes two blocks 8 k-rows apart in the same 16 columns) and the ds_read_b128 row reads."""
    for operand in "AB":
        assert model.read_conflicts(big, operand, True) == 1
        assert model.read_conflicts(big, operand, False) == 1
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "8 k-rows apart" in text and "conflict-free" in text


def test_the_stacked_alternative_would_be_two_way():
    """The layout NOT built: the two blocks of a half stacked in one aligned 8-row group (group g reading k-rows 4g .. 4g + 3) is 2-way
    under the same rule and XOR - why the natural k order (8 rows apart) is the one in the kernel."""
    lanes = []
    for lane in range(64):
        gq, q, pp = lane >> 4, (lane >> 2) & 3, lane & 3
        row = 4 * gq + q
        lanes.append(256 * row + 16 * ((pp >> 1) ^ (((row & 3) << 2) | ((row >> 2) & 3))) + 8 * (pp & 1))
    assert model.conflict_degree(lanes, 8, model.HALVES) == 2
