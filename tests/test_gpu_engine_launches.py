"""The launches behind every decoder call site of the engine, per weight format (16-bit, e4m3 = llm_fp8, MXFP4 = llm_fp4).

The number and kind of launches per layer is the decode step's speed contract (28 layers x 7 launches are queued per token), and which
call site lets the decode linear form the RMSNorm itself decides bits: the fused and the unfused norm are not bit-equal in the one-row
VALU form.  So the sequence of C entries each call site reaches is pinned here as literals, taken from a run of this file on the code
before the weight format moved behind one object (v3d.linears.Linears) - a change of the host layer must leave every list as it is.

The trace wraps the C entries on the loaded library object and records their names (without the `v3d_` prefix) in call order; queries
(`*_workspace_bytes`, `*_chunk`, `*_fuses_norm`, `*_host`, `v3d_last_error`) are left out.  A decode linear is recorded with its row count
and whether a norm weight was passed; `v3d_linear_decode` forwards to the rows entry with M = 1 and is recorded as such.

The model is the smallest at which every branch is reachable: hidden 1280 = 10 K-tiles, the least at which the fused-norm matrix-core
form applies (9 to 32) - for more than 4 rows, so M = 6 fuses and M = 3 does not; intermediate 384 makes the down projection's
K % 256 = 128, so MXFP4 launches it 4 rows at a time; 10 query heads over 5 K/V heads are groups of 2, a size the one-row decode
attention has (it has none of 5: 1, 2, 4, 7, 8).  For the same reason as MXFP4's 4-row launches the e4m3 decode linear refuses more than 4 rows at that
projection (Engine's docstring): the e4m3 traces of the 6-row group and of the 5-question answer batch end at that refused call.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from v3d import _native, ops  # noqa: E402
from v3d._native import V3DError  # noqa: E402

DEV = "cuda"
FORMATS = {"bf16": {}, "e4m3": {"llm_fp8": True}, "mxfp4": {"llm_fp4": True}}
PHASES = ("prefill_12", "prefill_12_last_row", "prefill_7", "decode_forward", "decode_rows_3", "decode_rows_6", "answer_group_head")
QUERIES = ("_workspace_bytes", "_chunk", "_fuses_norm", "_host")
DEC_ROWS = ("v3d_linear_decode_rows", "v3d_linear_decode_fp8_rows", "v3d_linear_decode_mxfp4_rows")        # (x, ldx, M, ...)


def _config():
    from v3d.engine import EngineConfig, LlmConfig, VitConfig
    return EngineConfig(vit=VitConfig(hidden=144, inter=272, layers=1, heads=2),          # (the one-layer ViT of test_gpu_fp4._tiny())
                        llm=LlmConfig(hidden=1280, inter=384, layers=2, heads=10, kv_heads=5, vocab=320, max_pos=1024))


class Trace:
    """Wraps every C entry of the loaded library (queries apart) and lists the entries a call reaches."""

    def __init__(self, mp):
        self.calls = []
        lib = _native.lib()
        for name in _native.SIGNATURES:
            if not name.endswith(QUERIES) and name != "v3d_last_error":
                mp.setattr(lib, name, self._wrap(name, getattr(lib, name)))

    def _wrap(self, name, real):
        def entry(*a):
            if name == "v3d_linear_decode":                          # (x, norm_weight, ...): the rows entry with M = 1
                rec = "linear_decode_rows M=1" + (" norm" if a[1] is not None else "")
            elif name in DEC_ROWS:
                rec = f"{name[4:]} M={a[2]}" + (" norm" if name == "v3d_linear_decode_rows" and a[3] is not None else "")
            else:
                rec = name[4:]
            self.calls.append(rec)
            return real(*a)
        return entry

    def __call__(self, fn, refused=False):
        """the entries fn() reaches; refused: fn must end in a V3DError (the list then ends with the refused entry)"""
        del self.calls[:]
        if refused:
            with pytest.raises(V3DError, match="activation rows for this shape"):
                fn()
        else:
            fn()
        return list(self.calls)


def trace_format(fmt):
    """{phase: entries} of one engine in the given weight format"""
    from oracle import pipeline_oracle as PO
    from v3d.engine import Engine, random_state_dict
    cfg = _config()
    sd = random_state_dict(cfg, torch.float32, "cpu", seed=5, std=0.05)
    eng = Engine(cfg, sd, dtype=torch.bfloat16, device=DEV, max_frames=1, **FORMATS[fmt])
    g = torch.Generator().manual_seed(6)
    x = (torch.randn(12, cfg.llm.hidden, generator=g) * 0.5).bfloat16().to(DEV)
    images = torch.randn(1, 3, 384, 384, generator=g).to(DEV)
    coords = ((torch.rand(1, 384, 384, 3, generator=g) - 0.5) * 20).to(DEV)
    prefix = torch.cat([torch.randint(0, 320, (14,), generator=g), torch.tensor([PO.IMAGE_TOKEN_INDEX])])
    questions = [torch.randint(0, 320, (n,), generator=g) for n in (9, 4, 7, 5, 6)]
    narrow = fmt == "e4m3"                      # more than 4 rows: refused at the down projection (K % 256 == 128)
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        tr = Trace(mp)
        out["prefill_12"] = tr(lambda: eng.llm_forward(x.clone(), 0))
        out["prefill_12_last_row"] = tr(lambda: eng.llm_forward(x.clone(), 0, last_rows=[11]))
        out["prefill_7"] = tr(lambda: eng.llm_forward(x[:7].clone(), 0))
        tok = x[5:6].clone()
        out["decode_forward"] = tr(lambda: eng.decode_forward(tok, 7))
        ctxs = [eng.new_context() for _ in range(6)]
        for c in ctxs:
            eng.use(c)
            eng.llm_forward(x[:9].clone(), 0, head=False)
        for M in (3, 6):
            grp = eng.new_group(M)
            grp.x[:M].copy_(x[:M])
            out[f"decode_rows_{M}"] = tr(lambda: eng.decode_forward_rows(grp, ctxs[:M], [9] * M), refused=narrow and M > 4)
        eng.use(eng.new_context())
        eng.prefill_scene(prefix, images, coords)
        whole = tr(lambda: eng.answer_group(questions, max_new_tokens=2), refused=narrow)
        torch.cuda.synchronize()
    # the head step: behind the gather of every question's last row (the second gather; the first embeds the questions), up to the
    # first token choice
    at = [i for i, n in enumerate(whole) if n == "embed_gather"][1]
    out["answer_group_head"] = whole[at + 1: whole.index("argmax_rows")]
    return out


_traces = {}


def _trace(fmt):
    if fmt not in _traces:
        _traces[fmt] = trace_format(fmt)
    return _traces[fmt]


# One decoder layer of each kind (the model has two), then the final norm + LM head.  W16 / W8 / W4: the decode linear's entry.
W16, W8, W4 = "linear_decode_rows", "linear_decode_fp8_rows", "linear_decode_mxfp4_rows"
GEMM_LAYER = ["rmsnorm", "gemm", "rope_kv_store", "attention", "gemm", "rmsnorm", "gemm", "gemm"]
Q8_LAYER = {g: ["rmsnorm_quantize_fp8", g, "rope_kv_store", "attention", "quantize_fp8_rows", g, "rmsnorm_quantize_fp8", g, "quantize_fp8_rows", g]
            for g in ("gemm_fp8", "gemm_mxfp4")}


def _rows_layer(qkv, wo, gu, wd):
    """a layer of decode_forward_rows that normalises with rmsnorm() first; wd: the down projection's launches"""
    return ["rmsnorm", qkv, "rope_kv_append_rows", "attention_decode_rows", wo, "rmsnorm", gu] + wd


def _unfused(lin, M):
    return _rows_layer(*[f"{lin} M={M}"] * 3, [f"{lin} M={M}"])


EXPECTED = {
    "bf16": {
        "prefill_12": GEMM_LAYER * 2 + ["rmsnorm", W16 + " M=1"],
        "prefill_12_last_row": GEMM_LAYER + ["rmsnorm", "gemm", "rope_kv_store", "attention_decode", W16 + " M=1", W16 + " M=1 norm", W16 + " M=1"]
        + ["rmsnorm", W16 + " M=1"],
        "prefill_7": GEMM_LAYER * 2 + ["rmsnorm", W16 + " M=1"],
        "decode_forward": [W16 + " M=1 norm", "rope_kv_append", "attention_decode", W16 + " M=1", W16 + " M=1 norm", W16 + " M=1"] * 2
        + ["rmsnorm", W16 + " M=1"],
        "decode_rows_3": _unfused(W16, 3) * 2 + ["rmsnorm", W16 + " M=3"],
        "decode_rows_6": [W16 + " M=6 norm", "rope_kv_append_rows", "attention_decode_rows", W16 + " M=6", W16 + " M=6 norm", W16 + " M=6"] * 2
        + [W16 + " M=6 norm"],
        "answer_group_head": ["rmsnorm", W16 + " M=5"],
    },
    "e4m3": {
        "prefill_12": Q8_LAYER["gemm_fp8"] * 2 + ["rmsnorm", W8 + " M=1"],
        "prefill_12_last_row": Q8_LAYER["gemm_fp8"] + ["rmsnorm_quantize_fp8", "gemm_fp8", "rope_kv_store", "attention_decode", W8 + " M=1", "rmsnorm",
                                                      W8 + " M=1", W8 + " M=1"] + ["rmsnorm", W8 + " M=1"],
        "prefill_7": GEMM_LAYER * 2 + ["rmsnorm", W8 + " M=1"],                       # up to 8 rows: the 16-bit copies
        "decode_forward": _unfused(W8, 1) * 2 + ["rmsnorm", W8 + " M=1"],
        "decode_rows_3": _unfused(W8, 3) * 2 + ["rmsnorm", W8 + " M=3"],
        "decode_rows_6": _unfused(W8, 6),                                             # ends at the refused down projection of layer 0
        "answer_group_head": ["rmsnorm", W8 + " M=5"],
    },
    "mxfp4": {
        "prefill_12": Q8_LAYER["gemm_mxfp4"] * 2 + ["rmsnorm", W16 + " M=1"],
        "prefill_12_last_row": Q8_LAYER["gemm_mxfp4"] + ["rmsnorm_quantize_fp8", "gemm_mxfp4", "rope_kv_store", "attention_decode", W4 + " M=1", "rmsnorm",
                                                        W4 + " M=1", W4 + " M=1"] + ["rmsnorm", W16 + " M=1"],
        "prefill_7": ["rmsnorm", W4 + " M=7", "rope_kv_store", "attention", W4 + " M=7", "rmsnorm", W4 + " M=7", W4 + " M=4", W4 + " M=3"] * 2
        + ["rmsnorm", W16 + " M=1"],
        "decode_forward": _unfused(W4, 1) * 2 + ["rmsnorm", W16 + " M=1"],
        "decode_rows_3": _unfused(W4, 3) * 2 + ["rmsnorm", W16 + " M=3"],
        "decode_rows_6": _rows_layer(*[W4 + " M=6"] * 3, [W4 + " M=4", W4 + " M=2"]) * 2 + [W16 + " M=6 norm"],      # the 16-bit head fuses
        "answer_group_head": ["rmsnorm", W16 + " M=5"],
    },
}


def test_the_fused_norm_form_is_reachable_at_this_width():
    assert ops.linear_decode_rows_fuses_norm(6, 1792, 1280, ops.DEC_BIAS)
    assert not ops.linear_decode_rows_fuses_norm(3, 1792, 1280, ops.DEC_BIAS)


@pytest.mark.parametrize("phase", PHASES)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_launch_sequence(fmt, phase):
    got = _trace(fmt)[phase]
    assert got == EXPECTED[fmt][phase], got
