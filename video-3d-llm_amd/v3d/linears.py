"""The Qwen2 decoder's weight format behind one object: 16-bit, e4m3 (Engine(llm_fp8=True): L[key + "8"] = (codes, row scales) beside the
16-bit L[key]) or MXFP4 (llm_fp4: L[key + "4"] = (codes, exponents) INSTEAD of L[key]; the LM head stays 16-bit).  `Linears` is all that
knows which after construction: the engine's call sites name a layer dict, a key and an epilogue, and say where one site's launches
differ from another's (`fuse`).  Every ops function is looked up when it is called."""
import weakref

from . import ops

KEYS = ("wqkv", "wo", "wgu", "wd")
_DEC_EPI = {ops.EPI_BIAS: ops.DEC_BIAS, ops.EPI_RES: ops.DEC_RES, ops.EPI_SWIGLU: ops.DEC_SWIGLU}


class Linears:
    def __init__(self, eng):
        self.eng = weakref.proxy(eng)      # (no cycle: dropping the engine frees its memory at once)
        self.fmt = "e4m3" if eng.llm_fp8 else "mxfp4" if eng.llm_fp4 else None      # None: 16-bit
        self.eps = eng.cfg.llm.eps

    # ------------------------------------------------------------------ construction
    def quantize_layer(self, L):
        """the quantised images of a layer's four matrices"""
        if self.fmt == "e4m3":
            for k in KEYS:
                L[k + "8"] = ops.quantize_fp8_rows(L[k])
        elif self.fmt == "mxfp4":
            for k in KEYS:
                L[k + "4"] = ops.quantize_mxfp4_rows(L.pop(k))        # the 16-bit copy is dropped: nothing reads it again

    def quantize_head(self):
        """(re-)quantise the LM head, eng.l_head -> eng.l_head8: e4m3 only"""
        if self.fmt == "e4m3":
            self.eng.l_head8 = ops.quantize_fp8_rows(self.eng.l_head)

    # ------------------------------------------------------------------ prefill: S rows through a GEMM
    def prefill(self, a, L, key, out, ln=None, stamp=None, **kw):
        """out = a [S, K] - with ln: RMSNorm(a; ln) - through L[key]; kw: bias / res / epilogue as ops.gemm takes them.
        A quantised engine uses the e4m3-activation GEMMs (W8A8 / W4A8) for more than 8 rows only: the rows are quantised first, in one
        pass with the norm (the 16-bit normed rows are never stored).  Up to 8 rows an e4m3 engine runs the 16-bit GEMM on the 16-bit
        copies it keeps; an MXFP4 engine has none and runs the W4A16 decode linears, the epilogue mapped.
        stamp (bench: HIP events): a callable that wraps exactly the GEMM launch - the norm / quantisation pass stays outside it."""
        eng, S = self.eng, a.shape[0]
        if self.fmt and S > 8:
            q8, s8 = eng.l_q8[:S, : a.shape[1]], eng.l_s8[:S]
            if ln is None:
                ops.quantize_fp8_rows(a, q8, s8)
            else:
                ops.rmsnorm_quantize_fp8(a, ln, self.eps, q8, s8)
            gemm, w = (ops.gemm_mxfp4, L[key + "4"]) if self.fmt == "mxfp4" else (ops.gemm_fp8, L[key + "8"])
            args = (q8, s8, *w, eng.dtype)
        else:
            if ln is not None:
                a = ops.rmsnorm(a, ln, self.eps, out=eng.l_h[:S])
            if self.fmt == "mxfp4":                  # (no GEMM runs, so nothing is stamped)
                kw["epilogue"] = _DEC_EPI.get(kw.get("epilogue"), ops.DEC_NONE)
                return self.rows(a, L, key, out, **kw)
            gemm, args = ops.gemm, (a, L[key])
        if stamp is None:
            return gemm(*args, out=out, **kw)
        return stamp(lambda: gemm(*args, out=out, **kw))

    # ------------------------------------------------------------------ decode form: M <= 32 rows, the weights streamed once
    # A decode linear runs on the 16-bit L[key] where the format keeps one to run on: e4m3 keeps 16-bit copies (for short prefills) but
    # streams the codes; an MXFP4 layer holds no 16-bit matrix, the MXFP4 engine's LM head is one.
    def rows(self, a, L, key, out, **kw):
        """out = a [M, K] through L[key] with 16-bit activations (W16 / W8A16 / W4A16); kw: bias / res / epilogue (ops.DEC_*)"""
        w = None if self.fmt == "e4m3" else L.get(key)
        if w is not None:
            return ops.linear_decode_rows(a, w, out, **kw)
        if self.fmt == "e4m3":
            return ops.linear_decode_fp8_rows(a, *L[key + "8"], out, **kw)
        q, e = L[key + "4"]
        M = a.shape[0]
        if M <= 4 or q.shape[1] % 128 == 0:          # K % 256 == 0: one launch (matrix-core form for 2..32 rows)
            return ops.linear_decode_mxfp4_rows(a, q, e, out, **kw)
        res = kw.pop("res", None)                    # VALU form: 4 rows per launch; a row's bits do not depend on its group
        for m in range(0, M, 4):
            ops.linear_decode_mxfp4_rows(a[m: m + 4], q, e, out[m: m + 4], res=None if res is None else res[m: m + 4], **kw)
        return out

    def norm_rows(self, x, ln, L, key, out, h, fuse, **kw):
        """out = RMSNorm(x [M, K]; ln) through L[key], decode form.  fuse is the call site's rule for 16-bit weights - True: the linear
        forms the norm itself (one row: the VALU form, whose bits are NOT those of rmsnorm() + linear), None: it does iff
        ops.linear_decode_rows_fuses_norm says so (more than four rows, matrix-core form: the bits of rmsnorm() + linear), False: never.
        The quantised linears never do.  Unfused, the normed rows go to h."""
        w = None if self.fmt == "e4m3" else L.get(key)
        if w is not None:
            if fuse is None:
                fuse = ops.linear_decode_rows_fuses_norm(x.shape[0], w.shape[0], w.shape[1], kw.get("epilogue", ops.DEC_NONE))
            if fuse:
                return ops.linear_decode_rows(x, w, out, norm_weight=ln, eps=self.eps, **kw)
        ops.rmsnorm(x, ln, self.eps, out=h)
        return self.rows(h, L, key, out, **kw)

    def head(self, x, last, logits, fuse=False):
        """final RMSNorm + LM head over the M rows of x: logits [M, padded vocab]; the normed rows go to `last` unless the linear forms
        the norm (fuse: as norm_rows).  Only e4m3 has a quantised head; an MXFP4 engine's is 16-bit and takes the 16-bit rule."""
        eng = self.eng
        return self.norm_rows(x, eng.l_norm, {"head": eng.l_head, "head8": getattr(eng, "l_head8", None)}, "head", logits, last, fuse)
