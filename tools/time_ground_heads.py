"""The 'mlp' / 'score' grounding heads' training cost:
  heads   the head-tail kernels at the 7B model's width (H 3584) for 50 and 200 proposals: v3d_ground_rowdot_bce ('mlp': x = the object
          features [n, 3584]; 'score': x = the scoring MLP's rows [n, 1024]) and v3d_mul_rows_grad [n, 1024] - us per launch by events;
          run under `rocprofv3 --kernel-trace --stats -- python tools/time_ground_heads.py heads` for the profiler's kernel times;
  step    one grounding training step (train.ground_sample_forward_backward: SigLIP 26 layers over bench.py's frames -> projector -> Qwen2-7B
          -> head -> loss -> backward of all of it; no optimizer) per head type, 'infonce' beside 'mlp' and 'score', 50 proposals.
python tools/time_ground_heads.py [heads|step|all] [steps]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "video-3d-llm_amd"))
from v3d import ops, train  # noqa: E402

dt, dev = torch.bfloat16, torch.device("cuda:0")


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def heads(iters=50):
    for n in (50, 200):
        positive, pw = train.ground_bce_targets([1, 7, 30], n)
        positive = positive.to(dev)
        for name, C, rounded in (("mlp", 3584, True), ("score", 1024, False)):
            x = torch.randn(n, C, device=dev, dtype=dt)
            w = torch.randn(C, device=dev, dtype=dt) * C ** -0.5
            b = None if rounded else torch.zeros(1, device=dev, dtype=dt)
            ms = _time(lambda: ops.ground_rowdot_bce(x, w, positive, pw, bias=b, products_rounded=rounded), iters)
            print(f"ground_rowdot_bce ({name:5s}) n={n:4d} C={C:5d} {ms * 1e3:8.1f} us", flush=True)
        o, dm = torch.randn(n, 1024, device=dev, dtype=dt), torch.randn(n, 1024, device=dev, dtype=dt)
        q = torch.randn(1024, device=dev, dtype=dt)
        ms = _time(lambda: ops.mul_rows_grad(dm, o, q), iters)
        print(f"mul_rows_grad           n={n:4d} C= 1024 {ms * 1e3:8.1f} us", flush=True)


def step(steps=2, n_obj=50):
    import bench
    L, H, I, n_q, n_kv, hd, V = 28, 3584, 18944, 28, 4, 128, 152064
    Lv, Hv, Iv, tokens, kpad = 26, 1152, 4304, 729, 640
    width = (n_q + 2 * n_kv) * hd
    mk = lambda *shape, s=1.0: torch.empty(*shape, device=dev, dtype=dt).normal_(0.0, s)     # noqa: E731
    ones = lambda n_: torch.ones(n_, device=dev, dtype=dt)                                    # noqa: E731
    layers = [{"ln1": ones(H), "qkv": mk(width, H, s=H ** -0.5), "qkv_bias": mk(width, s=0.1), "o": mk(H, n_q * hd, s=H ** -0.5),
               "ln2": ones(H), "gate_up": mk(2 * I, H, s=H ** -0.5), "down": mk(H, I, s=I ** -0.5)} for _ in range(L)]

    def vit_layer():
        sd = {"ln1_w": ones(Hv), "ln1_b": mk(Hv, s=0.02), "ln2_w": ones(Hv), "ln2_b": mk(Hv, s=0.02), "o_w": mk(Hv, Hv, s=Hv ** -0.5),
              "o_b": mk(Hv, s=0.02), "fc1_w": mk(Iv, Hv, s=Hv ** -0.5), "fc1_b": mk(Iv, s=0.02), "fc2_w": mk(Hv, Iv, s=Iv ** -0.5), "fc2_b": mk(Hv, s=0.02)}
        for n_ in ("q", "k", "v"):
            sd[n_ + "_w"], sd[n_ + "_b"] = mk(Hv, Hv, s=Hv ** -0.5), mk(Hv, s=0.02)
        return train.siglip_pad_layer(sd)

    patch_w = mk(Hv, kpad, s=588 ** -0.5)
    patch_w[:, 588:] = 0
    F_ = bench.FRAMES
    base = {"vision": {"patch_w": patch_w, "patch_b": mk(Hv, s=0.02), "pos": mk(tokens, Hv, s=0.02), "layers": [vit_layer() for _ in range(Lv)]},
            "projector": {"w1": mk(H, Hv, s=Hv ** -0.5), "b1": mk(H, s=0.02), "w2": mk(H, H, s=H ** -0.5), "b2": mk(H, s=0.02)},
            "newline": mk(H, s=0.02), "embed": mk(V, H, s=0.02), "llm": {"layers": layers, "norm": ones(H)}}

    def head(i, o, out):
        return {"w0": mk(o, i, s=i ** -0.5), "b0": mk(o, s=0.02), "ln_w": ones(o), "ln_b": mk(o, s=0.02), "w3": mk(out, o, s=o ** -0.5), "b3": mk(out, s=0.02)}
    grounds = {"infonce": {"obj": head(H, H, H), "query": head(H, H, H), "zero_target": mk(H)}, "mlp": {"head": head(H, H, H)},
               "score": {"obj": head(H, 1024, 1024), "query": head(H, 1024, 1024), "score": head(1024, 1024, 1)}}
    rope = train.RopeTables(hd, 8192, 1e6, dt, dev)
    table = ops.Sin3DTable(H, 512, dt, dev)
    patches = mk(F_ * tokens, kpad)
    patches[:, 588:] = 0
    ids = torch.randint(0, 512, (F_, 14, 14, 3), device=dev, dtype=torch.int32)
    pre_ids, post_ids = torch.randint(0, V, (bench.TEXT_PRE,), device=dev), torch.randint(0, V, (bench.TEXT_POST,), device=dev)
    ground_row = bench.TEXT_PRE + F_ * 210 + bench.TEXT_POST - 2
    mask = (torch.rand(n_obj, F_ * tokens, device=dev) < 0.01).to(torch.uint8)
    box_pe = mk(n_obj, H, s=0.5)
    for kind in ("infonce", "mlp", "score"):
        params = dict(base, ground=grounds[kind])
        if kind == "infonce":
            positive, kw = torch.zeros(n_obj + 1, dtype=torch.uint8), {}
            positive[[1, 7]] = 1
        else:
            positive, pw = train.ground_bce_targets([1, 7], n_obj)
            kw = {"pos_weight": pw}
        positive = positive.to(dev)
        run = lambda: train.ground_sample_forward_backward(params, patches, ids, table, pre_ids, post_ids, ground_row, mask, box_pe, positive,  # noqa: E731
                                                           rope, F_, n_q, n_kv, hd, head_type=kind, **kw)
        ms = _time(run, steps)
        loss = float(run()[0])
        print(f"grounding step ({kind:7s}, {n_obj} proposals, S = {bench.TEXT_PRE + F_ * 210 + bench.TEXT_POST}): {ms:8.1f} ms   loss {loss:.4f}",
              flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what in ("heads", "all"):
        heads()
    if what in ("step", "all"):
        step(int(sys.argv[2]) if len(sys.argv) > 2 else 2)
