"""ms per decode step of a beam search with four beams against a four-row greedy decode-group step, in one process, alternating, at the 7B
widths behind the bench scene's prompt (S = 6794 rows, bf16) on one MI355X; and the shares of v3d_beam_topk / v3d_beam_step /
v3d_beam_kv_gather in the beam step.  Both steps run the same decode_forward_rows over four rows that share the prompt's K/V
(shared_prefix = S, read from the context's one cache); the greedy step adds argmax_rows + embed_gather, the beam step the three beam
kernels + embed_gather.

    timeout -k 10 900 python tools/time_beam.py > profiles/beam_search.txt"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "video-3d-llm_amd"))
import bench  # noqa: E402
from v3d import ops  # noqa: E402
from v3d.engine import Engine, EngineConfig, random_state_dict  # noqa: E402

dt, dev = torch.bfloat16, torch.device("cuda:0")
B, STEPS, ROUNDS = 4, 8, 4


def _ms(pairs):
    return sum(a.elapsed_time(b) for a, b in pairs) / len(pairs)


def main():
    cfg = EngineConfig()
    eng = Engine(cfg, random_state_dict(cfg, dt, dev, seed=0), dtype=dt, device=dev, max_frames=bench.FRAMES)
    inp = bench.synth_inputs(dev, dt, seed=1000)
    images, coords = ops.preprocess_rgb(inp["frames"], dt), ops.unproject_sampled(inp["depth"], inp["K"], inp["P"], 384, dt)
    x = eng.build_inputs_embeds(inp["input_ids"], eng.encode_images(images), eng.voxel_ids(coords))
    S = x.shape[0]
    logits0 = eng.llm_forward(x, 0, last_rows=[S - 1]).clone()
    l, scene = cfg.llm, eng.ctx
    st = eng._answer_state(B)
    K, half, rows = 2 * B, st.n // 2, st.rows
    L = STEPS * ROUNDS + 2
    bs = ops.BeamState(B, L, K, l.vocab, (), 1.0, device=dev)
    ptrs = ops.beam_kv_layers(st.kv)
    ev = lambda: torch.cuda.Event(enable_timing=True)        # noqa: E731
    toks = torch.zeros(B, dtype=torch.int64, device=dev)
    t_beam, t_greedy, t_topk, t_step, t_gather = [], [], [], [], []

    def beam_step(t, xin, timed):
        e = [ev() for _ in range(5)]
        e[0].record()
        ops.beam_topk(xin, bs.running, K, bs.cand_score, bs.cand_flat, bs.topk_ws, done=bs.done, V=l.vocab)
        e[1].record()
        ops.beam_step(bs, t)
        e[2].record()
        cur = (t & 1) * half
        if t >= 1:
            ops.beam_kv_gather(st.kv, ptrs, S, t, half - cur, cur, bs.parents, done=bs.done)
        e[3].record()
        ops.embed_gather(eng.embed, bs.next_tokens, out=rows.x[:B])
        out = eng.decode_forward_rows(rows, st.ctxs[cur: cur + B], [S + t] * B, shared_prefix=S, prefix_kv=scene.kv)
        e[4].record()
        if timed:
            t_beam.append((e[0], e[4])); t_topk.append((e[0], e[1])); t_step.append((e[1], e[2])); t_gather.append((e[2], e[3]))
        return out

    def greedy_step(t, xin, timed):
        a, b = ev(), ev()
        a.record()
        ops.argmax_rows(xin, toks, rows.amax_ws)
        ops.embed_gather(eng.embed, toks, out=rows.x[:B])
        out = eng.decode_forward_rows(rows, st.ctxs[8: 8 + B], [S + t] * B, shared_prefix=S, prefix_kv=scene.kv)      # slices no beam uses
        b.record()
        if timed:
            t_greedy.append((a, b))
        return out

    xb = beam_step(0, logits0[None], False)                   # step 0: one row in, four beams out (also the warm-up)
    xg = greedy_step(0, rows.logits[:B, : l.vocab].clone(), False)
    t = 1
    for _ in range(ROUNDS):
        for k in range(STEPS):
            xb = beam_step(t + k, xb, True)
        xg = xb.clone()
        for k in range(STEPS):
            xg = greedy_step(t + k, xg, True)
        t += STEPS
    torch.cuda.synchronize()
    assert int(bs.done.cpu()) == 0, "the search ended inside the timed steps"
    beam, greedy, tk, ts, tg = _ms(t_beam), _ms(t_greedy), _ms(t_topk), _ms(t_step), _ms(t_gather)
    print(f"beam search step, {B} beams (K = {K}), S = {S}, 7B widths, bf16, {len(t_beam)} steps each, alternating in blocks of {STEPS}")
    print(f"  beam step   (topk + step + kv_gather + embed + decode_forward_rows) : {beam:8.3f} ms")
    print(f"  greedy step (argmax_rows + embed + decode_forward_rows, 4 rows)     : {greedy:8.3f} ms    ratio {beam / greedy:.3f}")
    print(f"  v3d_beam_topk      : {tk * 1e3:8.1f} us  = {100 * tk / beam:5.2f} % of the beam step")
    print(f"  v3d_beam_step      : {ts * 1e3:8.1f} us  = {100 * ts / beam:5.2f} %")
    print(f"  v3d_beam_kv_gather : {tg * 1e3:8.1f} us  = {100 * tg / beam:5.2f} %   (own rows 1 .. {t - 1}, 28 layers, one launch)", flush=True)


if __name__ == "__main__":
    with torch.no_grad():
        main()
