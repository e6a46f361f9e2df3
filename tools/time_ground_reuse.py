"""One scene prefill shared by a scene's grounding queries / caption requests, against one full pass per query, at the true shapes on one
MI355X: 32 frames, the 7B widths, 28 layers, 50 proposals, 32 queries of 50 rows behind the 15-row prefix [system | user | <image>] (bf16).

  ground    ScanRefer / Multi3DRefer: per scene, back-projection + RGB preprocessing + Engine.prefill_scene(objects = 50 proposals) +
            ONE Engine.ground_group over the scene's 32 queries -> queries/s (and the ms of each part); the baseline, in the same process:
            Engine.ground_scores on the full prompt of one query at a time (what eval_3d runs without --reuse-scenes).
  caption   Scan2Cap: per scene, the same prefill + ONE Engine.answer_group over 32 caption prompts, each with its own box centre on its
            <coord> row, 32 new tokens each -> captions/s; the baseline, in the same process: Engine.generate(prefix + question, box_input)
            one prompt at a time.

Each step is its own process under its own time limit:
    timeout -k 10 600 python tools/time_ground_reuse.py ground > profiles/ground_reuse.txt && \\
    timeout -k 10 600 python tools/time_ground_reuse.py caption >> profiles/ground_reuse.txt"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "video-3d-llm_amd"))
import bench  # noqa: E402
from v3d import ops  # noqa: E402
from v3d.engine import Engine, EngineConfig, random_state_dict  # noqa: E402

dt, dev = torch.bfloat16, torch.device("cuda:0")
N_QUERIES, Q_ROWS, N_OBJ, GROUND_ROW, COORD_ID, NEW_TOKENS = 32, 50, 50, 40, 151648, 32


def _engine():
    cfg = EngineConfig()
    sd = random_state_dict(cfg, dt, dev, seed=0, ground_head=True)
    return Engine(cfg, sd, dtype=dt, device=dev, max_frames=bench.FRAMES)


def _scene_inputs(inp):
    coords = ops.unproject_sampled(inp["depth"], inp["K"], inp["P"], 384, dt)
    return ops.preprocess_rgb(inp["frames"], dt), coords


def _wall(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def ground(n_scenes=4, n_alone=8):
    eng = _engine()
    scenes = [bench.synth_inputs(dev, dt, seed=1000 + i) for i in range(2)]
    g = torch.Generator(device=dev).manual_seed(777)
    boxes = torch.cat([(torch.rand(N_OBJ, 3, generator=g, device=dev) - 0.5) * torch.tensor([8.0, 8.0, 2.0], device=dev),
                       torch.rand(N_OBJ, 3, generator=g, device=dev) * 2.0 + 0.3], 1)
    queries = [torch.randint(0, 151000, (Q_ROWS,), generator=g, device=dev).cpu() for _ in range(N_QUERIES)]
    rows = [GROUND_ROW] * N_QUERIES
    prefix = lambda inp: inp["input_ids"][: bench.TEXT_PRE + 1]        # noqa: E731

    def reuse(i):
        inp = scenes[i % 2]
        images, coords = _scene_inputs(inp)
        eng.prefill_scene(prefix(inp), images, coords, objects=boxes)
        return eng.ground_group(queries, rows)

    def alone(i):
        inp = scenes[i % 2]
        images, coords = _scene_inputs(inp)
        ids = torch.cat([prefix(inp), queries[i % N_QUERIES]])
        return eng.ground_scores(ids, bench.TEXT_PRE + 1 + GROUND_ROW, images, coords, boxes)

    assert reuse(0).shape == (N_QUERIES, N_OBJ + 1) and alone(0).shape == (N_OBJ + 1,)
    t_reuse = _wall(reuse, n_scenes)
    images, coords = _scene_inputs(scenes[0])
    t_prefill = _wall(lambda i: eng.prefill_scene(prefix(scenes[0]), images, coords, objects=boxes), 2)
    t_plain = _wall(lambda i: eng.prefill_scene(prefix(scenes[0]), images, coords), 2)
    eng.prefill_scene(prefix(scenes[0]), images, coords, objects=boxes)
    t_group = _wall(lambda i: eng.ground_group(queries, rows), 4)
    t_alone = _wall(alone, n_alone)
    print(f"ground  ({bench.FRAMES} frames, {N_OBJ} proposals, {N_QUERIES} queries x {Q_ROWS} rows per scene, bf16)")
    print(f"  one prefill per scene + ground_group : {t_reuse * 1e3:8.1f} ms per scene  = {N_QUERIES / t_reuse:7.1f} queries/s   ({n_scenes} scenes)")
    print(f"      prefill_scene(objects)           : {t_prefill * 1e3:8.1f} ms   (without objects {t_plain * 1e3:.1f} ms)")
    print(f"      ground_group, {N_QUERIES} queries          : {t_group * 1e3:8.1f} ms   = {t_group * 1e3 / N_QUERIES:.2f} ms per query")
    print(f"  ground_scores, one full pass per query: {t_alone * 1e3:8.1f} ms per query = {1 / t_alone:7.1f} queries/s   ({n_alone} queries)")
    print(f"  ratio                                 : {N_QUERIES / t_reuse * t_alone:8.1f} x", flush=True)


def caption(n_scenes=2, n_alone=4):
    eng = _engine()
    scenes = [bench.synth_inputs(dev, dt, seed=1000 + i) for i in range(2)]
    g = torch.Generator(device=dev).manual_seed(778)
    questions = []
    for _ in range(N_QUERIES):
        q = torch.randint(0, 151000, (Q_ROWS,), generator=g, device=dev).cpu()
        q[30] = COORD_ID
        questions.append(q)
    boxes = ((torch.rand(N_QUERIES, 3, generator=g, device=dev) - 0.5) * torch.tensor([8.0, 8.0, 2.0], device=dev)).cpu().tolist()
    prefix = lambda inp: inp["input_ids"][: bench.TEXT_PRE + 1]        # noqa: E731

    def reuse(i):
        inp = scenes[i % 2]
        images, coords = _scene_inputs(inp)
        eng.prefill_scene(prefix(inp), images, coords)
        return eng.answer_group(questions, max_new_tokens=NEW_TOKENS, box_inputs=boxes, coord_token_id=COORD_ID)

    def alone(i):
        inp = scenes[i % 2]
        images, coords = _scene_inputs(inp)
        k = i % N_QUERIES
        return eng.generate(torch.cat([prefix(inp), questions[k]]), images, coords, max_new_tokens=NEW_TOKENS, box_input=torch.tensor([boxes[k]]),
                            coord_token_id=COORD_ID)

    assert len(reuse(0)) == N_QUERIES and alone(0).shape == (NEW_TOKENS,)
    t_reuse = _wall(reuse, n_scenes)
    t_alone = _wall(alone, n_alone)
    print(f"caption ({bench.FRAMES} frames, {N_QUERIES} prompts x {Q_ROWS} rows per scene with one <coord> row each, {NEW_TOKENS} new tokens, bf16)")
    print(f"  one prefill per scene + answer_group(box_inputs): {t_reuse * 1e3:8.1f} ms per scene   = {N_QUERIES / t_reuse:7.1f} captions/s   ({n_scenes} scenes)")
    print(f"  generate(box_input), one full pass per prompt   : {t_alone * 1e3:8.1f} ms per caption = {1 / t_alone:7.1f} captions/s   ({n_alone} prompts)")
    print(f"  ratio                                           : {N_QUERIES / t_reuse * t_alone:8.1f} x", flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what not in ("ground", "caption"):
        raise SystemExit(__doc__)
    with torch.no_grad():
        {"ground": ground, "caption": caption}[what]()
