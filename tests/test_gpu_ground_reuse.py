"""One scene prefill for ScanRefer / Multi3DRefer queries and Scan2Cap captions: v3d_ground_scores_rows and v3d_add_rows bit for bit against
the one-query / one-row entries, Engine.question_embeds (box-centre PEs inside a batch of question rows), Engine.ground_group against the CPU
oracle on the tiny model and against an f64 reference at the 7B widths, and Engine.answer_group with boxes against generate()."""
import gc

import pytest
import torch

import answer_check as ac
from oracle import llm_oracle as L
from oracle import pipeline_oracle as PO

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
SCORE_TOL = {torch.bfloat16: 4e-2, torch.float16: 6e-3}          # tests/test_gpu_engine.py::test_scene_grounding_matches_oracle, for these cosines
COORD = 317
IMG = PO.IMAGE_TOKEN_INDEX


@pytest.fixture
def ops():
    from v3d import ops as o
    return o


# ------------------------------------------------------------------ the two entries


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("G", [1, 3, 32])
@pytest.mark.parametrize("n", [1, 9])
@pytest.mark.parametrize("C", [1000, 3584])
def test_ground_scores_rows_equals_one_query_launches(ops, C, n, G, dt):
    """Row g of v3d_ground_scores_rows carries the bits of v3d_ground_scores on query g: C = 1000 (no multiple of 256 or 64) and 3584, row
    strides larger than C for both operands, one all-zero object row (the 1e-12 clamp on its norm) wherever there is more than one row."""
    g = torch.Generator().manual_seed(100 * C + 10 * n + G)
    obj = torch.randn(n, C + 24, generator=g).to(dt)
    if n > 1:
        obj[n // 2] = 0
    q = (torch.randn(G, C + 40, generator=g) * 3).to(dt)
    obj, q = obj.cuda()[:, :C], q.cuda()[:, :C]
    assert obj.stride(0) > C and q.stride(0) > C
    got = ops.ground_scores_rows(obj, q)
    assert got.shape == (G, n) and got.dtype == dt
    for k in range(G):
        want = ops.ground_scores(obj, q[k])
        assert torch.equal(got[k], want), (k, got[k], want)
    assert bool(torch.isfinite(got.float()).all())
    if n > 1:
        assert bool((got[:, n // 2] == 0).all())


def test_ground_scores_rows_refuses_bad_operands(ops):
    from v3d._native import V3DError
    o = torch.randn(3, 64).half().cuda()
    with pytest.raises(V3DError):
        ops.ground_scores_rows(o, torch.randn(2, 32).half().cuda())
    with pytest.raises(V3DError):
        ops.ground_scores_rows(o, torch.randn(2, 64).bfloat16().cuda())


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("C", [256, 3584])
def test_add_rows_equals_a_loop_of_add_row(ops, C, dt):
    """x[rows[i]] += add[src[i]] in one launch = one v3d_add_row launch per row, bit for bit: unsorted rows, repeated sources, a row stride
    larger than C; every row not listed keeps its bits."""
    g = torch.Generator().manual_seed(C)
    x0 = torch.randn(40, C + 16, generator=g).to(dt).cuda()
    add = torch.randn(5, C, generator=g).to(dt).cuda()
    rows, src = [17, 3, 29, 8, 0, 39, 22], [2, 0, 2, 4, 1, 0, 2]
    got = x0.clone()
    ops.add_rows(got[:, :C], rows, src, add)
    want = x0.clone()
    for r, s in zip(rows, src):
        ops.add_row(want[:, :C], torch.tensor([r]).cuda(), add[s])
    assert torch.equal(got, want)
    rest = [r for r in range(40) if r not in rows]
    assert torch.equal(got[rest], x0[rest]) and torch.equal(got[:, C:], x0[:, C:])
    assert not torch.equal(got[rows], x0[rows])
    one = x0.clone()                                      # one source for every row: v3d_add_row itself
    ops.add_rows(one[:, :C], rows, [3] * len(rows), add)
    ref = x0.clone()
    ops.add_row(ref[:, :C], torch.tensor(rows).cuda(), add[3])
    assert torch.equal(one, ref)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_add_rows_odd_widths_and_distinct_rows(ops, dt):
    """C = 1003 on odd row strides (no 16-byte access possible: every column through the one-by-one tail) and C = 1003 on strides that are
    multiples of 8 (125 vectors + 3 tail columns): the f32 sum rounded once, as torch forms it.  A repeated destination row is refused."""
    from v3d._native import V3DError
    g = torch.Generator().manual_seed(9)
    for ld in (1005, 1008):
        x0 = torch.randn(12, ld, generator=g).to(dt).cuda()
        add = torch.randn(4, ld, generator=g).to(dt).cuda()
        got = x0.clone()
        ops.add_rows(got[:, :1003], [11, 2, 5], [1, 1, 3], add[:, :1003])
        want = x0.clone()
        for r, s in ((11, 1), (2, 1), (5, 3)):
            want[r, :1003] = (x0[r, :1003].float() + add[s, :1003].float()).to(dt)
        assert torch.equal(got, want)
    with pytest.raises(V3DError, match="distinct"):
        ops.add_rows(x0, [1, 4, 1], [0, 0, 0], add)
    with pytest.raises(V3DError):
        ops.add_rows(x0, [1, 12], [0, 0], add)


# ------------------------------------------------------------------ the tiny engine


class _Box:
    pass


def _tiny_cfg():
    from v3d.engine import EngineConfig, LlmConfig, VitConfig
    return EngineConfig(vit=VitConfig(hidden=144, inter=272, layers=2, heads=2),
                        llm=LlmConfig(hidden=256, inter=384, layers=2, heads=2, kv_heads=1, vocab=320, max_pos=1024))


def _once(fn):
    """fn, computed at its first call and answered from that result afterwards"""
    kept = []

    def call(*a, **kw):
        if not kept:
            kept.append(fn(*a, **kw))
        return kept[0]
    return call


TINY_OCFG = dict(layers=2, heads=2, kv_heads=1, rope_theta=1e6, eps=1e-6, vit_layers=2, vit_heads=2)
GROUND_LENS = (14, 9, 23, 6, 17)                            # five queries of different lengths (rows after the prefix)
GROUND_ROWS = (13, 0, 11, 3, 9)                             # the <ground> row inside each: the last row of query 0, the first of query 1


@pytest.fixture(scope="module", params=["bf16", "f16"])
def tiny(request):
    """Tiny engine with an infonce head, one scene (F = 2, 7 boxes) and the CPU oracle's scores of five grounding queries, computed once."""
    from v3d.engine import Engine, random_state_dict
    w = _Box()
    w.dt = DTYPES[request.param]
    cfg = _tiny_cfg()
    w.sd = random_state_dict(cfg, torch.float32, "cpu", seed=5, std=0.05, ground_head=True)
    w.eng = Engine(cfg, w.sd, dtype=w.dt, device="cuda", max_frames=2)
    g = torch.Generator().manual_seed(6)
    w.images = torch.randn(2, 3, 384, 384, generator=g)
    coords = (torch.rand(2, 48, 1, 48, 1, 3, generator=g) - 0.5).expand(2, 48, 8, 48, 8, 3).reshape(2, 384, 384, 3) * torch.tensor([8.0, 8.0, 3.0])
    w.coords = coords.contiguous()
    w.boxes = torch.cat([(torch.rand(7, 3, generator=g) - 0.5) * torch.tensor([6.0, 6.0, 2.0]), torch.rand(7, 3, generator=g) * 4 + 0.5], 1)
    w.prefix = torch.cat([torch.randint(0, 300, (9,), generator=g), torch.tensor([IMG])])
    w.P = 9 + 2 * 210
    w.queries = [torch.randint(0, 300, (n,), generator=g) for n in GROUND_LENS]
    # scene_ground on every query's full prompt; its question-independent stages (ViT, projector, visual tokens, patch masks: 2 s of CPU
    # time per call) see the same arguments every time and are computed once
    with pytest.MonkeyPatch.context() as mp:
        for mod, fn in ((L, "siglip_tower"), (L, "projector"), (PO, "visual_sequence"), (L, "object_patch_mask")):
            mp.setattr(mod, fn, _once(getattr(mod, fn)))
        w.want = [PO.scene_ground(w.sd, TINY_OCFG, torch.cat([w.prefix, q]), 10 + r, w.images, w.coords, w.boxes, w.dt)["scores"].float()
                  for q, r in zip(w.queries, GROUND_ROWS)]
    w.images_d, w.coords_d = w.images.cuda(), w.coords.cuda()
    yield w
    w.__dict__.clear()
    gc.collect()
    torch.cuda.empty_cache()


def test_question_embeds_with_boxes_equal_build_inputs_embeds(tiny):
    """Rows of the batch = rows [P:] of build_inputs_embeds(prefix + question, box_input, coord_token_id), bit for bit, for every question:
    two <coord> tokens in one question, none in another, a question whose box is None (its <coord> rows stay plain), different lengths;
    a pad row - question 4 ends with <coord>, so its pad rows repeat that id - never takes a PE."""
    w, eng = tiny, tiny.eng
    g = torch.Generator().manual_seed(11)
    body = lambda n: torch.randint(0, 300, (n,), generator=g)        # noqa: E731
    c = torch.tensor([COORD])
    questions = [torch.cat([body(3), c, body(4), c, body(2)]),       # two <coord> tokens
                 body(7),                                             # none
                 torch.cat([body(2), c, body(9)]),                    # box None
                 torch.cat([c, body(1)]),
                 torch.cat([body(4), c])]                             # ends with <coord>: shorter than Sq, pad rows hold id 317
    boxes = [[0.4, -1.3, 0.7], [2.0, 2.0, 0.1], None, [-3.1, 0.2, -0.9], [1.7, -2.6, 1.2]]
    feats = eng.encode_images(w.images_d)
    vox = eng.voxel_ids(w.coords_d.to(w.dt))
    want = []
    for q, b in zip(questions, boxes):
        x = eng.build_inputs_embeds(torch.cat([w.prefix, q]), feats, vox, box_input=None if b is None else torch.tensor([b]), coord_token_id=COORD)
        want.append(x[w.P:].clone())
    got = eng.question_embeds(questions, boxes, COORD).clone()
    Sq = max(len(q) for q in questions)
    assert got.shape == (5 * Sq, 256)
    plain = eng.question_embeds(questions).clone()
    for k, q in enumerate(questions):
        rows = got[k * Sq: k * Sq + len(q)]
        assert torch.equal(rows, want[k]), k
        hit = (q == COORD).cuda()
        changed = (rows != plain[k * Sq: k * Sq + len(q)]).any(1)
        assert torch.equal(changed, hit if boxes[k] is not None else torch.zeros_like(hit)), k
        assert torch.equal(got[k * Sq + len(q): (k + 1) * Sq], plain[k * Sq + len(q): (k + 1) * Sq]), "a pad row took a PE"
    assert torch.equal(got[4 * Sq + 5: 5 * Sq], eng.embed[COORD][None].expand(Sq - 5, -1))
    # the two <coord> rows of question 0 took the same PE; questions 0 and 3 different ones
    pe = lambda k, j: got[k * Sq + j].float() - plain[k * Sq + j].float()      # noqa: E731
    assert (pe(0, 3) - pe(0, 8)).abs().max() < 0.1 and (pe(0, 3) - pe(3, 0)).abs().max() > 0.5


def test_ground_group_matches_the_oracle_per_query(tiny):
    """Five queries behind one prefill with the scene's 7 proposals: each row of scores against pipeline_oracle.scene_ground on that query's
    full prompt, within the tolerance test_scene_grounding_matches_oracle states for these cosines (4e-2 bf16, 6e-3 f16); the queries in
    another order give the same rows, permuted, bit for bit."""
    w, eng = tiny, tiny.eng
    eng.use(eng.new_context())
    assert eng.prefill_scene(w.prefix, w.images_d, w.coords_d, objects=w.boxes) == w.P
    assert eng.ctx.ground_of.shape == (7, 256) and eng.ctx.ground_obj.shape == (8, 256)
    got = eng.ground_group(w.queries, list(GROUND_ROWS))
    assert got.shape == (5, 8) and got.dtype == w.dt
    worst = max((got[k].float().cpu() - w.want[k]).abs().max().item() for k in range(5))
    print(f"\n[ground_group tiny {w.dt}] max |score - oracle| over 5 queries x 8 columns: {worst:.3e} (tolerance {SCORE_TOL[w.dt]:.0e})")
    for k in range(5):
        assert (got[k].float().cpu() - w.want[k]).abs().max().item() < SCORE_TOL[w.dt], k
    perm = [3, 0, 4, 2, 1]
    again = eng.ground_group([w.queries[k] for k in perm], [GROUND_ROWS[k] for k in perm])
    assert torch.equal(again, got[perm])
    # the per-query launch of the uncached path sees the same scene: the same scores up to the f32 summation order of other GEMM tiles
    alone = eng.ground_scores(torch.cat([w.prefix, w.queries[2]]), 10 + GROUND_ROWS[2], w.images_d, w.coords_d, w.boxes)
    assert (alone.float() - got[2].float()).abs().max().item() < SCORE_TOL[w.dt]


def test_ground_group_errors(tiny):
    from v3d._native import V3DError
    w, eng = tiny, tiny.eng
    eng.use(eng.new_context())
    with pytest.raises(V3DError, match="prefill_scene"):
        eng.ground_group(w.queries, list(GROUND_ROWS))                       # nothing prefilled
    eng.prefill_scene(w.prefix, w.images_d, w.coords_d)
    assert eng.ctx.ground_of is None
    with pytest.raises(V3DError, match="objects"):
        eng.ground_group(w.queries, list(GROUND_ROWS))                       # prefilled without objects
    eng.prefill_scene(w.prefix, w.images_d, w.coords_d, objects=w.boxes)
    for rows in ([14, 0, 11, 3, 9], [13, 0, 11, 6, 9], [13, -1, 11, 3, 9], [13, 0, 11, 3]):
        with pytest.raises(V3DError, match="ground_rows"):
            eng.ground_group(w.queries, rows)                                 # outside its question (a pad row of the batch), or one short
    with pytest.raises(V3DError):
        eng.ground_group([], [])
    with pytest.raises(V3DError):
        eng.ground_group([w.queries[1]] * 33, [0] * 33)
    long = torch.randint(0, 300, (40,))
    with pytest.raises(V3DError, match="workspaces"):
        eng.ground_group([long] * 32, [0] * 32)                               # 32 x 40 rows > max_pos 1024
    assert eng.ground_group(w.queries[:1], [13]).shape == (1, 8)             # and the context still works


@pytest.mark.parametrize("kind", ["mlp", "score"])
def test_ground_group_with_the_other_heads(tiny, kind):
    """ground_head_type 'mlp' / 'score' (one-query head per row of the batch): each query's scores [7] against Engine.ground_scores on its
    full prompt - another path to the same quantity (whole-prompt tiles, one-row last layer) - within the bound
    test_ground_head_variants_golden states for these heads, 4e-2 max(1, max |score|) in bf16 (f16: 6e-3 of it)."""
    from v3d.engine import Engine
    w = tiny
    cfg = _tiny_cfg()
    cfg.ground_head_type = kind
    sd = {k: v for k, v in w.sd.items() if not k.startswith("ground_head")}
    sd.update(L.seeded_ground_head(kind, 256, 3))
    eng = Engine(cfg, sd, dtype=w.dt, device="cuda", max_frames=2)
    eng.prefill_scene(w.prefix, w.images_d, w.coords_d, objects=w.boxes)
    assert eng.ctx.ground_of.shape == (7, 256) and eng.ctx.ground_obj is None
    got = eng.ground_group(w.queries[:3], list(GROUND_ROWS[:3])).float()
    assert got.shape == (3, 7)
    eng.use(eng.new_context())
    for k in range(3):
        want = eng.ground_scores(torch.cat([w.prefix, w.queries[k]]), 10 + GROUND_ROWS[k], w.images_d, w.coords_d, w.boxes).float()
        tol = SCORE_TOL[w.dt] * max(1.0, want.abs().max().item())
        assert (got[k] - want).abs().max().item() <= tol, (k, got[k], want)


def test_prefill_without_objects_answers_as_before(tiny):
    """prefill_scene without objects keeps no object tensors and leaves the prefix K/V of the prefill with objects, bit for bit (the object
    branch runs after the decoder and writes none of its buffers); answer_group behind either gives the same tokens."""
    w, eng = tiny, tiny.eng
    steps = 4
    a = eng.use(eng.new_context())
    eng.prefill_scene(w.prefix, w.images_d, w.coords_d)
    assert a.ground_of is None and a.ground_obj is None
    plain = eng.answer_group(w.queries, max_new_tokens=steps)
    b = eng.use(eng.new_context())
    eng.prefill_scene(w.prefix, w.images_d, w.coords_d, objects=w.boxes)
    for i in range(2):
        assert torch.equal(a.kv[i][: w.P], b.kv[i][: w.P])
    with_obj = eng.answer_group(w.queries, max_new_tokens=steps)
    assert all(torch.equal(p, q) and p.shape == (steps,) for p, q in zip(plain, with_obj))


CAP_SEED = 21


def test_scan2cap_answer_group_tokens_equal_generate(tiny):
    """Six caption prompts with their own boxes behind one prefill: answer_group(box_inputs, coord_token_id) gives generate(prefix + question,
    box_input)'s tokens - except from a step at which generate()'s own top-2 margin is below 0.02 of its largest |logit|, for at
    most one question (a condition on CAP_SEED).  Swapping two questions' boxes changes their K/V rows: the boxes reach the decoder."""
    from v3d import ops
    w, eng = tiny, tiny.eng
    steps = 5
    g = torch.Generator().manual_seed(CAP_SEED)
    c = torch.tensor([COORD])
    questions = [torch.cat([torch.randint(0, 300, (a,), generator=g), c, torch.randint(0, 300, (b,), generator=g)])
                 for a, b in ((3, 9), (6, 2), (1, 14), (8, 8), (3, 6), (11, 4))]
    boxes = [[(torch.rand(1, generator=g).item() - 0.5) * s for s in (8.0, 8.0, 3.0)] for _ in questions]
    scene = eng.use(eng.new_context())
    eng.prefill_scene(w.prefix, w.images_d, w.coords_d)
    got = eng.answer_group(questions, max_new_tokens=steps, box_inputs=boxes, coord_token_id=COORD)
    st = eng._answer_state(6)
    kv = [[st.ctxs[k].kv[i][w.P: w.P + len(q)].clone() for k, q in enumerate(questions)] for i in range(2)]
    eng.use(eng.new_context())
    excused = 0
    for k, (q, b) in enumerate(zip(questions, boxes)):
        full = torch.cat([w.prefix, q])
        want = eng.generate(full, w.images_d, w.coords_d, max_new_tokens=steps, box_input=torch.tensor([b]), coord_token_id=COORD)
        for i in range(2):                                   # the question's rows (> 8 in a batch of 6 x 16: the MFMA tiles on both sides)
            assert torch.equal(kv[i][k], eng.ctx.kv[i][w.P: w.P + len(q)]), (k, i)
        if torch.equal(want, got[k]):
            continue
        first = next(s for s in range(steps) if int(want[s]) != int(got[k][s]))
        # generate()'s launches again, keeping the logits of step `first`
        x = eng.build_inputs_embeds(full, eng.encode_images(w.images_d), eng.voxel_ids(w.coords_d.to(w.dt)), box_input=torch.tensor([b]),
                                    coord_token_id=COORD)
        S = x.shape[0]
        logits = eng.llm_forward(x, 0, last_rows=[S - 1])
        for s in range(first):
            xe = ops.embed_gather(eng.embed, want[s: s + 1].cuda(), out=eng.l_x[S + s: S + s + 1])
            logits = eng.decode_forward(xe, S + s)
        top2 = torch.topk(logits.float(), 2).values
        margin = ((top2[0] - top2[1]) / logits.float().abs().max()).item()
        print(f"\n[scan2cap tiny {w.dt}] question {k} differs from step {first}: generate()'s margin there {margin:.3e}")
        assert margin < 0.02, (k, first, want.tolist(), got[k].tolist(), margin)
        excused += 1
    assert excused <= 1
    eng.use(scene)
    swapped = [boxes[1], boxes[0]] + boxes[2:]
    eng.answer_group(questions, max_new_tokens=1, box_inputs=swapped, coord_token_id=COORD)
    differs = [any(not torch.equal(kv[i][k], st.ctxs[k].kv[i][w.P: w.P + len(q)]) for i in range(2)) for k, q in enumerate(questions)]
    assert differs[0] and differs[1] and not any(differs[2:]), differs


# ------------------------------------------------------------------ 7B widths against f64

OCFG = dict(layers=2, heads=28, kv_heads=4, rope_theta=1e6, eps=1e-6)
VOCAB = 1024
WIDE_LENS = (50, 41, 9, 64, 33, 17, 58, 26)                 # 8 queries; the batch is 8 x 64 rows
WIDE_ROWS = (49, 0, 4, 30, 32, 10, 57, 13)
WIDE_SEED = 0


@pytest.fixture(scope="module")
def wide_weights():
    from v3d.engine import EngineConfig, LlmConfig, VitConfig, random_state_dict
    cfg = EngineConfig(vit=VitConfig(layers=1), llm=LlmConfig(layers=2, vocab=VOCAB, max_pos=2048))
    assert (cfg.llm.hidden, cfg.llm.heads, cfg.llm.kv_heads, cfg.llm.inter) == (3584, 28, 4, 18944)
    return cfg, ac.scale_qk(random_state_dict(cfg, torch.float32, "cpu", seed=41, std=0.02, ground_head=True), 2)


def _head64(x, w, pfx):
    """nn.Sequential(Linear, ReLU, LayerNorm, Linear) (llava_qwen.py:93-104) in f64"""
    h = torch.relu(x @ w[pfx + "0.weight"].T + w[pfx + "0.bias"])
    h = (h - h.mean(-1, keepdim=True)) / torch.sqrt(h.var(-1, unbiased=False, keepdim=True) + 1e-5) * w[pfx + "2.weight"] + w[pfx + "2.bias"]
    return h @ w[pfx + "3.weight"].T + w[pfx + "3.bias"]


def _unit64(x):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)


@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_ground_group_at_7b_widths_against_f64(wide_weights, name):
    """Engine.prefill_scene(objects) + ground_group at hidden 3584, 28 / 4 heads x 128, MLP 18944, two layers, F = 2 (P = 434), 8 queries of
    9 .. 64 rows, 9 proposals, by the rules of tests/answer_check.py.
    Reference: Reference.forward64 over the queries' embedding rows behind the f64 prefix (the engine's own inputs_embeds of the prefix as
    input, as in tests/test_gpu_answer_path_f64.py) gives the f64 residual at each <ground> row; final RMSNorm, both branches of the infonce
    head, the normalisations and the dot products are written out in f64 here, over the engine's 16-bit weights widened and the engine's
    16-bit object features (ctx.ground_of: an input of the head; the object path has its own tests).
    Noise level e_ref: the 16-bit oracle (Reference.forward16, then llm_oracle.rmsnorm + llm_oracle.infonce_scores in the engine's dtype)
    against f64 - the per-row relative L2 of the residual at the ground rows, and max |dscore|.
    The engine passes if its ground-row residuals are within FACTOR = 4 x e_ref[resid] and answer_check's caps for a final residual, its
    scores within 4 x e_ref[scores] and within the absolute 4e-2 (bf16) / 6e-3 (f16); its best column per query is the f64 arg-max unless
    the f64 top-2 gap is at most 2 e_ref[scores] - and, asserted on the reference alone before the engine's scores are read, at most 1 of
    the 8 queries has a gap that small (a condition on WIDE_SEED).  No bound comes from the engine's output.
    MEASURED on one MI355X at the committed seed (run with -s for the figures):
                  e_ref[resid]   e_ref[scores]   engine resid / e_ref   engine scores / e_ref   smallest f64 top-2 gap   near-ties
        bf16      8.6e-3         4.8e-4          1.04                   1.00                    3.0e-2                   0 of 8
        f16       1.1e-3         7.9e-5          1.01                   1.02                    3.0e-2                   0 of 8
    The engine's error is the 16-bit oracle's own; the first seed tried met the near-tie condition, none was discarded."""
    from v3d.engine import Engine
    cfg, sd = wide_weights
    dt = DTYPES[name]
    eng = Engine(cfg, sd, dtype=dt, device="cuda", max_frames=2)
    ref = ac.Reference(sd, dt, OCFG, "cuda")
    g = torch.Generator().manual_seed(4300 + WIDE_SEED)
    images = torch.randn(2, 3, 384, 384, generator=g).cuda()
    coords = ((torch.rand(2, 48, 1, 48, 1, 3, generator=g) - 0.5).expand(2, 48, 8, 48, 8, 3).reshape(2, 384, 384, 3) * torch.tensor([8.0, 8.0, 3.0])).contiguous().cuda()
    boxes = torch.cat([(torch.rand(9, 3, generator=g) - 0.5) * torch.tensor([6.0, 6.0, 2.0]), torch.rand(9, 3, generator=g) * 4 + 0.5], 1)
    prefix = torch.cat([torch.randint(0, VOCAB, (14,), generator=g), torch.tensor([IMG])])
    queries = [torch.randint(0, VOCAB, (n,), generator=g) for n in WIDE_LENS]
    G, Smax = len(queries), max(WIDE_LENS)
    x_pre = eng.build_inputs_embeds(prefix, eng.encode_images(images), eng.voxel_ids(coords.to(dt))).clone()
    P = eng.prefill_scene(prefix, images, coords, objects=boxes)
    assert P == 434 == x_pre.shape[0]
    objf = eng.ctx.ground_of
    assert objf.shape == (9, 3584) and bool(torch.isfinite(objf.float()).all())
    pre = ref.prefix(x_pre)
    # ---- both references, the engine not looked at
    ids = torch.zeros((G, Smax), dtype=torch.int64)
    for k, q in enumerate(queries):
        ids[k, : len(q)] = q
    x16 = ref.embed(ids)
    rows = torch.tensor(WIDE_ROWS, device="cuda")
    take = lambda t: t[torch.arange(G, device="cuda"), rows]          # noqa: E731
    r64 = take(ref.forward64(x16.double(), P, pre["past64"])[1])
    r16 = take(ref.forward16(x16, P, pre["past16"])[1])
    w16 = {k: v.to(dt).cuda() for k, v in sd.items() if k.startswith("ground_head")}
    w16["model.norm.weight"] = ref.w16["model.norm.weight"]
    w64 = {k: v.double() for k, v in w16.items()}
    q64 = _unit64(_head64(ac._rms64(r64, w64["model.norm.weight"], OCFG["eps"]), w64, "ground_head_query."))
    o64 = _unit64(_head64(torch.cat([objf.double(), w64["ground_head_zero_target"][None]], 0), w64, "ground_head_obj."))
    s64 = q64 @ o64.T                                                   # [G, 10]
    s16 = torch.stack([L.infonce_scores(objf, w16["ground_head_zero_target"], L.rmsnorm(r16[k][None], w16["model.norm.weight"], OCFG["eps"]), w16)
                       for k in range(G)]).double()
    e_resid = ac._row_err(r16.double(), r64).max().item()
    e_scores = (s16 - s64).abs().max().item()
    top2 = torch.topk(s64, 2, dim=-1).values
    gap = top2[:, 0] - top2[:, 1]
    near = int((gap <= 2 * e_scores).sum())
    print(f"\n[ground_group 7B widths {name}] e_ref resid {e_resid:.3e} scores {e_scores:.3e}; f64 top-2 gaps {[f'{v:.3e}' for v in gap.tolist()]}; "
          f"queries inside 2 e_ref: {near}")
    assert near <= 1, f"{near} of {G} queries have an f64 top-2 gap within 2 e_ref[scores] = {2 * e_scores:.3e}: another WIDE_SEED"
    # ---- the engine
    got = eng.ground_group(queries, list(WIDE_ROWS))
    assert got.shape == (G, 10) and bool(torch.isfinite(got.float()).all())
    resid = eng._answer_state(G).rows.x[:G].double()                   # the gathered <ground> rows of the residual stream, before the final norm
    err = ac._row_err(resid, r64)
    whole = ((resid - r64).norm() / r64.norm()).item()
    ds = (got.double() - s64).abs().max().item()
    print(f"[ground_group 7B widths {name}] engine: residual row error {err.max().item():.3e} = {err.max().item() / e_resid:.2f} x e_ref (whole {whole:.3e}); "
          f"max |dscore| {ds:.3e} = {ds / e_scores:.2f} x e_ref")
    cap_whole, cap_row = ac.caps("resid", dt)
    assert whole <= cap_whole and err.max().item() <= cap_row
    assert err.max().item() <= ac.FACTOR * e_resid
    assert ds <= ac.FACTOR * e_scores and ds <= SCORE_TOL[dt]
    best, best64 = got.float().argmax(-1), s64.argmax(-1)
    for k in range(G):
        assert int(best[k]) == int(best64[k]) or gap[k].item() <= 2 * e_scores, (k, int(best[k]), int(best64[k]), gap[k].item())
    del eng, ref
    gc.collect()
    torch.cuda.empty_cache()
