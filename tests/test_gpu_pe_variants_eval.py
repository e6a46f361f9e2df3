"""The ScanQA eval runner on a checkpoint whose config names another position encoding (`sample9-discrete-sin3d`): the dataset and the
checks of tests/test_gpu_eval_harness.py, one question at a time and with scene reuse.  The weights were not trained with that type; what is
checked is that the runner loads the type and that its answers are the engine's own under it."""
import json
import os

import pytest

import tiny_model_fixture as TM
from test_gpu_eval_harness import _dataset

pytestmark = pytest.mark.gpu


def test_eval_runner_takes_the_type_from_the_checkpoint(tmp_path):
    from v3d import eval_scanqa as E
    root = str(tmp_path)
    qs = _dataset(root)
    ckpt = TM.write_checkpoint(os.path.join(root, "llava_qwen_tiny"), TM.load())
    with open(os.path.join(ckpt, "config.json")) as f:
        cfg = json.load(f)
    cfg["world_position_embedding_type"] = "sample9-discrete-sin3d"
    with open(os.path.join(ckpt, "config.json"), "w") as f:
        json.dump(cfg, f)
    argv = ["--model-path", ckpt, "--video-folder", root, "--embodiedscan-folder", os.path.join(root, "embodiedscan"),
            "--metadata-folder", os.path.join(root, "metadata"), "--question-file", os.path.join(root, "questions.json"),
            "--max_frame_num", "4", "--max-new-tokens", "5"]
    assert E.main(argv + ["--answer-file", os.path.join(root, "out", "plain.jsonl"), "--no-pipeline"]) == 0
    assert E.main(argv + ["--answer-file", os.path.join(root, "out", "reuse.jsonl"), "--reuse-scenes", "--no-pipeline"]) == 0
    plain = [json.loads(l) for l in open(os.path.join(root, "out", "plain.jsonl"))]
    reuse = [json.loads(l) for l in open(os.path.join(root, "out", "reuse.jsonl"))]
    assert [r["sample_id"] for r in plain] == [r["sample_id"] for r in reuse] == [q["id"] for q in qs]
    tokenizer, model, image_processor, name = E.load_model(ckpt)
    cfg = model.engine.cfg
    assert (cfg.aggregation, cfg.n_points, cfg.discrete) == ("sample9", 9, True) and model.engine.pe_table.n_points == 9
    from llava.video_utils import VideoProcessor
    vp = VideoProcessor(video_folder=root, annotation_dir=os.path.join(root, "embodiedscan"), metadata_dir=os.path.join(root, "metadata"))
    for q, r in zip(qs, plain):
        ids = E.build_prompt_ids(q, tokenizer)
        images, vd = E._video_inputs(vp, image_processor, q["video"], model, 4)
        toks = model.engine.generate(ids[0], images[0], vd["world_coords"][0], max_new_tokens=5, eos_token_id=model._eos())
        assert E.clean_answer(tokenizer.batch_decode(toks.view(1, -1), skip_special_tokens=True)[0]) == r["pred_response"]
    # the reuse path gives the same answers unless a near-tie flips a token (tests/test_gpu_eval_harness.py:93-94)
    same = sum(a["pred_response"] == b["pred_response"] for a, b in zip(plain, reuse))
    assert same >= len(qs) - 2, (plain, reuse)
