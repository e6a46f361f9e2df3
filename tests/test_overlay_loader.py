"""The overlay as a drop-in for the reference's loader path (CPU side; the GPU half is tests/test_gpu_loader.py): the overlay
package alone exports the names, registers them with the HF Auto classes and refuses unknown arguments instead of swallowing
them."""
import os
import subprocess
import sys
import textwrap

import tiny_model_fixture as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERLAY = os.path.join(ROOT, "video-3d-llm_amd")


def _run(code, pythonpath, cwd):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(pythonpath), PYTHONDONTWRITEBYTECODE="1", HF_HUB_OFFLINE="1")
    return subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, cwd=cwd, capture_output=True, text=True, timeout=600)


def test_overlay_alone_exports_registers_and_refuses_unknown_arguments(tmp_path):
    ckpt = TM.write_checkpoint(str(tmp_path / "llava_qwen_tiny"), TM.load())
    r = _run(f"""
        from llava.model import LlavaQwenForCausalLM, LlavaQwenConfig
        import llava.model as M
        assert M.__all__ == ["LlavaQwenConfig", "LlavaQwenForCausalLM"]
        from transformers import AutoConfig, AutoModelForCausalLM
        cfg = AutoConfig.from_pretrained({ckpt!r})
        assert type(cfg) is LlavaQwenConfig
        assert AutoModelForCausalLM._model_mapping[LlavaQwenConfig] is LlavaQwenForCausalLM
        for kw in (dict(trust_remote_code=True), dict(load_in_8bit=True), dict(some_new_flag=1)):
            try:
                LlavaQwenForCausalLM.from_pretrained({ckpt!r}, **kw)
            except (TypeError, NotImplementedError) as e:
                print("REFUSED", sorted(kw), type(e).__name__)
        from v3d import loader
        sd = loader.read_weights({ckpt!r})
        ec = loader.engine_config(cfg, sd)
        print("CFG", ec.vit.hidden, ec.vit.layers, ec.vit.heads, ec.vit.inter, ec.llm.hidden, ec.llm.layers, ec.llm.heads, ec.llm.kv_heads,
              ec.llm.inter, ec.llm.vocab, ec.llm.max_pos)
        print("GROUND", ec.ground_head_type, ec.object_feature_type)
        cfg.ground_head_type, cfg.object_feature_type = "score", "patch27-pe"        # the variants no shipped script selects
        ec = loader.engine_config(cfg, sd)
        print("GROUND", ec.ground_head_type, ec.object_feature_type)
        """, [OVERLAY], cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.count("REFUSED") == 3, r.stdout
    assert "CFG 144 2 2 272 256 2 2 1 384 320 2048" in r.stdout, r.stdout
    assert "GROUND infonce patch14-pe" in r.stdout and "GROUND score patch27-pe" in r.stdout, r.stdout
