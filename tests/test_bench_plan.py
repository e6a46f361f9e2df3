"""What `bench.py` measures beside its headline: nothing in a plain run; with --full, every measurement the --no-* options leave in."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

PLAIN = ["--gpus", "1", "--steps", "4", "--warmup", "1"]
EVERYTHING = {"s4096_proxy", "cached_questions", "decode_step", "eval_runner", "ground_config2", "fp8_config3", "train_config4", "cpu_baseline"}


def plan(*args, world=1):
    return bench.extra_plan(bench.parse_args([*PLAIN, *args]), world)


def test_a_plain_run_measures_only_the_headline():
    assert plan() == set()
    for opt in ("--no-extras", "--no-cpu-baseline", "--no-fp8-extra", "--no-train-extra", "--fp8"):
        assert plan(opt) == set()


def test_full_runs_every_other_measurement_and_the_no_options_trim_it():
    assert plan("--full") == EVERYTHING
    assert plan("--full", "--fp8") == EVERYTHING - {"fp8_config3"}          # the headline already is the fp8 run
    assert plan("--full", "--no-fp8-extra") == EVERYTHING - {"fp8_config3"}
    assert plan("--full", "--no-train-extra") == EVERYTHING - {"train_config4"}
    assert plan("--full", "--no-cpu-baseline") == EVERYTHING - {"cpu_baseline"}
    assert plan("--full", "--no-extras") == {"cpu_baseline"}
    assert plan("--full", "--no-extras", "--no-cpu-baseline") == set()
    assert plan("--full", "--eval-runner-only") == {"eval_runner", "cpu_baseline"}
    assert plan("--full", "--eval-runner-only", "--no-cpu-baseline") == {"eval_runner"}


def test_full_adds_nothing_with_more_than_one_rank():
    assert plan("--full", world=2) == set()


def test_eval_runner_only_needs_full(capsys):
    with pytest.raises(SystemExit) as e:
        bench.parse_args([*PLAIN, "--eval-runner-only"])
    assert e.value.code == 2 and "--full" in capsys.readouterr().err
