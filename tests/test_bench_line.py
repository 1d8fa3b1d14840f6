"""bench.py's output contract on CPU: the one result line (short, strict JSON, the headline keys) and --dump-outputs (float32 .npy
files under the size limit, the same sample positions on every run); on the GPU: a plain run (no --full) prints the headline alone."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _strict(s):
    def bad(c):
        raise ValueError(c)
    return json.loads(s, parse_constant=bad)


def test_result_line_is_short_strict_json_with_the_headline():
    # a whole result object as the bench produced it (25.6 KB on one line: too long for a reader of the output's tail)
    full = json.load(open(os.path.join(ROOT, "profiles", "r5z_bench.json")))
    full["kernel_ms_total"] = float("nan")
    s = bench.result_line(full)
    assert "\n" not in s and len(s) < bench.RESULT_LINE_MAX
    r = _strict(s)
    for k in ("metric", "value", "unit", "per_gpu", "n_gpus", "steps", "warmup", "ms_per_step", "ms_per_step_repeats", "dtype",
              "config", "roofline", "cpu_baseline", "rel_l1", "gate_met", "f32x3", "latency", "training"):
        assert k in r, k
    assert r["ms_per_step"] == full["ms_per_step"] and r["value"] == full["value"] and r["steps"] == full["steps"]
    assert r["kernel_ms_total"] is None and r["non_finite"] == ["kernel_ms_total"]
    assert set(r["config"]["parity"]) == {"rel_l1", "gate_met"}
    assert r["config"]["compliant_default"]["dtype"] == "f32x3"
    assert r["roofline"]["kernel"] == full["roofline"]["kernel"] and "tiles" not in r["roofline"]
    assert r["dw3x3"]["f32x3"]["met"] is True and r["dw3x3"]["bf16"]["met"] is False
    assert r["training"]["config"] == {"n_gpus": 1, "global_batch": 16} and "loss_first_step" in r["training"]


def test_result_line_of_a_two_rank_job():
    # what the N > 1 driver command reads from the line (tests/test_ddp_gpu.py runs it on the GPU)
    line = {"metric": "m", "value": 100.0, "unit": "maps/s", "per_gpu": 50.0, "n_gpus": 2, "steps": 3, "warmup": 1, "ms_per_step": 480.0,
            "ranks_seen": {"world_size": 2, "backend": "gloo", "devices_visible": 1, "ranks_per_device": 2},
            "training": {"value": 20.0, "ms_per_step": 400.0, "allreduce_ms": 3.0, "overlap_frac": None, "loss_first_step": 5.9,
                         "allreduce": "flat float32 gradient", "allreduce_plan": {"payload_MB": 86.2},
                         "config": {"workload": "w", "launch": "l", "n_gpus": 2, "global_batch": 8}, "per_gpu": 10.0}}
    r = _strict(bench.result_line(line))
    assert r["ranks_seen"] == line["ranks_seen"] and "non_finite" not in r
    t = r["training"]
    assert t["config"] == {"n_gpus": 2, "global_batch": 8} and t["allreduce_ms"] == 3.0 and "overlap_frac" in t and t["loss_first_step"] == 5.9


def test_a_nan_loss_is_named_not_hidden():
    # strict JSON has no NaN: the value becomes null AND the line names it, so a diverged training step cannot pass for a number
    line = {"metric": "m", "value": 100.0, "ms_per_step": 80.0, "steps": 3,
            "training": {"value": 20.0, "ms_per_step": 400.0, "loss_first_step": float("nan"), "config": {"n_gpus": 2, "global_batch": 8}}}
    r = _strict(bench.result_line(line))
    assert r["training"]["loss_first_step"] is None and r["non_finite"] == ["training.loss_first_step"]


def test_result_line_of_the_training_step():
    line = {"metric": "training samples/sec", "value": 500.0, "unit": "samples/s", "per_gpu": 500.0, "n_gpus": 1, "steps": 6, "warmup": 2,
            "ms_per_step": 32.0, "dtype": "fp16 activations, f32 master weights", "config": {"workload": "w", "n_gpus": 1, "global_batch": 16},
            "loss_first_step": 5.9, "allreduce_plan": {"payload_MB": 86.2, "groups_in_reduction_order": [{"elements": 1}] * 200}}
    r = _strict(bench.result_line(line))
    assert r["ms_per_step"] == 32.0 and r["config"]["global_batch"] == 16 and "allreduce_plan" not in r


def test_dump_outputs_writes_float32_within_the_limit(tmp_path):
    g = torch.Generator().manual_seed(3)
    edges = torch.rand(8, 257, generator=g)
    pred = torch.rand(8, 1, 24, 32, generator=g)
    prob = torch.rand(bench.DUMP_MAX_VALUES + 12345, generator=g).to(torch.bfloat16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"bin_edges": edges, "pred": pred, "prob": prob, "none": None})
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["bin_edges.npy", "pred.npy", "prob_sample.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64e6
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype == np.float32 and np.array_equal(x, y)
    assert np.array_equal(np.load(tmp_path / "a" / "pred.npy"), pred.numpy())
    s = np.load(tmp_path / "a" / "prob_sample.npy")
    assert s.size == bench.DUMP_MAX_VALUES - edges.numel() - pred.numel()
    assert np.isin(s, prob.float().numpy()).all()


def test_small_outputs_are_written_whole(tmp_path):
    loss = torch.tensor([4.5])
    bench.dump_outputs(str(tmp_path), {"loss": loss, "lr": torch.tensor([3e-4], dtype=torch.float64)})
    assert np.load(tmp_path / "loss.npy").tolist() == [4.5]
    assert np.load(tmp_path / "lr.npy").tolist() == [3e-4]


def test_training_dump_keeps_the_scalars_whole_and_samples_the_parameters(tmp_path):
    # --train: loss, lr, beta1 and the flat float32 master parameters (21.6 M values in the real step)
    params = torch.arange(bench.DUMP_MAX_VALUES + 1000, dtype=torch.float32)
    bench.dump_outputs(str(tmp_path), {"loss": torch.tensor([4.5]), "lr": torch.tensor([3e-4], dtype=torch.float64),
                                       "beta1": torch.tensor([0.95], dtype=torch.float64), "params": params})
    assert sorted(os.listdir(tmp_path)) == ["beta1.npy", "loss.npy", "lr.npy", "params_sample.npy"]
    s = np.load(tmp_path / "params_sample.npy")
    assert s.size == bench.DUMP_MAX_VALUES - 3 and np.all(np.diff(s) >= 0)     # sorted positions: the values of arange are the positions
    assert np.load(tmp_path / "beta1.npy").tolist() == [0.95]


def test_cli_takes_steps_dump_and_detail(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", "d", "--detail", "f.json"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.dump_outputs, a.detail) == (7, 2, "d", "f.json")


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2", "--full"])
    assert bench.parse().full is True


# what only `--full` measures or checks: none of it may appear in (or cost time in) a plain run
FULL_ONLY_KEYS = ("ms_per_step_repeats", "f32x3", "f16", "f32", "cpu_baseline", "rel_l1", "gate_met", "roofline", "dw3x3", "latency",
                  "training", "kernel_ms_total")


@pytest.mark.gpu
def test_a_plain_run_prints_the_headline_alone(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` as a fresh child process: one strict-JSON line with the headline, the last timed step's
    outputs under --dump-outputs, and none of the --full objects."""
    import subprocess
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = _strict(lines[0])
    assert d["metric"].startswith("depth maps/sec @ 480x640 bf16") and d["unit"] == "maps/s" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert abs(d["value"] - 8 * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    assert d["config"]["launch"].startswith("hipGraph replay") and "non_finite" not in d
    for k in FULL_ONLY_KEYS:
        assert k not in d, k
    assert sorted(os.listdir(out)) == ["bin_edges.npy", "pred.npy", "prob_sample.npy"]
    pred = np.load(out / "pred.npy")
    assert pred.shape == (8, 1, 240, 320) and np.isfinite(pred).all()
