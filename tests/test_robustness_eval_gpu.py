"""`evaluate_all.py --robust_drop / --robust_sigma`: the robustness table through the command line, and the `degrade=` argument of
`EvalInputBuilder` it is built on."""
import ast
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import tof_degrade_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BASE = ["@configs/cfpnet_combine1.txt", "--selected_epoch", "best"]


def _cli(argv):
    import evaluate_all
    out, err = io.StringIO(), io.StringIO()
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
            evaluate_all.main(list(argv))
    finally:
        os.chdir(cwd)
    return out.getvalue().splitlines()


def test_cli_robustness_table(tmp_path):
    import evaluate_all
    from cfpnet_amd import config, data, metrics
    argv = BASE + ["--synthetic", "8", "--batch", "4", "--robust_drop", "0,0.5", "--robust_sigma", "0,0.05", "--save_dir", str(tmp_path)]
    lines = _cli(argv)
    assert len(lines) == 3 and lines[0].startswith("Metrics: ") and lines[2].startswith("Robustness: ")
    plain = ast.literal_eval(lines[0][len("Metrics: "):])
    table = json.loads(lines[2][len("Robustness: "):])
    print("Metrics:", plain)
    print("Robustness:", table)
    assert list(table) == ["drop", "sigma"] and list(table["drop"]) == ["0", "0.5"] and list(table["sigma"]) == ["0", "0.05"]
    assert list(plain) == list(metrics.KEYS)
    assert table["drop"]["0"] == plain and table["sigma"]["0"] == plain               # nothing asked: the `Metrics:` line exactly
    assert table["drop"]["0.5"] != plain and table["sigma"]["0.05"] != plain
    js = json.load(open(tmp_path / "robustness.json"))
    assert js["seed"] == evaluate_all.ROBUST_SEED and js["images"] == 8 and js["metrics"] == list(metrics.KEYS)
    assert js["counts"] == ["valid", "dropped", "noised"]
    for kind in ("drop", "sigma"):
        assert list(js[kind]) == list(table[kind])
        for v in table[kind]:
            assert js[kind][v]["metrics"] == table[kind][v]
    # the counts against the mirror, on the masks the simulation gives for these images
    build = data.EvalInputBuilder(config.parse_args(["@" + os.path.join(ROOT, "configs", "cfpnet_combine1.txt"), "--selected_epoch", "best"]), DEV)
    key = R.seed_key(evaluate_all.ROBUST_SEED)
    valid, dropped = [], []
    for step, (img, dep, _) in enumerate(data.batches(data.SyntheticEvalSamples(8, 480, 640), 4)):
        inp, _ = build(img, dep)
        for b, m in enumerate(inp["additional"]["mask"].cpu().numpy()):
            valid.append(int(m.sum()))
            dropped.append(len(set(R.dropped_zones(m, 0.5, key, step, b))))
    assert len(valid) == 8 and min(valid) > 2
    assert js["drop"]["0.5"]["counts"] == [np.mean(valid), np.mean(dropped), 0.0]
    assert js["drop"]["0"]["counts"] == [np.mean(valid), 0.0, 0.0]
    assert js["sigma"]["0.05"]["counts"] == [np.mean(valid), 0.0, np.mean(valid)]     # prob 1: every valid zone is noised
    assert js["sigma"]["0"]["counts"] == [np.mean(valid), 0.0, np.mean(valid)]
    # a second run prints the same
    assert _cli(argv) == lines


def test_builder_degrades_what_the_model_sees_and_keeps_the_measurement():
    import copy
    from cfpnet_amd import config, data
    img, dep, _ = next(data.batches(data.SyntheticEvalSamples(2, 480, 640), 2))
    for zt in ("8x8", "4x4"):
        a = copy.copy(config.defaults())
        a.zone_type = zt
        build = data.EvalInputBuilder(a, DEV)
        plain, _ = build(img, dep)
        raw = build.last_raw.clone()
        assert build.last_counts is None
        same, _ = build(img, dep, degrade={})
        for k in ("hist_data", "rect_data", "mask"):
            assert torch.equal(same["additional"][k], plain["additional"][k]), (zt, k)
        deg, _ = build(img, dep, degrade=dict(drop=0.5, sigma=0.05, prob=1.0, seed=7, step=1))
        assert torch.equal(build.last_raw, raw)                                   # `--zone_consistency` still sees the scene's measurement
        add, m0 = deg["additional"], plain["additional"]["mask"]
        w0 = build.sim.w0.cpu().numpy()
        ref = R.degrade(raw.cpu().numpy(), m0.cpu().numpy(), 0.5, (1.0, 0.0, 0.05), 7, 1, w0)
        assert np.array_equal(add["mask"].cpu().numpy(), ref["mask"]) and np.array_equal(build.last_counts.cpu().numpy(), ref["counts"])
        assert torch.equal(add["rect_data"], plain["additional"]["rect_data"]) and add["patch_info"] is plain["additional"]["patch_info"]
        assert not add["hist_data"][~add["mask"]].any() and not torch.equal(add["hist_data"], plain["additional"]["hist_data"])
        ulp = np.spacing(np.abs(ref["pts"]).astype(np.float32))
        assert (np.abs(add["hist_data"].cpu().numpy().astype(np.float64) - ref["pts"]) <= ulp).all()
    with pytest.raises(ValueError, match="unknown keys"):
        build(img, dep, degrade=dict(dropout=0.5))
