"""`cfp_normal_metrics` without a GPU: the symbols, the header, the workspace query and every argument check (dummy pointers: no kernel is
launched), the Python API's own refusals, the `--normal_metrics` switch of evaluate_all.py, the numpy restatement of the definition
(`normal_metrics_ref.py`) against `pointcloud_ref.py` and against itself, and the measurement the GPU tests' tolerance rests on.

TOL_MEASURED: the worst |a32 - a64| between the float32 and the float64 restatement over the GPU tests' own inputs is 3.40e-4 degrees
(measured here on the CPU, printed by test_measured_tolerance; set by the 480 x 640 case, 1.7e-4 on the 70 x 130 batch and below 5e-5 on the
small cases).  The GPU tests allow 4 x this, 1.36e-3 degrees, against the float64 restatement."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import normal_metrics_ref as R
import pointcloud_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE = -1, -2


@pytest.fixture(scope="module")
def lib():
    from cfpnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.load()


def test_symbols_header_and_makefile(lib):
    from cfpnet_amd import hip, metrics
    for name in ("cfp_normal_metrics", "cfp_normal_metrics_ws_bytes"):
        assert hasattr(lib, name)
    text = open(os.path.join(ROOT, "include", "cfpnet_hip.h")).read()
    assert "size_t cfp_normal_metrics_ws_bytes(int B, int H, int W);" in text
    assert "int cfp_normal_metrics(const float* pred, int Hp, int Wp, const float* gt, int H, int W, int B, int interpolate, float lo" in text
    for cited in ("a = atan2f(s, c) * (float)(180 / pi)", "k = min((int)(a * 10.0f), 1799)", "median_deg = (k* + 0.5) * 0.1", "(N + 1) / 2",
                  "{mean_deg, median_deg, rmse_deg, frac_11_25, frac_22_5, frac_30, n_valid}", "`Normal` of cfp_depth_unproject",
                  "four clamped neighbours all satisfy lo < g < hi", "never accumulated with atomics", "bit-identical with and without them",
                  "a < 11.25f, a < 22.5f, a < 30.0f", "H == 1 or W == 1 gives no valid pixel"):
        assert cited in text, cited
    assert len(hip.SIGNATURES["cfp_normal_metrics"][1]) == 17 and len(hip.SIGNATURES["cfp_normal_metrics_ws_bytes"][1]) == 3
    assert hip.SIGNATURES["cfp_normal_metrics_ws_bytes"][0] is ctypes.c_size_t
    mk = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "Makefile")).read()
    assert " normal_metrics.hip " in mk and any(" normal_metrics.o " in l and l.endswith(": metrics_pred.h") for l in mk.splitlines())
    src = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "normal_metrics.hip")).read()
    assert '#include "metrics_pred.h"' in src and "met_pred(" in src and "clipf(" not in src          # the depth is included, not restated
    for line in src.splitlines():                     # atomics only on integers: no float or double atomic anywhere
        if "atomicAdd(" in line:
            assert "sCells[" in line or "cells[" in line, line
    assert metrics.NORMAL_METRIC_NAMES == R.NAMES and metrics.NORMAL_BINS == R.NB == 1800


def test_ws_bytes(lib):
    ws = lib.cfp_normal_metrics_ws_bytes
    for bad in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, -2), (70000, 8, 8), (1, 70000, 70000)):
        assert ws(*bad) == 0, bad
    sizes = [(1, 1), (7, 9), (37, 53), (240, 320), (480, 640), (1080, 1920)]
    for B in (1, 2, 3, 8):
        got = [ws(B, h, w) for h, w in sizes]
        assert all(v >= B * 1800 * 4 and v % 8 == 0 for v in got)             # a histogram per image at least
        assert all(a <= b for a, b in zip(got, got[1:])), (B, got)
        assert all(ws(B, h, w) < ws(B + 1, h, w) for h, w in sizes)
        assert got[-1] <= B * (1 << 16)                                                  # bounded: partials per workgroup, not per pixel


def test_entry_point_refuses_bad_arguments_with_a_message(lib):
    """16 = a non-null, 16-byte aligned dummy device pointer: every case fails a check before anything is dereferenced or launched."""
    from cfpnet_amd import hip
    P, BIG = 16, 1 << 40

    def call(pred=P, hp=8, wp=8, gt=P, h=8, w=8, b=1, interp=0, lo=1e-3, hi=10.0, k=P, ws=P, nbytes=BIG, out=P, hist=0, amap=0):
        rc = lib.cfp_normal_metrics(pred, hp, wp, gt, h, w, b, interp, lo, hi, k, ws, nbytes, out, hist, amap, 0)
        return rc, hip.last_error()

    for name in ("pred", "gt", "k", "out", "ws"):
        rc, msg = call(**{name: 0})
        assert rc == EINVAL and "cfp_normal_metrics: null pointer" in msg, (name, rc, msg)
    for kw in (dict(b=0), dict(h=0), dict(w=-1), dict(hp=0), dict(wp=-3)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "non-positive" in msg, (kw, rc, msg)
    for kw in (dict(h=70000, w=70000, interp=1), dict(hp=70000, wp=70000, interp=1), dict(b=70000)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "too large" in msg, (kw, rc, msg)
    for kw in (dict(hp=4, wp=4), dict(hp=8, wp=4), dict(h=16, w=16)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "sizes differ" in msg, (kw, rc, msg)
    for lo, hi in ((2.0, 1.0), (1.0, 1.0), (float("nan"), 1.0), (0.0, float("nan"))):
        rc, msg = call(lo=lo, hi=hi)
        assert rc == EINVAL and "empty depth range" in msg, (lo, hi, rc, msg)
    rc, msg = call(nbytes=lib.cfp_normal_metrics_ws_bytes(1, 8, 8) - 1)
    assert rc == EINVAL and "workspace too small" in msg
    rc, msg = call(h=480, w=640, hp=480, wp=640, b=2, nbytes=lib.cfp_normal_metrics_ws_bytes(1, 480, 640))      # sized for another batch
    assert rc == EINVAL and "workspace too small" in msg
    rc, msg = call(ws=20)
    assert rc == EINVAL and "8-byte aligned" in msg
    with pytest.raises(RuntimeError, match="cfp_normal_metrics failed"):
        hip.call("cfp_normal_metrics", P, 4, 4, P, 8, 8, 1, 0, 1e-3, 10.0, P, P, BIG, P, 0, 0, 0)


def test_python_api_refuses_before_anything_runs():
    import torch
    from cfpnet_amd import metrics, pointcloud
    sig = inspect.signature(metrics.normal_metrics)
    assert list(sig.parameters) == ["pred", "gt", "lo", "hi", "intrinsics", "size", "hist", "angle_map"]
    assert sig.parameters["size"].default is None and sig.parameters["hist"].default is False and sig.parameters["angle_map"].default is False
    assert "pointcloud._intrinsics(" in inspect.getsource(metrics.normal_metrics) and "ZJUL5_INTRINSICS" in inspect.getsource(metrics.normal_metrics)
    host = torch.ones(1, 4, 6)
    for bad in (host, host.double(), np.ones((1, 4, 6), np.float32)):
        with pytest.raises(ValueError, match="float32 device tensor"):
            metrics.normal_metrics(bad, bad, 1e-3, 10.0)
    assert pointcloud.ZJUL5_INTRINSICS == PR.ZJUL5
    # the running average on host rows: images without a valid pixel are skipped, the histograms add up
    avg = metrics.RunningNormalAverage()
    assert avg.get_value() == {} and avg.histogram() == [0] * 1800
    nan = float("nan")
    rows = torch.tensor([[10.0, 8.0, 12.0, 0.5, 0.75, 1.0, 100.0], [nan, nan, nan, nan, nan, nan, 0.0], [20.0, 10.0, 14.0, 0.25, 0.25, 0.5, 7.0]],
                        dtype=torch.float64)
    h = torch.zeros(3, 1800, dtype=torch.int32)
    h[0, 5], h[2, 5], h[2, 1799] = 100, 3, 4
    avg.update(rows[:2], h[:2])
    avg.update(rows[2:], h[2:])
    assert avg.get_value() == {"mean_deg": 15.0, "median_deg": 9.0, "rmse_deg": 13.0, "frac_11_25": 0.375, "frac_22_5": 0.5, "frac_30": 0.75,
                               "images": 2}
    hist = avg.histogram()
    assert hist[5] == 103 and hist[1799] == 4 and sum(hist) == 107
    with pytest.raises(ValueError, match=r"\[B,7\]"):
        avg.update(torch.zeros(2, 10, dtype=torch.float64))
    only_empty = metrics.RunningNormalAverage()
    only_empty.update(rows[1:2])
    assert only_empty.get_value() == {}


def test_evaluate_all_takes_the_switch_off_argv():
    import evaluate_all
    argv = ["--synthetic", "2", "--normal_metrics", "--intrinsics", "600,601.5,320,240", "--save_dir", "out"]
    assert evaluate_all._pop(argv, "--normal_metrics", False, None) is True
    assert evaluate_all._pop(argv, "--intrinsics", None, evaluate_all._intrinsics) == (600.0, 601.5, 320.0, 240.0)
    assert argv == ["--synthetic", "2", "--save_dir", "out"]
    assert evaluate_all._pop(argv, "--normal_metrics", False, None) is False
    src = inspect.getsource(evaluate_all.main)
    assert '_pop(argv, "--normal_metrics"' in src and "normals.json" in src and 'print(f"Normals: ' in src
    assert src.index('print(f"Regions: ') < src.index('print(f"Normals: ') and src.index('print(f"Uncertainty: ') < src.index('print(f"Normals: ')
    # --intrinsics alone stays the error it was, raised before a device or a model is touched; with --normal_metrics it passes that check
    with pytest.raises(ValueError, match="need --save_points"):
        evaluate_all.main(["--synthetic", "2", "--intrinsics", "1,1,0,0"])
    with pytest.raises(ValueError, match="need --save_points"):
        evaluate_all.main(["--synthetic", "2", "--normal_metrics", "--points_stride", "4"])
    with pytest.raises(ValueError, match="--range_edges needs --region_metrics"):          # a later check: the intrinsics one let it through
        evaluate_all.main(["--synthetic", "2", "--normal_metrics", "--intrinsics", "1,1,0,0", "--range_edges", "2,4"])


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["odd_19x27_to_37x53", "same_24x40_direct", "row_1x33", "column_33x1", "full_240x320_to_480x640",
                                  "batch3_nonfinite"])
def test_float32_normals_are_pointcloud_refs_bit_for_bit(name):
    """The shared cases: the normal of the prediction inside `angle_map` is `pointcloud_ref`'s float32 normal of the same case, and the
    normal of a ground truth is the one `pointcloud_ref` forms when the map is handed to it as a prediction without interpolation."""
    c = PR.UNPROJECT_CASES[name]
    pred, K = PR.unproject_inputs(name)
    want = PR.unproject_reference(name)[1]
    for b in range(pred.shape[0]):
        gt = PR.depth(pred[b], c["H"], c["W"], c["interp"])              # any map of the right size; its own normal is checked below
        _, n_p, n_g = R.angle_map(pred[b], gt, K[b], c["interp"], np.float32)
        assert n_p.dtype == np.float32 and n_p.tobytes() == want[b].tobytes()
        assert n_g.tobytes() == PR.normals(gt, K[b]).tobytes() == want[b].tobytes()     # gt = the prediction's depth: the same five depths


def test_angle_forms():
    rng = np.random.default_rng(3)
    p = rng.normal(size=(500, 3))
    p /= np.linalg.norm(p, axis=-1, keepdims=True)
    g = rng.normal(size=(500, 3))
    g /= np.linalg.norm(g, axis=-1, keepdims=True)
    a64 = R.angle64(p, g)
    assert np.abs(a64 - np.degrees(np.arccos(np.clip((p * g).sum(-1), -1, 1)))).max() < 1e-6
    a32 = R.angle32(p.astype(np.float32), g.astype(np.float32))
    assert np.abs(a32 - a64).max() < 1e-4
    q = p.astype(np.float32)
    assert (R.angle32(q, q) == 0).all() and R.angle32(q, -q).min() > 179.9              # equal normals: exactly 0
    assert R.bins(np.array([0.0, 0.09999, 0.1, 11.25, 179.99, 180.0], np.float32)).tolist() == [0, 0, 1, 112, 1799, 1799]
    h = np.zeros(1800, np.int64)
    assert np.isnan(R.median_from_hist(h))
    h[0] = 5
    assert R.median_from_hist(h) == 0.05
    h[7] = 5
    assert R.median_from_hist(h) == 0.05                                                # rank (10 + 1) / 2 = 5 is still in bin 0
    h[7] = 6
    assert R.median_from_hist(h) == 0.75
    out, hist, counts = R.reduce_map(np.array([[1.0, np.nan, 12.0], [25.0, 40.0, np.nan]], np.float32))
    assert out[6] == 4 and out[0] == 19.5 and counts == [1, 2, 3] and out[3:6].tolist() == [0.25, 0.5, 0.75] and hist.sum() == 4
    assert out[1] == (120 + 0.5) * 0.1 and out[2] == np.sqrt((1 + 144 + 625 + 1600) / 4)
    out, hist, counts = R.reduce_map(np.full((2, 2), np.nan, np.float32))
    assert out[6] == 0 and np.isnan(out[:6]).all() and hist.sum() == 0


@pytest.mark.parametrize("name", list(R.CASES))
def test_cases_cover_what_they_are_there_for(name):
    c = R.CASES[name]
    pred, gt, K = R.inputs(name)
    a64 = R.reference(name)
    valid = ~np.isnan(a64)
    print(f"{name}: valid {valid.sum((1, 2)).tolist()} of {c['H'] * c['W']}, |a32 - a64| worst {R.case_tol(name):.3e} deg")
    if min(c["H"], c["W"]) == 1:
        assert not valid.any()
        return
    assert all(0 < v.sum() <= v.size for v in valid) and (c["H"] < 64 or all(v.sum() < v.size for v in valid))
    # a pixel is valid only if the ground truth and its four clamped neighbours are in range
    with np.errstate(invalid="ignore"):
        in_range = (gt > np.float32(R.LO)) & (gt < np.float32(R.HI))
    for b in range(gt.shape[0]):
        assert not (valid[b] & ~R._neigh5(in_range[b])).any()
    assert (a64[valid] >= 0).all() and (a64[valid] <= 180).all()
    counts = [R.reduce_map(R.reference(name, np.float32)[b])[2] for b in range(gt.shape[0])]
    assert all(0 < k[0] <= k[1] <= k[2] < valid[b].sum() for b, k in enumerate(counts)), counts          # every threshold splits the pixels
    if name == "batch3_35x65_to_70x130":
        assert np.isnan(pred[2]).any() and np.isposinf(pred[2]).any() and np.isneginf(pred[2]).any()
        assert (gt == 0).any() and (gt > R.HI).sum() == 2 and c["H"] % 16 and c["W"] % 64 and c["H"] > 64 and c["W"] > 128
        assert not valid[0, 39:42, 100].any() and not valid[0, 40, 99:102].any() and valid[0, 38, 100]       # the value above hi takes its neighbours out
        in5 = R._neigh5(in_range[2])
        assert (in5 & ~valid[2]).sum() > 40                                              # the NaN patches: a zero normal of the prediction


def test_exact_cases_in_the_restatement():
    pred, gt, K = R.exact_equal_inputs()
    a = R.angle_map(pred[0], gt[0], K[0], 1, np.float32)[0]
    ok = ~np.isnan(a)
    assert ok.sum() > 1000 and (a[ok] == 0).all()
    out, hist, counts = R.reduce_map(a)
    assert out[1] == 0.05 and out[3:6].tolist() == [1.0, 1.0, 1.0] and out[0] == 0 and hist[0] == ok.sum()
    pred, gt, K = R.plane_inputs()
    for dt in (np.float32, np.float64):
        a, n_p, _ = R.angle_map(pred[0], gt[0], K[0], 0, dt)
        assert (n_p == np.array([0, 0, -1], dt)).all()                                  # fronto-parallel: exactly (0, 0, -1)
        inner = a[1:-1, 1:-1]
        worst = float(np.abs(inner.astype(np.float64) - R.PLANE_ANGLE_DEG).max())
        print(f"plane {dt.__name__}: interior angles vs {R.PLANE_ANGLE_DEG:.6f} deg, worst {worst:.3e} (bound {R.PLANE_BOUND_DEG:.3e})")
        assert not np.isnan(inner).any() and worst <= R.PLANE_BOUND_DEG
    assert abs(R.PLANE_ANGLE_DEG - np.degrees(np.arccos(np.sqrt(0.87)))) < 1e-9 and R.PLANE["K"][0] == 60.0


def test_measured_tolerance():
    """TOL_MEASURED of the module docstring.  It must stay a small angle for the GPU comparison to mean something."""
    t = R.tol_measured()
    per_case = {name: R.case_tol(name) for name in R.CASES}
    print(f"TOL_MEASURED = {t:.4e} deg; GPU tolerance 4 x = {4 * t:.4e} deg; per case {per_case}")
    assert R.TOL_MEASURED == t == max(per_case.values()) and 0.0 < 4 * t < 0.5
