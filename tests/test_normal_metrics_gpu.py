"""`cfp_normal_metrics` on the GPU against the numpy restatement of its definition (`normal_metrics_ref.py`, itself checked in
test_normal_metrics_abi.py), against the normals `cfp_depth_unproject` writes, the Python API and the `--normal_metrics` switch.

Tolerances, none of them measured on the kernel:
  angle map    NaN at exactly the reference's pixels; elsewhere within 4 x R.tol_measured() of the float64 restatement -- the worst
               |a32 - a64| between the two restatements over these very inputs, measured on the CPU (3.40e-4 degrees, so 1.36e-3 here).
  cross-check  against atan2(|cross|, dot) in float64 of the two normals cfp_depth_unproject writes: 4 x the worst error of the float32
               angle formula on the same float32 normals (R.formula_tol, measured on the CPU; ~2e-5 degrees); exactly 0 where the two
               normals are bitwise equal.
  reductions   from the kernel's own angle map in numpy: integers equal, the float64 sums within 1e-12 relative, the median equal.
  counts       against the float64 reference with nothing excluded: between the counts at threshold -+ tolerance."""
import ast
import contextlib
import functools
import io
import json
import os

import numpy as np
import pytest
import torch

import normal_metrics_ref as R
import pointcloud_ref as PR

pytestmark = pytest.mark.gpu

from cfpnet_amd import hip, metrics, pointcloud as PC  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)        # a copy: the shared inputs are read-only arrays


def nm_abi(pred, gt, K, interp, hist=True, amap=True, lo=R.LO, hi=R.HI):
    """The C entry point itself, every output with sentinel guard elements behind it and a workspace full of garbage -> numpy dict."""
    p, g, k = dev(pred), dev(gt), dev(K)
    B, h, w = pred.shape
    H, W = gt.shape[1:]
    out = torch.full((B * 7 + 8,), -77.0, dtype=torch.float64, device=DEV)
    hs = torch.full((B * R.NB + GUARD,), -7, dtype=torch.int32, device=DEV) if hist else None
    am = torch.full((B * H * W + GUARD,), -55.0, dtype=torch.float32, device=DEV) if amap else None
    nbytes = hip.load().cfp_normal_metrics_ws_bytes(B, H, W)
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.full((nbytes // 8 + 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    hip.call("cfp_normal_metrics", p.data_ptr(), h, w, g.data_ptr(), H, W, B, interp, lo, hi, k.data_ptr(), ws.data_ptr(), nbytes,
             out.data_ptr(), hip.ptr(hs), hip.ptr(am), hip.current_stream())
    out, ws = out.cpu().numpy(), ws.cpu().numpy()
    assert (out[B * 7:] == -77.0).all() and (ws[nbytes // 8:] == 0x5A5A5A5A5A5A5A5A).all()
    res = dict(out=out[:B * 7].reshape(B, 7))
    if hist:
        hs = hs.cpu().numpy()
        assert (hs[B * R.NB:] == -7).all()
        res["hist"] = hs[:B * R.NB].reshape(B, R.NB)
    if amap:
        am = am.cpu().numpy()
        assert (am[B * H * W:] == -55.0).all()
        res["map"] = am[:B * H * W].reshape(B, H, W)
    return res


@functools.lru_cache(maxsize=None)
def run(name):
    """One launch per case with both optional outputs, shared by the tests; read-only."""
    pred, gt, K = R.inputs(name)
    return nm_abi(pred, gt, K, R.CASES[name]["interp"])


# ---- 1. the angle map against the float64 restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.CASES))
def test_angle_map_matches_the_reference(name):
    c = R.CASES[name]
    got = run(name)
    want = R.reference(name)
    tol = 4 * R.tol_measured()
    R.close_map(got["map"], want, tol, name)
    n = (~np.isnan(want)).sum((1, 2))
    assert got["out"][:, 6].tolist() == n.tolist()
    if min(c["H"], c["W"]) == 1:
        assert (n == 0).all() and np.isnan(got["out"][:, :6]).all() and not got["hist"].any()            # n_valid = 0: NaN metrics
    else:
        assert (n > 0).all() and np.isfinite(got["out"]).all()


# ---- 2. the reductions, from the kernel's own map ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.CASES))
def test_reductions_are_the_definition_applied_to_the_kernels_own_map(name):
    got = run(name)
    for b in range(got["out"].shape[0]):
        out, hist, counts = R.reduce_map(got["map"][b])
        o = got["out"][b]
        assert got["hist"][b].dtype == np.int32 and np.array_equal(got["hist"][b], hist), (name, b)
        assert o[6] == out[6] == hist.sum()
        if out[6] == 0:
            assert np.isnan(o[:6]).all()
            continue
        n = int(out[6])
        assert [int(round(o[3 + i] * n)) for i in range(3)] == counts and [o[3 + i] for i in range(3)] == [k / n for k in counts], (name, b)
        assert o[1] == out[1], (name, b, o[1], out[1])                                   # the median: equal
        rel = [abs(o[i] - out[i]) / abs(out[i]) if out[i] else abs(o[i]) for i in (0, 2)]
        print(f"{name} image {b}: n = {n}, mean {o[0]:.6f} median {o[1]:.2f} rmse {o[2]:.6f} fractions {o[3:6].tolist()}; "
              f"sums vs numpy, relative {rel[0]:.2e} / {rel[1]:.2e}")
        assert max(rel) <= 1e-12, (name, b, rel)


# ---- 3. counts and median against the reference, nothing excluded -----------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if min(c["H"], c["W"]) > 1])
def test_threshold_counts_and_median_lie_in_the_references_interval(name):
    got = run(name)
    want = R.reference(name)
    tol = 4 * R.tol_measured()
    for b in range(want.shape[0]):
        n = int(got["out"][b, 6])
        for i, t in enumerate(R.THRESHOLDS):
            lo, hi = R.count_interval(want[b], t, tol)
            k = int(round(got["out"][b, 3 + i] * n))
            print(f"{name} image {b}: #(a < {t}) = {k}, the reference allows [{lo}, {hi}]")
            assert lo <= k <= hi, (name, b, t, k, lo, hi)
        lo, hi = R.median_bin_interval(want[b], tol)
        k = int(round(got["out"][b, 1] * 10.0 - 0.5))
        assert got["out"][b, 1] == (k + 0.5) * 0.1 and lo <= k <= hi, (name, b, k, lo, hi)


# ---- 4. the cross-check with cfp_depth_unproject ------------------------------------------------------------------------------------------

def _unproject_normals(depth, K, H, W, interp, lo, hi):
    d, k = dev(depth), dev(K)
    B, h, w = depth.shape
    nrm = torch.empty(B, H, W, 3, dtype=torch.float32, device=DEV)
    pts = torch.empty(B, H, W, 3, dtype=torch.float32, device=DEV)
    hip.call("cfp_depth_unproject", d.data_ptr(), h, w, H, W, B, interp, lo, hi, k.data_ptr(), pts.data_ptr(), nrm.data_ptr(), hip.current_stream())
    return nrm.cpu().numpy()


@pytest.mark.parametrize("name", R.CROSS_CHECK_CASES + ("exact_equal",))
def test_cross_check_with_the_normals_of_depth_unproject(name):
    """n_p: the normals cfp_depth_unproject writes for the prediction; n_g: for the ground truth passed as a prediction with
    interpolate = 0 and an infinite clip range (so that it is read as it is)."""
    if name == "exact_equal":
        pred, gt, K = R.exact_equal_inputs()
        interp, got = 1, nm_abi(pred, gt, K, 1)
    else:
        pred, gt, K = R.inputs(name)
        interp, got = R.CASES[name]["interp"], run(name)
    H, W = gt.shape[1:]
    n_p = _unproject_normals(pred, K, H, W, interp, R.LO, R.HI)
    n_g = _unproject_normals(gt, K, H, W, 0, float("-inf"), float("inf"))
    with np.errstate(invalid="ignore"):
        in_range = (gt > np.float32(R.LO)) & (gt < np.float32(R.HI))
    valid = np.stack([R._neigh5(m) for m in in_range]) & (n_p != 0).any(-1) & (n_g != 0).any(-1)
    a = got["map"]
    assert np.array_equal(~np.isnan(a), valid), name
    tol = 4 * max(R.formula_tol(c) for c in R.CROSS_CHECK_CASES)
    want = R.angle64(n_p[valid], n_g[valid])
    worst = float(np.abs(a[valid].astype(np.float64) - want).max())
    same = (n_p.view(np.uint32) == n_g.view(np.uint32)).all(-1) & valid
    print(f"{name}: worst |a - atan2(|n_p x n_g|, n_p . n_g)| = {worst:.3e} deg (tolerance {tol:.3e}); {int(same.sum())} of {int(valid.sum())} "
          f"valid pixels have bitwise equal normals")
    assert worst <= tol and 0 < tol < 1e-3
    assert (a[same] == 0).all()                                                          # bitwise equal normals: exactly 0
    if name == "exact_equal":
        assert same.sum() == valid.sum() > 1000


# ---- 5. the exact cases -------------------------------------------------------------------------------------------------------------------

def test_gt_equal_to_the_enlarged_prediction_gives_zero_everywhere():
    pred, gt, K = R.exact_equal_inputs()
    got = nm_abi(pred, gt, K, 1)
    a, o = got["map"][0], got["out"][0]
    ok = ~np.isnan(a)
    assert ok.sum() > 1000 and (a[ok] == 0).all()
    assert o[6] == ok.sum() and o[0] == 0 and o[1] == 0.05 and o[2] == 0 and o[3:6].tolist() == [1.0, 1.0, 1.0]
    assert got["hist"][0, 0] == ok.sum() and got["hist"][0].sum() == ok.sum()


def test_fronto_parallel_prediction_against_a_tilted_plane():
    pred, gt, K = R.plane_inputs()
    got = nm_abi(pred, gt, K, 0)
    inner = got["map"][0, 1:-1, 1:-1]
    worst = float(np.abs(inner.astype(np.float64) - R.PLANE_ANGLE_DEG).max())
    print(f"plane: interior angles vs the analytic {R.PLANE_ANGLE_DEG:.6f} deg, worst {worst:.3e} (bound {R.PLANE_BOUND_DEG:.3e})")
    assert not np.isnan(inner).any() and worst <= R.PLANE_BOUND_DEG
    assert got["out"][0, 6] == 48 * 72 and got["out"][0, 3:6].tolist() == [0.0, 1.0, 1.0]              # 11.25 < 21.13 < 22.5: the whole map, edges included


# ---- 6. invariants --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["batch3_35x65_to_70x130", "full_2x240x320_to_480x640"])
def test_repeats_and_optional_outputs_do_not_change_a_bit(name):
    pred, gt, K = R.inputs(name)
    interp = R.CASES[name]["interp"]
    first = run(name)
    again = nm_abi(pred, gt, K, interp)
    for k in ("out", "hist", "map"):
        assert first[k].tobytes() == again[k].tobytes(), k
    for hist, amap in ((False, False), (True, False), (False, True)):
        part = nm_abi(pred, gt, K, interp, hist=hist, amap=amap)
        assert part["out"].tobytes() == first["out"].tobytes(), (hist, amap)
        assert not hist or part["hist"].tobytes() == first["hist"].tobytes()
        assert not amap or part["map"].tobytes() == first["map"].tobytes()


def test_python_api():
    name = "batch3_35x65_to_70x130"
    pred, gt, K = R.inputs(name)
    want = run(name)
    P, G = dev(pred), dev(gt)
    rows = metrics.normal_metrics(P, G, R.LO, R.HI, dev(K))
    assert isinstance(rows, torch.Tensor) and rows.shape == (3, 7) and rows.dtype == torch.float64 and rows.is_cuda
    assert rows.cpu().numpy().tobytes() == want["out"].tobytes()
    rows2, hist, amap = metrics.normal_metrics(P[:, None], G[:, None], R.LO, R.HI, dev(K), size=(70, 130), hist=True, angle_map=True)
    assert hist.dtype == torch.int32 and hist.shape == (3, 1800) and amap.shape == (3, 70, 130) and amap.dtype == torch.float32
    assert torch.equal(rows2, rows) and hist.cpu().numpy().tobytes() == want["hist"].tobytes() and amap.cpu().numpy().tobytes() == want["map"].tobytes()
    rows3, amap3 = metrics.normal_metrics(P, G, R.LO, R.HI, dev(K), angle_map=True)
    assert torch.equal(rows3, rows) and torch.equal(amap3.view(torch.int32), amap.view(torch.int32))
    # host intrinsics are used for every image; the default is the ZJU-L5 sensor's
    k0 = tuple(float(v) for v in R.K_70x130[0])
    one = metrics.normal_metrics(P[:1], G[:1], R.LO, R.HI, k0)
    assert one.cpu().numpy().tobytes() == want["out"][:1].tobytes()
    assert torch.equal(metrics.normal_metrics(P, G, R.LO, R.HI), metrics.normal_metrics(P, G, R.LO, R.HI, PC.ZJUL5_INTRINSICS))
    for bad in (dict(intrinsics=(1.0, 0.0, 2.0, 3.0)), dict(intrinsics=dev(np.ones((2, 4), np.float32))), dict(size=(35, 65)), dict(size=(0, 5))):
        with pytest.raises(ValueError):
            metrics.normal_metrics(P, G, R.LO, R.HI, **bad)
    with pytest.raises(ValueError, match="empty depth range"):
        metrics.normal_metrics(P, G, 2.0, 1.0)
    with pytest.raises(ValueError, match="batch sizes differ"):
        metrics.normal_metrics(P, G[:2], R.LO, R.HI)
    with pytest.raises(ValueError, match="float32 device tensor"):
        metrics.normal_metrics(P, G.cpu(), R.LO, R.HI)
    with pytest.raises(RuntimeError, match="sizes differ"):                               # the API derives interpolate; the entry point refuses before a launch
        hip.call("cfp_normal_metrics", P.data_ptr(), 35, 65, G.data_ptr(), 70, 130, 3, 0, R.LO, R.HI, dev(K).data_ptr(), P.data_ptr(), 1 << 30,
                 rows.data_ptr(), 0, 0, hip.current_stream())


# ---- 7. the command line ------------------------------------------------------------------------------------------------------------------

BASE = ["@configs/cfpnet_combine1.txt", "--selected_epoch", "best", "--synthetic", "4", "--batch", "4"]


def _cli(argv):
    import evaluate_all
    out, err = io.StringIO(), io.StringIO()
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
            res = evaluate_all.main(list(argv))
    finally:
        os.chdir(cwd)
    return res, out.getvalue().splitlines(), err.getvalue().splitlines()


def test_cli_normal_metrics(tmp_path, monkeypatch):
    plain, lines0, err0 = _cli(BASE)
    calls = []
    real = metrics.normal_metrics

    def recording(pred, gt, lo, hi, intrinsics=None, **kw):
        calls.append((pred.clone(), gt.clone(), lo, hi, intrinsics, kw))
        return real(pred, gt, lo, hi, intrinsics, **kw)

    monkeypatch.setattr(metrics, "normal_metrics", recording)
    res, lines, err = _cli(BASE + ["--normal_metrics", "--save_dir", str(tmp_path)])
    monkeypatch.undo()
    assert res == plain and lines[:2] == lines0 and len(lines0) == 2 and len(lines) == 3          # the Metrics lines do not change
    assert [l.split(" images in ")[0] for l in err] == [l.split(" images in ")[0] for l in err0]
    assert lines[2].startswith("Normals: ")
    printed = ast.literal_eval(lines[2][len("Normals: "):])
    assert len(calls) == 1
    pred, gt, lo, hi, intr, kw = calls[0]
    assert intr is None and (lo, hi) == (1e-3, 10.0) and kw == {"hist": True} and pred.shape[0] == 4 and tuple(gt.shape[-2:]) == (480, 640)
    rows, hist = real(pred, gt, lo, hi, PC.ZJUL5_INTRINSICS, hist=True)              # called directly on what the model produced
    rows, hist = rows.cpu().numpy(), hist.cpu().numpy()
    keep = rows[:, 6] > 0
    assert keep.all()
    means = rows[keep, :6].mean(0)
    assert list(printed) == list(metrics.NORMAL_METRIC_NAMES) + ["images"] and printed["images"] == 4
    for i, k in enumerate(metrics.NORMAL_METRIC_NAMES):
        assert printed[k] == round(float(means[i]), 3) or abs(printed[k] - means[i]) <= 5.001e-4, (k, printed[k], means[i])
    assert sorted(os.listdir(str(tmp_path))) == ["normals.json"]
    js = json.load(open(os.path.join(str(tmp_path), "normals.json")))
    assert js["metrics"] == list(metrics.NORMAL_METRIC_NAMES) and js["images"] == 4 and len(js["histogram"]) == 1800
    assert js["histogram"] == hist.sum(0).tolist() and sum(js["histogram"]) == int(rows[:, 6].sum())
    assert np.allclose(js["means"], means, rtol=1e-12, atol=0)
    print(f"cli: Normals {printed}")
    # with intrinsics of its own, and after Regions: / Uncertainty: when those are present
    monkeypatch.setattr(metrics, "normal_metrics", recording)
    _, lines, _ = _cli(BASE + ["--normal_metrics", "--intrinsics", "600,600,320,240", "--region_metrics", "--unc_metrics"])
    monkeypatch.undo()
    assert calls[1][4] == (600.0, 600.0, 320.0, 240.0)
    assert [l.split(":")[0] for l in lines if not l[0].isdigit()] == ["Metrics", "Uncertainty", "Regions", "Normals"] and lines[:2] == lines0
    with pytest.raises(ValueError, match="need --save_points"):
        _cli(BASE + ["--intrinsics", "600,600,320,240"])
