"""`cfp_tof_zone_consistency` on the GPU: the round trip of a ground-truth map through `cfp_tof_hist_sim` (bit exact), the numpy restatement
of the definition (`zone_consistency_ref.py`, itself checked in test_zone_consistency_abi.py), determinism, the Python API and the
`--zone_consistency` switch.

Tolerances, none of them measured on the kernel:
  integers     n_signal, n_pix, n_window and state: equal.
  mu_p, sigma_p  within 1e-12 relative of the restatement: both sum float64 over the same bins in the same order; this allows for `sqrt`.
  summary      recomputed in numpy from the kernel's own zone table: the integers equal, the float64 sums within 1e-12 relative.
  dev_map      NaN at exactly the restatement's pixels, bit-equal elsewhere: one float32 subtraction of values that are bit-equal."""
import ast
import contextlib
import functools
import io
import json
import os

import numpy as np
import pytest
import torch

import zone_consistency_ref as R

pytestmark = pytest.mark.gpu

from cfpnet_amd import hip, metrics, tof  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
INT_COLS, SUM_INT = (2, 3, 4, 5), (0, 7, 8, 9)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)        # a copy: the shared inputs are read-only arrays


def zc_abi(pred, rect, mask, raw, H, W, interp, lo, hi, max_d, floor, dmap=True, bins=None):
    """The C entry point itself, every output pre-filled with a sentinel and with sentinel guard elements behind it -> numpy dict."""
    p, r, m, w = dev(pred), dev(rect), dev(mask), dev(raw)
    B, h, wd = pred.shape
    Z = rect.shape[1]
    zone = torch.full((B * Z * 6 + 8,), -77.0, dtype=torch.float64, device=DEV)
    summ = torch.full((B * 10 + 8,), -66.0, dtype=torch.float64, device=DEV)
    dm = torch.full((B * H * W + GUARD,), -55.0, dtype=torch.float32, device=DEV) if dmap else None
    hip.call("cfp_tof_zone_consistency", p.data_ptr(), h, wd, H, W, B, interp, lo, hi, r.data_ptr(), m.data_ptr(), w.data_ptr(), Z, max_d,
             R.n_bins(max_d) if bins is None else bins, R.BIN_WIDTH, floor, zone.data_ptr(), summ.data_ptr(), hip.ptr(dm), hip.current_stream())
    zone, summ = zone.cpu().numpy(), summ.cpu().numpy()
    assert (zone[B * Z * 6:] == -77.0).all() and (summ[B * 10:] == -66.0).all()
    res = dict(zone=zone[:B * Z * 6].reshape(B, Z, 6), summary=summ[:B * 10].reshape(B, 10))
    assert not (res["zone"] == -77.0).any() and not (res["summary"] == -66.0).any()                   # every entry written
    if dmap:
        dm = dm.cpu().numpy()
        assert (dm[B * H * W:] == -55.0).all() and not (dm[:B * H * W] == -55.0).any()
        res["map"] = dm[:B * H * W].reshape(B, H, W)
    return res


def run_case(name, dmap=True):
    c = R.CASES[name]
    pred, rect, mask, raw = R.inputs(name)
    return zc_abi(pred, rect, mask, raw, c["H"], c["W"], c["interp"], c["lo"], c["hi"], c["max_d"], c["floor"], dmap=dmap)


@functools.lru_cache(maxsize=None)
def run(name):
    """One call per case with the map, shared by the tests; read-only."""
    return run_case(name)


# ---- 1. the round trip: a ground-truth map is perfectly consistent with its own simulation ------------------------------------------------

def test_round_trip_of_a_ground_truth_map_is_bit_exact():
    rt = R.ROUND_TRIP
    g = dev(R.round_trip_depth())
    B, H, W, zn, S = rt["B"], rt["H"], rt["W"], rt["zone_num"], rt["nsamp"]
    Z = zn * zn
    w0, w1 = torch.linspace(1, 0, steps=S).to(DEV), torch.linspace(0, 1, steps=S).to(DEV)
    fh = torch.empty(B, Z, 2, dtype=torch.float64, device=DEV)
    rect = torch.empty(B, Z, 4, dtype=torch.float32, device=DEV)
    mask = torch.empty(B, Z, dtype=torch.uint8, device=DEV)
    pts = torch.empty(B, Z, S, dtype=torch.float32, device=DEV)
    hip.call("cfp_tof_hist_sim", g.data_ptr(), H * W, B, H, W, zn, rt["zone_px"], rt["sy0"], rt["sx0"], None, 0, rt["max_d"], R.n_bins(rt["max_d"]),
             R.BIN_WIDTH, rt["floor"], w0.data_ptr(), w1.data_ptr(), S, hip.TOF_SAMPLE_UNIFORM, fh.data_ptr(), rect.data_ptr(), mask.data_ptr(),
             pts.data_ptr(), None, hip.current_stream())
    fh_n, rect_n, mask_n = fh.cpu().numpy(), rect.cpu().numpy(), mask.cpu().numpy()
    got = zc_abi(R.round_trip_depth(), rect_n, mask_n, fh_n, H, W, 0, rt["lo"], rt["hi"], rt["max_d"], rt["floor"])
    zone, summ = got["zone"], got["summary"]
    print(f"round trip: mask {mask_n.tolist()}, summary {summ.tolist()}")
    assert 0 < mask_n.sum() < mask_n.size and mask_n[0].any() and mask_n[1].any()                     # zones with and without a return
    assert zone[..., :2].tobytes() == fh_n.tobytes()                                                  # mu_p, sigma_p: bit for bit
    state = zone[..., 5]
    assert np.isin(state, (0, 3)).all() and np.array_equal(state == 0, mask_n != 0)
    assert (zone[..., 3] == rt["zone_px"] ** 2).all()
    for b in range(B):
        assert summ[b, 0] == mask_n[b].sum() == summ[b, 9] and summ[b, 7] == 0 and summ[b, 8] == 0
        assert summ[b, 1] == 0.0 and summ[b, 2] == 0.0 and summ[b, 4] == 0.0 and summ[b, 5] == 1.0 and summ[b, 3] == 0.0
    # the map is the ground truth minus the zone's own mu inside the measured zones
    want = R.dev_map(R.PR.depth(R.round_trip_depth()[0], H, W, 0, rt["lo"], rt["hi"]), rect_n[0], mask_n[0], fh_n[0])
    assert got["map"][0].tobytes() == want.tobytes()


# ---- 2. against the restatement -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.CASES))
def test_zone_table_matches_the_restatement(name):
    got, want = run(name)["zone"], R.reference(name)["zone"]
    assert got.shape == want.shape
    for k in INT_COLS:
        assert np.array_equal(got[..., k], want[..., k]), (name, k, got[..., k].tolist(), want[..., k].tolist())
    for k in (0, 1):
        rel = np.abs(got[..., k] - want[..., k]) / np.where(want[..., k] != 0, np.abs(want[..., k]), 1.0)
        print(f"{name}: column {k} worst relative difference {rel.max():.3e}")
        assert rel.max() <= 1e-12, (name, k, rel.max())
    none = want[..., 2] == 0
    assert (got[..., 0][none] == 0.0).all() and (got[..., 1][none] == 1e-9).all()                     # no return: 0 and 1e-9, as the simulation
    if name == "flat":
        assert got[0, 0, 1] == 1e-9


@pytest.mark.parametrize("name", list(R.CASES))
def test_summary_is_the_definition_applied_to_the_kernels_own_table(name):
    got = run(name)
    _, _, _, raw = R.inputs(name)
    for b in range(got["summary"].shape[0]):
        s, want = got["summary"][b], R.summarize(got["zone"][b], raw[b])
        for k in SUM_INT:
            assert s[k] == want[k], (name, b, k, s[k], want[k])
        assert np.array_equal(np.isnan(s), np.isnan(want)), (name, b, s.tolist(), want.tolist())
        ok = ~np.isnan(want)
        rel = np.abs(s[ok] - want[ok]) / np.where(want[ok] != 0, np.abs(want[ok]), 1.0)
        print(f"{name} image {b}: summary {s.tolist()}; vs numpy, relative {rel.max():.2e}")
        assert rel.max() <= 1e-12, (name, b, rel.tolist())
        assert s[5] == want[5] or np.isnan(want[5])                                                  # a ratio of two integers
    assert np.array_equal(np.isnan(got["summary"]), np.isnan(R.reference(name)["summary"]))


@pytest.mark.parametrize("name", list(R.CASES))
def test_dev_map_matches_the_restatement(name):
    got, want = run(name)["map"], R.reference(name)["map"]
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), name
    ok = ~np.isnan(want)
    assert got[ok].tobytes() == want[ok].tobytes(), name


# ---- 3. determinism and the optional output -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["interp_19x27_to_37x53", "batch3_nonfinite", "big_zone"])
def test_repeats_and_the_optional_map_do_not_change_a_bit(name):
    first = run(name)
    again = run_case(name)
    for k in ("zone", "summary", "map"):
        assert first[k].tobytes() == again[k].tobytes(), k
    part = run_case(name, dmap=False)
    assert "map" not in part and part["zone"].tobytes() == first["zone"].tobytes() and part["summary"].tobytes() == first["summary"].tobytes()


def test_many_zones_go_through_the_map_kernel_in_chunks():
    """Z = 600 > 256: the rectangles of an image pass through LDS in three chunks; the first measured zone in index order wins."""
    rng = np.random.default_rng(5)
    H, W, Z = 40, 56, 600
    pred = (1.0 + 2.0 * rng.random((1, H, W))).astype(np.float32)
    sy, sx = rng.uniform(-4, H - 2, Z), rng.uniform(-4, W - 2, Z)
    rect = np.stack([sy, sx, sy + rng.uniform(1, 7, Z), sx + rng.uniform(1, 7, Z)], -1).astype(np.float32)[None]
    mask = (rng.random((1, Z)) < 0.5).astype(np.uint8)
    mask[0, :300] = 0                                     # the first measured zone of most pixels lies in the second or third chunk
    raw = np.stack([rng.uniform(1, 3, Z), rng.uniform(0.01, 0.1, Z)], -1)[None]
    got = zc_abi(pred, rect, mask, raw, H, W, 0, 1e-3, 10.0, 4.0, 0)
    d = np.stack([R.PR.depth(pred[0], H, W, 0, 1e-3, 10.0)])
    want = R.dev_map(d[0], rect[0], mask[0], raw[0])
    assert 0 < np.isnan(want).sum() < want.size
    assert np.array_equal(np.isnan(got["map"][0]), np.isnan(want)) and got["map"][0][~np.isnan(want)].tobytes() == want[~np.isnan(want)].tobytes()
    zone = R.zone_table(d[0], rect[0], mask[0], raw[0], 4.0, 0)
    assert all(np.array_equal(got["zone"][0][:, k], zone[:, k]) for k in INT_COLS)
    s, ws = got["summary"][0], R.summarize(got["zone"][0], raw[0])
    assert all(s[k] == ws[k] for k in SUM_INT) and np.allclose(s, ws, rtol=1e-12, atol=0)


# ---- 4. the Python API ------------------------------------------------------------------------------------------------------------------------

def test_python_api():
    name = "batch3_nonfinite"
    c = R.CASES[name]
    pred, rect, mask, raw = R.inputs(name)
    want = run(name)
    P, RC, M, RW = dev(pred), dev(rect), dev(mask), dev(raw)
    kw = dict(size=(c["H"], c["W"]), max_distance=c["max_d"], floor_count=c["floor"])
    summ, zone = metrics.zone_consistency(P, RW, RC, M, c["lo"], c["hi"], **kw)
    assert summ.shape == (3, 10) and zone.shape == (3, 4, 6) and summ.dtype == zone.dtype == torch.float64 and summ.is_cuda and zone.is_cuda
    assert summ.cpu().numpy().tobytes() == want["summary"].tobytes() and zone.cpu().numpy().tobytes() == want["zone"].tobytes()
    summ2, zone2, dmap = metrics.zone_consistency(P[:, None], RW, RC, M.bool(), c["lo"], c["hi"], dev_map=True, **kw)       # size: twice the prediction by default too
    assert torch.equal(zone2, zone) and dmap.shape == (3, 32, 40) and dmap.dtype == torch.float32
    assert summ2.cpu().numpy().tobytes() == want["summary"].tobytes() and dmap.cpu().numpy().tobytes() == want["map"].tobytes()
    summ3, _ = metrics.zone_consistency(P, RW, RC, M, c["lo"], c["hi"], max_distance=c["max_d"], floor_count=c["floor"])
    assert summ3.cpu().numpy().tobytes() == want["summary"].tobytes()
    default, _ = metrics.zone_consistency(P, RW, RC, M, c["lo"], c["hi"])
    explicit, _ = metrics.zone_consistency(P, RW, RC, M, c["lo"], c["hi"], max_distance=4.0, floor_count=tof.AMBIENT_FLOOR)
    assert default.cpu().numpy().tobytes() == explicit.cpu().numpy().tobytes()
    for bad in (dict(raw_data=RW.cpu()), dict(rect_data=RC.double()), dict(mask=M.float()), dict(mask=M[:2]), dict(raw_data=RW[:, :3]),
                dict(rect_data=RC[:, :, :3]), dict(size=(0, 5)), dict(max_distance=0.0)):
        args = dict(pred=P, raw_data=RW, rect_data=RC, mask=M, lo=c["lo"], hi=c["hi"])
        args.update(bad)
        with pytest.raises(ValueError):
            metrics.zone_consistency(**args)
    with pytest.raises(ValueError, match="empty depth range"):
        metrics.zone_consistency(P, RW, RC, M, 2.0, 1.0)
    with pytest.raises(RuntimeError, match="sizes differ"):                               # the API derives interpolate; the entry point refuses before a launch
        hip.call("cfp_tof_zone_consistency", P.data_ptr(), 16, 20, 32, 40, 3, 0, 1e-3, 10.0, RC.data_ptr(), M.data_ptr(), RW.data_ptr(), 4, 4.0, 100,
                 0.04, 2, zone.data_ptr(), summ.data_ptr(), 0, hip.current_stream())


def test_eval_input_builder_keeps_the_measurement_of_the_last_batch():
    """`last_raw` is the simulation's fh gathered through the --zone_type block like the other three tensors; the returned dict is what it
    was; and the ground truth the measurement came from is consistent with it, zone for zone."""
    import copy
    from cfpnet_amd import config, data, geometry
    samples = list(data.SyntheticEvalSamples(2, 480, 640))
    img, dep, _ = next(data.batches(samples, 2))
    builds = {}
    for zt in ("8x8", "4x4"):
        a = copy.copy(config.defaults())
        a.zone_type = zt
        builds[zt] = data.EvalInputBuilder(a, DEV)
        assert builds[zt].last_raw is None
        inp, gt = builds[zt](img, dep)
        assert sorted(inp) == ["additional", "rgb"] and sorted(inp["additional"]) == ["hist_data", "mask", "patch_info", "rect_data"]
        builds[zt] = (builds[zt].last_raw, inp["additional"], gt)
    full, part = builds["8x8"][0], builds["4x4"][0]
    idx = torch.from_numpy(geometry.central_zone_block("4x4")).to(DEV)
    assert full.shape == (2, 64, 2) and full.dtype == torch.float64 and part.shape == (2, 16, 2)
    assert part.cpu().numpy().tobytes() == full[:, idx].contiguous().cpu().numpy().tobytes()
    raw, add, gt = builds["4x4"]
    summ, zone = metrics.zone_consistency(gt, raw, add["rect_data"], add["mask"], 1e-3, 10.0, size=(480, 640))
    summ, zone, mk = summ.cpu().numpy(), zone.cpu().numpy(), add["mask"].cpu().numpy()
    assert zone[..., :2].tobytes() == raw.cpu().numpy().tobytes() and np.array_equal(zone[..., 5] == 0, mk) and mk.any()
    assert (summ[:, 1] == 0).all() and (summ[:, 5] == 1).all() and (summ[:, 0] == mk.sum(1)).all()


# ---- 5. the command line ------------------------------------------------------------------------------------------------------------------

BASE = ["@configs/cfpnet_combine1.txt", "--selected_epoch", "best"]      # the model's configuration: argparse's own n_bins = 80 has no head kernel


def test_cli_zone_consistency(tmp_path):
    import evaluate_all
    out, err = io.StringIO(), io.StringIO()
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
            evaluate_all.main(BASE + ["--synthetic", "2", "--zone_consistency", "--save_dir", str(tmp_path)])
    finally:
        os.chdir(cwd)
    lines = out.getvalue().splitlines()
    assert len(lines) == 3 and lines[0].startswith("Metrics: ") and lines[2].startswith("ZoneConsistency: ")
    printed = ast.literal_eval(lines[2][len("ZoneConsistency: "):])
    print(f"cli: ZoneConsistency {printed}")
    assert list(printed) == list(metrics.ZONE_CONSISTENCY_NAMES) + ["images"] and 1 <= printed["images"] <= 2 and printed["n_compared"] > 0
    assert os.listdir(str(tmp_path)) == ["zone_consistency.json"]
    js = json.load(open(os.path.join(str(tmp_path), "zone_consistency.json")))
    assert js["metrics"] == list(metrics.ZONE_CONSISTENCY_NAMES) and js["images"] == printed["images"] and js["max_distance"] == 4.0
    zones = np.array(js["zones"])
    assert zones.shape == (2, 64, 6) and js["zone_columns"] == list(metrics.ZONE_COLUMNS)
    assert (zones[..., 3] == 56 * 56).all() and np.isin(zones[..., 5], (0, 1, 2, 3)).all()
    assert js["means"][0] == pytest.approx(np.mean([(z[:, 5] == 0).sum() for z in zones if (z[:, 5] == 0).any()]))
