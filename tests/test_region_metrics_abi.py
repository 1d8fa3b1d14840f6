"""`cfp_eval_metrics_regions` without a GPU: the symbols, the enum, the workspace query and the argument checks (no kernel is launched),
the Python API's own checks, the new switches of evaluate_all.py, the numpy reference of the definition (`region_metrics_ref.py`)
against a brute-force per-pixel loop, the summation-order margin of the tolerance on the GPU tests' inputs, and the `--zone_type`
geometry against the known answers."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest

import region_metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from cfpnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.load()


def test_symbols_and_enum(lib):
    from cfpnet_amd import hip, metrics
    assert hasattr(lib, "cfp_eval_metrics_regions") and hasattr(lib, "cfp_eval_metrics_regions_ws_bytes")
    text = open(os.path.join(ROOT, "include", "cfpnet_hip.h")).read()
    assert "enum { CFP_REGION_ALL = 0, CFP_REGION_FOV_IN, CFP_REGION_FOV_OUT, CFP_REGION_ZONE_VALID, CFP_REGION_ZONE_INVALID };" in text
    assert "size_t cfp_eval_metrics_regions_ws_bytes(int B);" in text and "int cfp_eval_metrics_regions(const float* pred" in text
    assert (hip.REGION_ALL, hip.REGION_FOV_IN, hip.REGION_FOV_OUT, hip.REGION_ZONE_VALID, hip.REGION_ZONE_INVALID) == (0, 1, 2, 3, 4)
    assert metrics.REGIONS == R.REGIONS == ("all", "fov_in", "fov_out", "zone_valid", "zone_invalid")
    assert len(hip.SIGNATURES["cfp_eval_metrics_regions"][1]) == 20
    assert "region_metrics.hip" in open(os.path.join(ROOT, "cfpnet_amd", "csrc", "Makefile")).read()
    assert metrics.range_labels(()) == ("all",) and metrics.range_labels((2, 4)) == ("all", "<2", "2-4", ">=4")
    assert metrics.range_labels((0.5, 1, 2.25)) == ("all", "<0.5", "0.5-1", "1-2.25", ">=2.25")


def test_ws_bytes_monotone(lib):
    ws = lib.cfp_eval_metrics_regions_ws_bytes
    assert ws(0) == 0 and ws(-3) == 0 and ws(1) > 0 and ws(1) % 8 == 0
    for a, b in zip(range(1, 9), range(2, 10)):
        assert ws(a) < ws(b)
    assert ws(1) >= 24 * 10 * 8                      # at least one table of 24 cells x 10 doubles


def test_invalid_arguments_are_refused_with_a_message(lib):
    """16 = a non-null, 16-byte aligned dummy device pointer; `edges` is the one host pointer and is real.  Every case fails a check
    before anything on the device is dereferenced or launched."""
    from cfpnet_amd import hip
    P, BIG = 16, 1 << 40
    EINVAL, ESHAPE = -1, -2

    def farr(*v):
        return (ctypes.c_float * max(len(v), 1))(*v)

    def call(pred=P, hp=8, wp=8, gt=P, h=8, w=8, b=1, interp=0, mode=0, lo=1e-3, hi=10.0, rect=P, mask=P, z=4, edges=(2.0, 4.0), n_edges=None,
             ws=P, nbytes=BIG, out=P):
        e = None if edges is None else farr(*edges)
        n = len(edges) if n_edges is None else n_edges
        rc = lib.cfp_eval_metrics_regions(pred, hp, wp, gt, h, w, b, interp, mode, lo, hi, rect, mask, z, e, n, ws, nbytes, out, 0)
        return rc, hip.last_error()

    for name in ("pred", "gt", "rect", "mask", "ws", "out"):
        rc, msg = call(**{name: 0})
        assert rc == EINVAL and "cfp_eval_metrics_regions: null pointer" in msg, (name, rc, msg)
    rc, msg = call(edges=None, n_edges=2)
    assert rc == EINVAL and "null pointer" in msg
    for kw in (dict(b=0), dict(h=0), dict(w=-1), dict(hp=0), dict(wp=0)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "non-positive" in msg, (kw, rc, msg)
    rc, msg = call(hp=4, wp=4)
    assert rc == ESHAPE and "sizes differ" in msg
    for z in (0, -4):
        rc, msg = call(z=z)
        assert rc == ESHAPE and "Z must be positive" in msg
    for n in (-1, 8):
        rc, msg = call(edges=tuple(float(i) for i in range(1, 9)), n_edges=n)
        assert rc == EINVAL and "n_edges" in msg, (n, rc, msg)
    for edges in ((2.0, 2.0), (4.0, 2.0), (1.0, float("nan")), (1.0, float("inf")), (float("-inf"), 1.0), (1.0, 2.0, 1.5)):
        rc, msg = call(edges=edges)
        assert rc == EINVAL and "strictly increasing" in msg, (edges, rc, msg)
    for lo, hi in ((2.0, 1.0), (1.0, 1.0)):
        rc, msg = call(lo=lo, hi=hi)
        assert rc == EINVAL and "empty depth range" in msg
    rc, msg = call(mode=2)
    assert rc == EINVAL and "mode" in msg
    rc, msg = call(nbytes=lib.cfp_eval_metrics_regions_ws_bytes(1) - 1)
    assert rc == EINVAL and "workspace too small" in msg
    rc, msg = call(ws=20)
    assert rc == EINVAL and "8-byte aligned" in msg
    # the twin answers the shared cases with the same codes
    assert lib.cfp_eval_metrics(P, 4, 4, P, 8, 8, 1, 0, 0, 1e-3, 10.0, P, BIG, P, 0) == ESHAPE
    assert lib.cfp_eval_metrics(P, 8, 8, P, 8, 8, 1, 0, 0, 2.0, 1.0, P, BIG, P, 0) == EINVAL
    with pytest.raises(RuntimeError, match="cfp_eval_metrics_regions failed"):
        hip.call("cfp_eval_metrics_regions", P, 8, 8, P, 8, 8, 1, 0, 0, 1e-3, 10.0, P, P, 0, farr(), 0, P, BIG, P, 0)


def test_python_api_rejects_host_tensors_and_bad_shapes_before_anything_runs():
    import torch
    from cfpnet_amd import metrics
    sig = inspect.signature(metrics.region_metrics)
    assert list(sig.parameters) == ["pred", "gt", "lo", "hi", "rect_data", "mask", "range_edges", "mode", "out"]
    assert sig.parameters["range_edges"].default == () and sig.parameters["mode"].default == metrics.EVALUATE_ALL
    p, g, r, m = torch.ones(1, 4, 4), torch.ones(1, 4, 4), torch.zeros(1, 4, 4), torch.ones(1, 4, dtype=torch.bool)
    with pytest.raises(ValueError, match="device tensors"):
        metrics.region_metrics(p, g, 1e-3, 10.0, r, m)                      # host tensors
    with pytest.raises(ValueError):
        metrics.region_metrics(p.double(), g, 1e-3, 10.0, r, m)
    run = metrics.RunningRegionAverage((2, 4))
    assert run.get_value() == {} and run.labels == ("all", "<2", "2-4", ">=4")
    with pytest.raises(ValueError):
        run.update(torch.zeros(2, 5, 3, 10, dtype=torch.float64))           # Q = 4 expected
    # the recurrence on host rows: an image is skipped only in the segments where it has no pixel
    rows = torch.full((3, 5, 1, 10), float("nan"), dtype=torch.float64)
    rows[..., 9] = 0
    rows[0, 0, 0] = torch.tensor([1.0] * 9 + [5.0])
    rows[2, 0, 0] = torch.tensor([3.0] * 9 + [7.0])
    rows[2, 3, 0] = torch.tensor([0.5] * 9 + [2.0])
    one = metrics.RunningRegionAverage()
    one.update(rows[:2])
    one.update(rows[2:])
    val = one.get_value()
    assert val["all"]["all"] == dict(zip(metrics.KEYS, [2.0] * 9)) and val["zone_valid"]["all"]["rmse"] == 0.5 and val["fov_in"]["all"] == {}
    assert one.image_counts["all"]["all"] == 2 and one.image_counts["zone_valid"]["all"] == 1 and one.image_counts["fov_out"]["all"] == 0


def test_evaluate_all_takes_the_switches_off_argv():
    import evaluate_all
    argv = ["--synthetic", "8", "--region_metrics", "--range_edges", "2,4", "--zone_area_only", "--zone_type", "4x4"]
    assert evaluate_all._pop(argv, "--region_metrics", False, None) is True
    assert evaluate_all._pop(argv, "--range_edges", "", str) == "2,4"
    assert argv == ["--synthetic", "8", "--zone_area_only", "--zone_type", "4x4"]          # the reference's own flags stay for its parser
    assert evaluate_all._pop(argv, "--region_metrics", False, None) is False
    src = inspect.getsource(evaluate_all.main)
    assert '_pop(argv, "--region_metrics"' in src and '_pop(argv, "--range_edges"' in src
    assert "Regions: " in src and "regions.json" in src and "zone_area_only" in src and "outside_zone_area_only" in src
    from cfpnet_amd import config
    ns = config.parse_args(["--zone_area_only", "--zone_type", "4x4"])
    assert ns.zone_area_only is True and ns.outside_zone_area_only is False and ns.zone_type == "4x4"


# ---- the numpy reference against a brute-force per-pixel loop ----------------------------------------------------------------------------

def test_reference_equals_a_per_pixel_loop():
    from cfpnet_amd import synthetic
    from cfpnet_amd.geometry import centered_zone_rects
    from oracle import metrics_oracle as MO
    H, W = 20, 30
    gt, pred = synthetic.make_eval_pair(H, W, 10, 15, 21, 0.1, 0.15)
    gt = (gt * np.float32(1.0 + 0.05 * np.arange(W))).astype(np.float32)          # stretch the depth over several ranges
    rect = centered_zone_rects(H, W, 3, 6, 4)                                     # rows 5..23 (overhang), columns 10..28
    mask = np.array([1, 0, 1, 1, 1, 0, 0, 1, 1], bool)
    edges = (1.0, 1.5, 2.5)
    lo, hi = R.LO, R.HI
    for mode, proto in ((0, MO.protocol_evaluate_all), (1, MO.protocol_validate)):
        table, counts = R.reference(pred, gt, lo, hi, rect, mask, edges, mode)
        # the full-resolution prediction of the protocol, through the oracle with every pixel valid
        _, full = proto(pred.copy(), np.full((H, W), np.float32(1.0)), lo, hi)
        full = full.reshape(H, W)
        aa, bb = max(0, int(rect[0, 0])), max(0, int(rect[0, 1]))
        cc, dd = min(H, int(rect[-1, 2])), min(W, int(rect[-1, 3]))
        assert (aa, bb, cc, dd) == (5, 10, 20, 28) == R.fov_rect(rect, H, W)
        members = {}
        for y in range(H):
            for x in range(W):
                g = gt[y, x]
                if not (g > lo and g < hi):
                    continue
                fov = aa <= y < cc and bb <= x < dd
                zone = any(mask[z] and rect[z, 0] <= y < rect[z, 2] and rect[z, 1] <= x < rect[z, 3] for z in range(9))
                regions = [0, 1 if fov else 2] + ([3 if zone else 4] if fov else [])
                r = sum(1 for e in edges if g >= np.float32(e))
                for reg in regions:
                    for q in (0, 1 + r):
                        members.setdefault((reg, q), []).append((g, full[y, x]))
        assert sum(len(v) for k, v in members.items() if k[1] == 0 and k[0] in (1, 2)) == counts[0, 0]
        n_checked = 0
        for reg in range(5):
            for q in range(len(edges) + 2):
                pix = members.get((reg, q), [])
                assert len(pix) == counts[reg, q], (reg, q)
                if not pix:
                    assert np.isnan(table[reg, q]).all()
                    continue
                g, p = np.array([a for a, _ in pix], np.float32), np.array([b for _, b in pix], np.float32)
                want = MO.compute_errors(g, p)
                assert np.array_equal(table[reg, q], np.array([want[k] for k in R.KEYS])), (reg, q)
                n_checked += 1
        assert n_checked >= 15
        assert counts[1, 0] + counts[2, 0] == counts[0, 0] and counts[3, 0] + counts[4, 0] == counts[1, 0]
        assert (counts[:, 1:].sum(1) == counts[:, 0]).all()


@pytest.mark.parametrize("name", list(R.CASES))
def test_float32_oracle_stays_within_a_quarter_of_the_tolerance_of_float64_sums(name):
    """The kernel sums the oracle's float32 terms in float64; the oracle sums them in float32.  On the GPU tests' inputs the two differ
    by well under a quarter of the tolerance on every non-empty segment, so the tolerance is not consumed by the summation order."""
    gt, pred, rect, mask, edges = R.case_inputs(name)
    for mode in (0, 1):
        table, counts = R.case_reference(name, mode)
        t64, c64 = R.reference(pred, gt, R.LO, R.HI, rect, mask, edges, mode, errors=R.errors_f64)
        assert np.array_equal(counts, c64)
        ne = counts > 0
        ratio = np.abs(table[ne] - t64[ne]) / (R.RTOL * np.maximum(np.abs(t64[ne]), 1e-3))
        print(f"{name} mode {mode}: {int(ne.sum())} non-empty segments, smallest {int(counts[ne].min())} px, worst ratio {ratio.max():.3e}")
        assert ratio.max() <= 0.25


def test_case_table_covers_what_it_claims():
    gt, pred, rect, mask, edges = R.case_inputs("overhang_bottom_right")
    assert R.fov_rect(rect, 75, 101) == (21, 34, 75, 101) and rect[-1, 2] > 75 and rect[-1, 3] > 101
    gt, pred, rect, mask, edges = R.case_inputs("overhang_top_left_E7")
    assert R.fov_rect(rect, 75, 101)[:2] == (0, 0) and rect[0, 0] < 0 and rect[0, 1] < 0 and len(edges) == 7 and pred.shape == gt.shape
    counts = R.case_reference("overhang_top_left_E7", 0)[1]
    assert (counts > 0).sum() * 2 >= counts.size, counts.tolist()              # at least half of the 45 segments are non-empty
    counts = R.case_reference("full_size", 0)[1]
    assert (counts[:, 3] == 0).all() and (counts[:, :3] > 0).all()             # nothing at or beyond 4 m
    assert R.case_reference("no_edges", 0)[0].shape == (5, 1, 9)
    gt, pred, rect, mask, edges = R.batch_inputs()
    assert not mask[1].any() and not (gt[2] > 0).any() and not np.array_equal(mask[0], mask[2])


# ---- --zone_type geometry ------------------------------------------------------------------------------------------------------------

def test_central_blocks_are_the_centred_smaller_grids():
    from cfpnet_amd import geometry as G
    full = G.centered_zone_rects(480, 640, 8, 56)
    for zt, n in (("6x6", 6), ("4x4", 4), ("2x2", 2)):
        idx = G.central_zone_block(zt)
        a = (8 - n) // 2
        assert idx.tolist() == [zy * 8 + zx for zy in range(a, a + n) for zx in range(a, a + n)]
        assert np.array_equal(full[idx], G.centered_zone_rects(480, 640, n, 56))
    assert G.central_zone_block("8x8").tolist() == list(range(64))
    for bad in ("3x3", "", "8X8", "16x16"):
        with pytest.raises(ValueError):
            G.central_zone_block(bad)


def test_patch_info_of_the_2x2_block_equals_the_known_answer(golden_dir):
    from cfpnet_amd import geometry as G
    case = json.load(open(os.path.join(golden_dir, "geometry.json")))["zone_2x2"]
    rects = G.centered_zone_rects(480, 640, 8, 56)[G.central_zone_block("2x2")]
    assert np.array_equal(rects, np.array(case["rects"], np.float32))
    pi = G.patch_info_from_rect_data(rects, (480, 640))
    assert pi["zone_num"] == case["zone_num"] == 2
    for s in (4, 8, 16):
        for k in ("pad_size", "patch_size", "index_wo_pad"):
            assert pi[s][k].tolist() == case[str(s)][k], (s, k)
