"""`cfp_tof_zone_consistency` without a GPU: the symbol, the header, the shared sensor-model header, every argument check (dummy pointers: no
kernel is launched), the Python API's own refusals, `RunningZoneConsistency`, the `--zone_consistency` switch of evaluate_all.py, and the
numpy restatement of the definition (`zone_consistency_ref.py`): that its cases cover what they are there for."""
import inspect
import os

import numpy as np
import pytest

import zone_consistency_ref as R
from zone_abi_cases import EINVAL, check_shared_refusals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cfpnet_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    from cfpnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.load()


def test_symbol_header_and_makefile(lib):
    from cfpnet_amd import hip, metrics, tof
    assert hasattr(lib, "cfp_tof_zone_consistency")
    text = open(os.path.join(ROOT, "include", "cfpnet_hip.h")).read()
    assert "int cfp_tof_zone_consistency(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi," in text
    for cited in ("{mu_p, sigma_p, n_signal, n_pix, n_window, state}",
                  "{n_compared, mae_mu, rmse_mu, rel_mu, mae_sigma, frac_1bin, frac_window, n_lost, n_unmeasured, n_measured}",
                  "sy <= (float)y < ey && sx <= (float)x < ex", "bin = (int)(((d - 0.f) * (float)bins) / (max_distance - 0.f))",
                  "((double)(float)((j+1)*bin_width) + j*bin_width)/2", "(double)((float)n + 1e-9f)", "sigma = sqrt(var/nf) + 1e-9",
                  "mu_m - w <= (double)d <= mu_m + w", "lowest start winning ties", "lowest-index zone with mask != 0", "csrc/tof_cluster.h",
                  "csrc/metrics_pred.h", "no global atomics and no floating-point atomics", "identical bits", "double* zone /* [B][Z][6] */",
                  "double* summary /* [B][10] */", "float* dev_map /* [B][H][W] or NULL */"):
        assert cited in text, cited
    assert len(hip.SIGNATURES["cfp_tof_zone_consistency"][1]) == 21
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert " zone_consistency.hip " in mk
    deps = {l.split(":")[1].strip(): l.split(":")[0].split() for l in mk.splitlines()
            if l.endswith((": metrics_pred.h", ": tof_cluster.h", ": zone_core.h"))}
    assert "zone_consistency.o" in deps["metrics_pred.h"] and sorted(deps["tof_cluster.h"]) == ["tof_sim.o", "zone_consistency.o"]
    assert sorted(deps["zone_core.h"]) == ["zone_consistency.o", "zone_loss.o"]
    assert metrics.ZONE_CONSISTENCY_NAMES == R.NAMES and tof.BIN_WIDTH == R.BIN_WIDTH


def test_the_sensor_model_is_included_not_restated():
    sim = open(os.path.join(CSRC, "tof_sim.hip")).read()
    new = open(os.path.join(CSRC, "zone_consistency.hip")).read()
    head = open(os.path.join(CSRC, "tof_cluster.h")).read()
    core = open(os.path.join(CSRC, "zone_core.h")).read()      # what the metric shares with the loss; the metric reaches both headers through it
    assert '#include "tof_cluster.h"' in sim and '#include "zone_core.h"' in new and '#include "tof_cluster.h"' in core
    for src in (sim, new):
        for call in ("tof_bin(", "tof_hist_add(", "tof_cluster(", "tof_moments("):
            assert call in src, call
    for src in (sim, new, core):
        for restated in ("1e-9f", "atomicMax(", "__ffsll(", "max_d - 0.f", "sqrt(var"):        # each lives in the header alone
            assert restated not in src and restated in head, restated
    assert '#include "metrics_pred.h"' in core and "met_pred(" in new and "met_pred(" in core and "zc_span(" in core
    assert "clipf(" not in new and "clipf(" not in core                                                # the depth is included, not restated
    adds = [l for l in new.splitlines() + core.splitlines() + head.splitlines() if "atomicAdd(" in l]
    assert len(adds) == 2
    for line in adds:                                     # integer LDS counters only: no global and no floating-point atomic
        assert "&sWindow" in line or "&cnt[" in line, line
    assert "__shared__ int sWindow;" in new and "__shared__ int cnt[kTofMaxBins];" in new and "atomicAdd(" not in sim


def test_entry_point_refuses_bad_arguments_with_a_message(lib):
    """16 = a non-null dummy device pointer: every case fails a check before anything is dereferenced or launched."""
    from cfpnet_amd import hip
    P = 16

    def call(pred=P, hp=8, wp=8, h=8, w=8, b=1, interp=0, lo=1e-3, hi=10.0, rect=P, mask=P, raw=P, z=4, md=4.0, bins=100, bw=0.04, floor=20,
             zone=P, summary=P, dmap=0):
        rc = lib.cfp_tof_zone_consistency(pred, hp, wp, h, w, b, interp, lo, hi, rect, mask, raw, z, md, bins, bw, floor, zone, summary, dmap, 0)
        return rc, hip.last_error()

    for name in ("pred", "rect", "mask", "raw", "zone", "summary"):
        rc, msg = call(**{name: 0})
        assert rc == EINVAL and "cfp_tof_zone_consistency: null pointer" in msg, (name, rc, msg)
    check_shared_refusals("cfp_tof_zone_consistency", call)       # dimensions, sizes, range, bins, histogram, B * Z, and their order
    with pytest.raises(RuntimeError, match="cfp_tof_zone_consistency failed"):
        hip.call("cfp_tof_zone_consistency", P, 4, 4, 8, 8, 1, 0, 1e-3, 10.0, P, P, P, 4, 4.0, 100, 0.04, 20, P, P, 0, 0)


def test_python_api_refuses_before_anything_runs():
    import torch
    from cfpnet_amd import metrics, tof
    sig = inspect.signature(metrics.zone_consistency)
    assert list(sig.parameters) == ["pred", "raw_data", "rect_data", "mask", "lo", "hi", "size", "max_distance", "floor_count", "dev_map"]
    assert sig.parameters["size"].default is None and sig.parameters["max_distance"].default == 4.0
    assert sig.parameters["floor_count"].default == tof.AMBIENT_FLOOR == 20 and sig.parameters["dev_map"].default is False
    src = inspect.getsource(tof.zone_inputs)               # the checks and conversions the metric shares with the loss
    assert "tof.zone_inputs(" in inspect.getsource(metrics.zone_consistency) and "tof.BIN_WIDTH" in inspect.getsource(metrics.zone_consistency)
    assert "int(md / BIN_WIDTH)" in src and "raw_data.to(torch.float64)" in src
    host = torch.ones(1, 4, 6)
    for bad in (host, host.double(), np.ones((1, 4, 6), np.float32)):
        with pytest.raises(ValueError, match="float32 device tensor"):
            metrics.zone_consistency(bad, torch.zeros(1, 2, 2, dtype=torch.float64), torch.zeros(1, 2, 4), torch.zeros(1, 2, dtype=torch.bool), 1e-3, 10.0)
    # the running average on host rows: images without a compared zone are skipped, a NaN entry is left out of its column's mean
    avg = metrics.RunningZoneConsistency()
    assert avg.get_value() == {} and avg.tables() == []
    nan = float("nan")
    rows = torch.tensor([[4.0, 0.02, 0.03, 0.01, 0.004, 1.0, 0.5, 1.0, 2.0, 5.0],
                         [0.0, nan, nan, nan, nan, nan, nan, 0.0, 3.0, 0.0],
                         [2.0, 0.06, 0.05, 0.03, 0.008, 0.5, nan, 0.0, 0.0, 2.0]], dtype=torch.float64)
    tables = torch.arange(3 * 2 * 6, dtype=torch.float64).reshape(3, 2, 6)
    avg.update(rows[:2], tables[:2])
    avg.update(rows[2:], tables[2:])
    got = avg.get_value()
    assert list(got) == list(metrics.ZONE_CONSISTENCY_NAMES) + ["images"] and got["images"] == 2
    assert got["n_compared"] == 3.0 and got["mae_mu"] == 0.04 and got["frac_1bin"] == 0.75 and got["frac_window"] == 0.5 and got["n_measured"] == 3.5
    assert avg.tables() == tables.tolist()
    with pytest.raises(ValueError, match=r"\[B,10\]"):
        avg.update(torch.zeros(2, 7, dtype=torch.float64))
    only_empty = metrics.RunningZoneConsistency()
    only_empty.update(rows[1:2])
    assert only_empty.get_value() == {}


def test_evaluate_all_takes_the_switch_off_argv():
    import evaluate_all
    from cfpnet_amd import data
    argv = ["--synthetic", "2", "--zone_consistency", "--save_dir", "out"]
    assert evaluate_all._pop(argv, "--zone_consistency", False, None) is True
    assert argv == ["--synthetic", "2", "--save_dir", "out"]
    assert evaluate_all._pop(argv, "--zone_consistency", False, None) is False
    src = inspect.getsource(evaluate_all.main)
    assert '_pop(argv, "--zone_consistency"' in src and "zone_consistency.json" in src and "float(args.simu_max_distance)" in src
    order = [src.index(f'print(f"{k}: ') for k in ("Metrics", "Uncertainty", "Regions", "Normals", "ZoneConsistency")]
    assert order == sorted(order)
    assert "build.last_raw" in src and "last_raw" in inspect.getsource(data.EvalInputBuilder.__call__)
    # the re-simulation needs the distance the measurement was made with: an error before a device or a model is touched
    with pytest.raises(ValueError, match="--random_simu_max_d"):
        evaluate_all.main(["--synthetic", "2", "--zone_consistency", "--random_simu_max_d"])


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------

def test_sensor_model_by_hand():
    assert R.n_bins(4.0) == 100 and R.n_bins(40.96) == 1024
    d = np.array([0.0, 0.039, 0.04, 1.0, 3.9999, 4.0, 4.0001, -0.0, -1e-6, np.nan, np.inf], np.float32)
    assert R.bins_of(d, 4.0, 100).tolist() == [0, 0, 1, 25, 99, 99, -1, 0, -1, -1, -1]                # 4.0 folds into the last bin
    c = np.zeros(100, np.int64)
    c[[10, 11, 12]], c[[20, 21]], c[30] = (2, 3, 2), (3, 4), 7                                        # three runs of 7: the lowest start wins
    assert R.runs(c) == [(10, 13, 7), (20, 22, 7), (30, 31, 7)]
    mu, sigma, n = R.moments(c)
    centre = lambda j: (float(np.float32((j + 1) * 0.04)) + j * 0.04) / 2
    assert n == 7 and abs(mu - (2 * centre(10) + 3 * centre(11) + 2 * centre(12)) / 7) < 1e-9 and abs(sigma - np.sqrt(4 * 0.04 ** 2 / 7)) < 1e-7
    assert R.moments(np.zeros(100, np.int64)) == (0.0, 1e-9, 0)                                       # no return: mu = 0, sigma = 1e-9
    v = np.array([0.01] * 50 + [1.0] * 5 + [1.05] * 3 + [2.0] * 2, np.float32)
    assert R.floor_counts(v, 4.0, 100, 2).nonzero()[0].tolist() == [25, 26] and R.floor_counts(v, 4.0, 100, 2)[[25, 26]].tolist() == [3, 1]
    assert R.members((1.5, -3.0, 3.0, 2.5), 5, 6).nonzero()[0].tolist() == [2, 2, 2] and R.members((np.nan, 0, 5, 6), 5, 6).sum() == 0
    assert R.members((2.0, 1.0, 2.0, 4.0), 5, 6).sum() == 0 and R.members((-np.inf, -np.inf, np.inf, np.inf), 5, 6).all()
    zone = np.array([[1.0, 0.1, 9, 10, 5, 0], [0, 1e-9, 0, 4, 1, 1], [2.0, 0.1, 5, 8, 0, 2], [0, 1e-9, 0, 0, 0, 3], [2.1, 0.3, 5, 6, 6, 0]])
    raw = np.array([[1.1, 0.2], [3.0, 0.1], [0, 0], [0, 0], [2.0, 0.1]])
    s = R.summarize(zone, raw)
    assert s[[0, 7, 8, 9]].tolist() == [2, 1, 1, 3] and abs(s[1] - 0.1) < 1e-12 and abs(s[2] - 0.1) < 1e-12 and s[5] == 0.0 and s[6] == 12 / 20
    assert abs(s[3] - (0.1 / 1.1 + 0.1 / 2.0) / 2) < 1e-12 and abs(s[4] - 0.15) < 1e-12
    empty = R.summarize(zone[2:4], raw[2:4])
    assert np.isnan(empty[1:7]).all() and empty[[0, 7, 8, 9]].tolist() == [0, 0, 1, 0]


@pytest.mark.parametrize("name", list(R.CASES))
def test_cases_cover_what_they_are_there_for(name):
    c = R.CASES[name]
    pred, rect, mask, raw = R.inputs(name)
    ref = R.reference(name)
    zone, summ, d = ref["zone"], ref["summary"], ref["depth"]
    state = zone[..., 5].astype(int)
    print(f"{name}: states {state.tolist()}, n_signal {zone[..., 2].tolist()}, n_pix {zone[..., 3].tolist()}, n_window {zone[..., 4].tolist()}")
    print(f"{name}: summary {summ.tolist()}")
    assert (state == R.COMPARED).any() and R.n_bins(c["max_d"]) == (1024 if name == "bins_1024" else 100)
    if name == "interp_19x27_to_37x53":
        assert rect.shape == (1, 7, 4) and pred.shape == (1, 19, 27) and c["interp"] == 1
        assert state[0].tolist() == [0, 0, 0, 1, 1, 3, 0]
        m = [R.members(r, 37, 53) for r in rect[0]]
        assert (m[0] & m[1]).sum() > 0 and 0 < m[2].sum() < 19 * 20 and not m[3].any() and not m[4].any() and not m[5].any()
        assert zone[0, :, 3].tolist() == [x.sum() for x in m] and any(0 < w < n for w, n in zip(zone[0, :, 4], zone[0, :, 3]))
        assert (rect[0, 0] != np.round(rect[0, 0])).all()
    elif name == "big_zone":
        assert zone[0, 0, 3] == 50 * 47 > 2048 and (50 * 47) % 2048 and zone[0, 1, 3] == 15 and c["floor"] == 0
        r = R.runs(R.zone_counts(name, 0, 1))
        assert r == [(30, 31, 7), (40, 41, 7)]                                                        # a tie: the lowest start survives
        assert zone[0, 1, 2] == 7 and abs(zone[0, 1, 0] - 1.22) < 0.02
        assert 0 < zone[0, 0, 4] < zone[0, 0, 3]
    elif name == "bins_1024":
        b = R.bins_of(d[0], c["max_d"], 1024)
        assert b.max() >= 1000 and (b == -1).sum() == 6 and zone[0, 1, 0] > 30 and (zone[0, :, 2] > 0).all()
    elif name == "hi_equals_max_d":
        assert c["hi"] == c["max_d"] and (pred > 4.0).sum() > 50 and (d == np.float32(4.0)).sum() == (pred >= 4.0).sum()
        assert R.zone_counts(name, 0, 1)[99] > 20                                                     # clipped onto max_distance: the last bin
    elif name == "batch3_nonfinite":
        assert np.isnan(pred).any() and np.isposinf(pred).any() and np.isneginf(pred).any()
        assert not (rect[0] == rect[1]).all() and not (mask[0] == mask[2]).all()
        assert state[0].tolist().count(R.UNMEASURED) == 1 and (state[0] == R.COMPARED).sum() == 3
        assert not mask[1].any() and summ[1, 9] == 0 and summ[1, 0] == 0 and np.isnan(summ[1, 1:7]).all() and R.NEITHER in state[1]
        assert state[2, :2].tolist() == [R.LOST, R.LOST] and summ[2, 7] == 2 and summ[2, 0] == 0 and summ[2, 6] == 0.0
        assert {R.COMPARED, R.LOST, R.UNMEASURED, R.NEITHER} <= set(state.ravel().tolist())           # the four states
    elif name == "flat":
        centre = (float(np.float32(51 * 0.04)) + 50 * 0.04) / 2
        assert zone[0, 0].tolist()[1:] == [1e-9, 4096 - 2, 4096, 4096, 0] and abs(zone[0, 0, 0] - centre * 4094 / float(np.float32(4094) + np.float32(1e-9))) < 1e-15
    # the map: NaN exactly outside the measured zones
    inside = np.zeros(d.shape, bool)
    for b in range(len(d)):
        for z in range(rect.shape[1]):
            if mask[b, z]:
                inside[b] |= R.members(rect[b, z], c["H"], c["W"])
    assert np.array_equal(~np.isnan(ref["map"]) | np.isnan(d), inside | np.isnan(d))


def test_round_trip_inputs():
    g = R.round_trip_depth()
    rt = R.ROUND_TRIP
    assert g.shape == (2, 96, 128) and (g == 0).any() and np.isnan(g).any() and (g > rt["max_d"]).any()
    assert rt["sy0"] == (96 - 72) // 2 and rt["sx0"] == (128 - 72) // 2
