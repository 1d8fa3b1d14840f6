"""`cfp_depth_unproject` / `cfp_points_compact` on the GPU against the numpy restatement of their definition (`pointcloud_ref.py`, itself
checked in test_pointcloud_abi.py), the Python API around them and the `--save_points` switch of evaluate_all.py.

Tolerances, none of them measured on the kernels:
  points   the project's own bound (tests/test_metrics.py), |got - want| <= 2e-5 * max(|want|, 1e-3) per coordinate against the float32
           restatement; NaN at exactly the same places.
  normals  zero at exactly the same pixels; elsewhere within 4 x R.normal_angle_measured() of the float32 restatement -- the worst angle
           between the float32 and the float64 restatement over these very inputs, measured on the CPU (test_pointcloud_abi.py prints
           it: 2.6e-3 rad, set by the float32 source coordinates of the protocol's blend at 480 x 640); the factor covers a kernel that
           orders the terms of the cross product differently from numpy.
  compact  counts and indices exactly against the float64 reference -- the thresholds of the case table keep 1e-4 relative away from
           every reference value, asserted on the CPU -- and rows bitwise equal to the dense map gathered at those indices."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import pointcloud_ref as R

pytestmark = pytest.mark.gpu

from cfpnet_amd import hip, pointcloud as PC  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def unproject_abi(pred, K, H, W, interp, normals=True, lo=R.LO, hi=R.HI):
    """The C entry point itself (the Python API derives `interpolate` from the sizes) -> (points, normals or None) as numpy."""
    p, k = dev(pred), dev(K)
    B, h, w = pred.shape
    pts = torch.full((B, H, W, 3), -77.0, dtype=torch.float32, device=DEV)
    nrm = torch.full((B, H, W, 3), -77.0, dtype=torch.float32, device=DEV) if normals else None
    hip.call("cfp_depth_unproject", p.data_ptr(), h, w, H, W, B, interp, lo, hi, k.data_ptr(), pts.data_ptr(), hip.ptr(nrm), hip.current_stream())
    return pts.cpu().numpy(), None if nrm is None else nrm.cpu().numpy()


# ---- 1. unproject against the reference ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.UNPROJECT_CASES))
def test_unproject_matches_the_reference(name):
    c = R.UNPROJECT_CASES[name]
    pred, K = R.unproject_inputs(name)
    want_p, want_n = R.unproject_reference(name)
    tol = 4 * R.normal_angle_measured()
    got_p, got_n = unproject_abi(pred, K, c["H"], c["W"], c["interp"])
    R.close_points(got_p, want_p, name)
    R.close_normals(got_n, want_n, tol, name)
    print(f"{name}: {int((got_p != want_p).sum() - np.isnan(want_p).sum())} of {want_p.size} coordinates and "
          f"{int((got_n != want_n).sum())} normal components differ from the float32 restatement in any bit")
    only_p, none = unproject_abi(pred, K, c["H"], c["W"], c["interp"], normals=False)
    assert none is None and only_p.tobytes() == got_p.tobytes()                   # the same points with and without normals
    if min(c["H"], c["W"]) == 1:
        assert not got_n.any()                                                     # no neighbour in one direction: every normal is zero
    else:
        nz = (got_n != 0).any(-1)
        assert nz.any() and ((got_n[nz].astype(np.float64) * got_p[nz]).sum(-1) < 0).all()       # faces the camera
    if name == "batch3_nonfinite":
        assert np.isnan(got_p[2]).any() and not np.isnan(got_p[:2]).any() and ((got_n[2] == 0).all(-1)).sum() > 40
        assert not (got_n[:2] == 0).all(-1).any()
    if name == "plane_48x72":
        inner = got_n[0, 1:-1, 1:-1].reshape(-1, 3)
        worst = float(R.angle(inner, np.broadcast_to(np.array(R.PLANE_N), inner.shape)).max())
        bound = R.PLANE_ANGLE_BOUND + 4 * R.case_angle(name)
        print(f"plane: interior normals vs the plane's normal, worst {worst:.3e} rad (bound {bound:.3e})")
        assert worst <= bound
    # the Python API takes the same route when its rule for `interpolate` (sizes differ) is the case's
    if c["interp"] == int((c["h"], c["w"]) != (c["H"], c["W"])):
        p2, n2 = PC.unproject(dev(pred), dev(K), size=(c["H"], c["W"]), lo=R.LO, hi=R.HI, normals=True)
        assert p2.cpu().numpy().tobytes() == got_p.tobytes() and n2.cpu().numpy().tobytes() == got_n.tobytes()


def test_same_size_with_and_without_interpolation_agree():
    """After the clip every value is finite, so reading a pixel twice with weights (1, 0) changes nothing."""
    pred, K = R.unproject_inputs("same_24x40_direct")
    a, an = unproject_abi(pred, K, 24, 40, 0)
    b, bn = unproject_abi(pred, K, 24, 40, 1)
    assert a.tobytes() == b.tobytes() and an.tobytes() == bn.tobytes()
    # without a clip (infinite bounds, as compute_errors passes them) an infinite prediction becomes NaN under interpolation only
    assert np.isinf(pred).any()
    a, _ = unproject_abi(pred, K, 24, 40, 0, lo=float("-inf"), hi=float("inf"))
    b, _ = unproject_abi(pred, K, 24, 40, 1, lo=float("-inf"), hi=float("inf"))
    assert np.isinf(a[..., 2]).sum() == np.isinf(pred).sum() and np.array_equal(np.isnan(b[..., 2]), np.isinf(pred))


def test_unproject_python_api():
    pred, K = R.unproject_inputs("odd_19x27_to_37x53")
    P = dev(pred)
    k = tuple(float(v) for v in R.UNPROJECT_CASES["odd_19x27_to_37x53"]["K"][0])
    pts = PC.unproject(P, k, size=(37, 53))
    assert pts.shape == (1, 37, 53, 3) and pts.dtype == torch.float32 and pts.is_cuda
    R.close_points(pts.cpu().numpy(), R.unproject_reference("odd_19x27_to_37x53")[0], "python api")
    both = PC.unproject(P[:, None], dev(K), size=(37, 53), normals=True)                     # [B,1,h,w], tensor intrinsics
    assert torch.equal(both[0], pts)
    into = (torch.zeros_like(pts), torch.zeros_like(pts))
    res = PC.unproject(P, k, size=(37, 53), normals=True, out=into)
    assert res[0] is into[0] and res[1] is into[1] and torch.equal(into[0], pts) and torch.equal(into[1], both[1])
    assert PC.unproject(P, k).shape == (1, 38, 54, 3)                                          # twice the prediction by default
    for bad in (dict(size=(37, 53), out=torch.zeros(1, 37, 53, 3, device=DEV), normals=True), dict(size=(37, 53), out=torch.zeros(1, 36, 53, 3, device=DEV)),
                dict(size=(37, 53), out=torch.zeros(1, 37, 53, 3)), dict(lo=2.0, hi=1.0), dict(size=(0, 5))):
        with pytest.raises(ValueError):
            PC.unproject(P, k, **bad)
    with pytest.raises(ValueError, match="intrinsics"):
        PC.unproject(P, dev(np.ones((2, 4), np.float32)))


# ---- 2. compaction ---------------------------------------------------------------------------------------------------------------------

def _cloud(name, normals, **kw):
    c = R.COMPACT_CASES[name]
    s = R.COMPACT_SHAPES[c["shape"]]
    pred, K, unc = R.compact_inputs(c["shape"])
    args = dict(size=(s["H"], s["W"]), lo=R.LO, hi=R.HI, depth_range=(c["near"], c["far"]), stride=c["stride"], normals=normals)
    if c["unc"] is not None:
        args.update(unc=dev(unc), unc_plane=hip.UNC_STD, unc_range=c["unc"])
    args.update(kw)
    return PC.point_cloud(dev(pred), dev(K), **args), PC.unproject(dev(pred), dev(K), size=(s["H"], s["W"]), lo=R.LO, hi=R.HI, normals=True)


def _check_rows(pc, dense, keep, normals, what, cap=None):
    """counts and indices exactly, rows bitwise equal to the dense map at those indices; -> the per-image counts."""
    B, H, W = keep.shape
    cap = pc.capacity if cap is None else cap
    counts = pc.counts.cpu().numpy()
    assert pc.counts.dtype == torch.int32 and pc.index.dtype == torch.int32
    assert np.array_equal(counts, keep.reshape(B, -1).sum(1)), (what, counts)
    pts, idx = pc.points.cpu().numpy(), pc.index.cpu().numpy()
    nrm = pc.normals.cpu().numpy() if normals else None
    assert (pc.normals is not None) == normals
    dp, dn = dense[0].cpu().numpy().reshape(B, H * W, 3), dense[1].cpu().numpy().reshape(B, H * W, 3)
    for b in range(B):
        want = np.flatnonzero(keep[b])[:cap]
        n = want.size
        assert np.array_equal(idx[b, :n], want), (what, b)
        assert pts[b, :n].tobytes() == dp[b][want].tobytes(), (what, b)
        if normals:
            assert nrm[b, :n].tobytes() == dn[b][want].tobytes(), (what, b)
    return counts


@pytest.mark.parametrize("normals", [True, False])
@pytest.mark.parametrize("name", list(R.COMPACT_CASES))
def test_compaction_matches_the_reference(name, normals):
    c = R.COMPACT_CASES[name]
    s = R.COMPACT_SHAPES[c["shape"]]
    keep, guard = R.compact_reference(name)
    assert guard >= R.GUARD
    pc, dense = _cloud(name, normals)
    full = -(-s["H"] // c["stride"]) * -(-s["W"] // c["stride"])
    assert pc.capacity == full and pc.points.shape == (2, full, 3) and pc.index.shape == (2, full) and pc.size == (s["H"], s["W"])
    counts = _check_rows(pc, dense, keep, normals, name)
    print(f"{name} normals={normals}: kept {counts.tolist()} of {full}")
    if name == "full_none_kept":
        assert (counts == 0).all() and [p["points"].shape[0] for p in pc.split()] == [0, 0]
    if name == "small_all_kept":
        assert counts[0] == full == pc.capacity                                   # count == cap: the last row is written, nothing beyond
    parts = pc.split()
    assert [p["points"].shape[0] for p in parts] == counts.tolist() and all((p["normals"] is not None) == normals for p in parts)
    if c["shape"] == "small" and c["unc"] is None:
        assert np.isnan(dense[0][1].cpu().numpy()).any() and not any(torch.isnan(p["points"]).any() for p in parts)      # the NaN patch is dropped


def test_capacity_below_the_count_reports_the_true_count_and_touches_nothing_beyond():
    """cap = 1000 on small_s1 (1252 and 917 kept): image 0 overflows, image 1 leaves 83 rows; both buffers carry a guard behind them."""
    name, cap, B, H, W = "small_s1", 1000, 2, 37, 53
    c = R.COMPACT_CASES[name]
    keep, _ = R.compact_reference(name)
    want_counts = keep.reshape(B, -1).sum(1)
    assert want_counts[0] > cap > want_counts[1]
    pred, K, _ = R.compact_inputs("small")
    dense = PC.unproject(dev(pred), dev(K), size=(H, W), normals=True)
    guard = 4096
    op = torch.full((B * cap * 3 + guard,), -55.0, dtype=torch.float32, device=DEV)
    on = torch.full((B * cap * 3 + guard,), -66.0, dtype=torch.float32, device=DEV)
    oi = torch.full((B * cap + guard,), -7, dtype=torch.int32, device=DEV)
    cnt = torch.full((B + 8,), -9, dtype=torch.int32, device=DEV)
    nbytes = hip.load().cfp_points_compact_ws_bytes(B, H, W, 1)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    hip.call("cfp_points_compact", dense[0].data_ptr(), dense[1].data_ptr(), H, W, B, 1, c["near"], c["far"], 0, 0, 0, 0, 0.0, 0.0, cap,
             op.data_ptr(), on.data_ptr(), oi.data_ptr(), cnt.data_ptr(), ws.data_ptr(), nbytes, hip.current_stream())
    op, on, oi, cnt = op.cpu().numpy(), on.cpu().numpy(), oi.cpu().numpy(), cnt.cpu().numpy()
    assert cnt[:B].tolist() == want_counts.tolist() and (cnt[B:] == -9).all()
    assert (op[B * cap * 3:] == -55.0).all() and (on[B * cap * 3:] == -66.0).all() and (oi[B * cap:] == -7).all()
    dp, dn = dense[0].cpu().numpy().reshape(B, -1, 3), dense[1].cpu().numpy().reshape(B, -1, 3)
    op, on, oi = op[:B * cap * 3].reshape(B, cap, 3), on[:B * cap * 3].reshape(B, cap, 3), oi[:B * cap].reshape(B, cap)
    for b in range(B):
        want = np.flatnonzero(keep[b])[:cap]
        n = want.size
        assert n == min(want_counts[b], cap) and np.array_equal(oi[b, :n], want)
        assert op[b, :n].tobytes() == dp[b][want].tobytes() and on[b, :n].tobytes() == dn[b][want].tobytes()
        assert (op[b, n:] == -55.0).all() and (on[b, n:] == -66.0).all() and (oi[b, n:] == -7).all()       # rows beyond stay untouched
    # the same through the Python API: the true count comes back, split() refuses
    pc = PC.point_cloud(dev(pred), dev(K), size=(H, W), depth_range=(c["near"], c["far"]), capacity=cap)
    assert pc.counts.cpu().tolist() == want_counts.tolist() and pc.points.shape == (B, cap, 3)
    with pytest.raises(RuntimeError, match="overflow"):
        pc.split()


def test_two_launches_are_bitwise_identical_and_out_is_reused():
    name = "full_s2_unc"
    keep, _ = R.compact_reference(name)
    first, dense = _cloud(name, True)
    again, _ = _cloud(name, True)
    snap = [t.cpu().numpy().tobytes() for t in (first.points, first.normals, first.index, first.counts)]
    n = first.counts.cpu().tolist()
    for b in range(2):                                  # rows beyond the count are not written: compare the rows that are
        for x, y in ((first.points, again.points), (first.normals, again.normals), (first.index, again.index)):
            assert x[b, :n[b]].cpu().numpy().tobytes() == y[b, :n[b]].cpu().numpy().tobytes()
    assert again.counts.cpu().tolist() == n
    # out=: the same tensors come back, rows beyond the counts keep what they held
    for t, v in ((first.points, -55.0), (first.normals, -66.0), (first.index, -7), (first.counts, -9)):
        t.fill_(v)
    c = R.COMPACT_CASES[name]
    pred, K, unc = R.compact_inputs(c["shape"])
    colors = torch.arange(2 * 3 * 480 * 640, dtype=torch.float32, device=DEV).reshape(2, 3, 480, 640)
    res = PC.point_cloud(dev(pred), dev(K), size=(480, 640), depth_range=(c["near"], c["far"]), unc=dev(unc), unc_range=c["unc"], stride=2,
                         colors=colors, out=first)
    assert res is first
    _check_rows(res, dense, keep, True, "out= reuse")
    for b in range(2):
        assert (res.points[b, n[b]:] == -55.0).all() and (res.normals[b, n[b]:] == -66.0).all() and (res.index[b, n[b]:] == -7).all()
        idx = res.index[b, :n[b]].long()
        assert torch.equal(res.colors[b, :n[b]], colors[b].reshape(3, -1)[:, idx].T)         # colours gathered with the index
    assert res.colors.shape == (2, res.capacity, 3)
    with pytest.raises(ValueError, match="out must be"):
        PC.point_cloud(dev(pred), dev(K), size=(480, 640), stride=4, out=first)
    for bad in (dict(stride=0), dict(capacity=0), dict(depth_range=(2.0, 1.0)), dict(unc=dev(unc), unc_range=(1.0, 0.0)), dict(unc=dev(unc[:, :2])),
                dict(unc=dev(unc).double()), dict(unc=dev(unc), unc_plane=3), dict(colors=colors[:, :2]), dict(colors=colors.cpu())):
        with pytest.raises(ValueError):
            PC.point_cloud(dev(pred), dev(K), size=(480, 640), **bad)


# ---- 3. the command line ---------------------------------------------------------------------------------------------------------------

BASE = ["@configs/cfpnet_combine1.txt", "--selected_epoch", "best", "--synthetic", "2", "--batch", "2"]


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


def _read_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    n = int(lines[2].split()[-1])
    dt = np.dtype([(l.split()[2], {"float": "<f4", "uchar": "u1"}[l.split()[1]]) for l in lines[3:-1]])
    assert len(raw) - end == n * dt.itemsize
    return np.frombuffer(raw[end:], dtype=dt)


def test_cli_save_points(tmp_path, monkeypatch):
    from cfpnet_amd import data
    plain, lines0, err0 = _cli(BASE)
    calls = []
    real = PC.point_cloud

    def recording(pred, intrinsics, **kw):
        calls.append((pred.clone(), intrinsics, {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}))
        return real(pred, intrinsics, **kw)

    monkeypatch.setattr(PC, "point_cloud", recording)
    res, lines, err = _cli(BASE + ["--save_points", "--points_stride", "4", "--points_normals", "--points_max_std", str(R.CLI_MAX_STD),
                                   "--save_dir", str(tmp_path)])
    monkeypatch.undo()
    assert res == plain and lines == lines0 and len(lines) == 2                  # the Metrics lines do not change
    assert sum(l.startswith("points: ") for l in err) == 1 and err[-2].startswith("points: ") and not any(l.startswith("points") for l in err0)
    assert sorted(os.listdir(str(tmp_path))) == ["points_0.ply", "points_1.ply"]
    assert len(calls) == 1
    pred, intr, kw = calls[0]
    assert intr == PC.ZJUL5_INTRINSICS and kw["stride"] == 4 and kw["normals"] is True and tuple(kw["size"]) == (480, 640)
    assert kw["unc_range"] == (float("-inf"), R.CLI_MAX_STD) and kw["unc"].shape == (2, 3, 240, 320) and kw["depth_range"] == (1e-3, 10.0)
    direct = real(pred, intr, **kw)                      # point_cloud called directly on what the model produced
    parts = direct.split()
    total = 0
    imgs = next(data.batches(data.SyntheticEvalSamples(2, 480, 640), 2))[0]
    rgb = imgs.numpy() * data.IMAGENET_STD[None, :, None, None] + data.IMAGENET_MEAN[None, :, None, None]
    for b in range(2):
        v = _read_ply(os.path.join(str(tmp_path), f"points_{b}.ply"))
        assert v.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue")
        n = parts[b]["points"].shape[0]
        assert v.size == n == int(direct.counts[b])
        assert np.stack([v["x"], v["y"], v["z"]], 1).tobytes() == parts[b]["points"].cpu().numpy().tobytes()
        assert np.stack([v["nx"], v["ny"], v["nz"]], 1).tobytes() == parts[b]["normals"].cpu().numpy().tobytes()
        idx = parts[b]["index"].cpu().numpy()
        assert (idx // 640 % 4 == 0).all() and (idx % 640 % 4 == 0).all() and (np.diff(idx) > 0).all()
        want_rgb = rgb[b].reshape(3, -1)[:, idx].T
        got_rgb = np.stack([v["red"], v["green"], v["blue"]], 1).astype(np.float64)
        assert 0 < n < 120 * 160                                                   # the limit keeps some pixels and drops some
        assert np.abs(got_rgb - want_rgb * 255.0).max() <= 0.5 + 1e-3             # rounded to the nearest of 0..255
        std = torch.nn.functional.interpolate(kw["unc"][b:b + 1, :1], (480, 640), mode="bilinear", align_corners=True)[0, 0].reshape(-1)[idx]
        assert float(std.max()) <= R.CLI_MAX_STD * (1 + 1e-5)
        assert (v["z"] > 1e-3).all() and (v["z"] < 10.0).all()
        total += n
    print(f"cli: kept {[p['points'].shape[0] for p in parts]} of {120 * 160} candidates per image")
    assert f"{total / 2:.1f}" in err[-2]
    # a run without a limit keeps at least as many; the flags alone are an error
    monkeypatch.setattr(PC, "point_cloud", recording)
    _cli(BASE + ["--save_points", "--save_dir", str(tmp_path / "b"), "--intrinsics", "600,600,320,240"])
    monkeypatch.undo()
    _, intr2, kw2 = calls[1]
    assert intr2 == (600.0, 600.0, 320.0, 240.0) and kw2["stride"] == 2 and kw2["normals"] is False and kw2["unc"] is None
    v = _read_ply(os.path.join(str(tmp_path / "b"), "points_0.ply"))
    assert v.dtype.names == ("x", "y", "z", "red", "green", "blue") and v.size >= parts[0]["points"].shape[0]
    with pytest.raises(ValueError, match="need --save_points"):
        _cli(BASE + ["--points_stride", "4"])
