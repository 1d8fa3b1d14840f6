"""`cfp_depth_unproject` / `cfp_points_compact` without a GPU: the symbols, the header, the workspace query and every argument check
(dummy pointers: no kernel is launched), the Python API's own refusals, the new switches of evaluate_all.py, the PLY writer, the numpy
restatement of the definition (`pointcloud_ref.py`) against itself in float64 and against the metric oracle, and the two measurements the
GPU tests' tolerances rest on: the angle float32 arithmetic alone moves a normal, and the distance of every compaction threshold from
the nearest reference value."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import pointcloud_ref as R

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
    from cfpnet_amd import hip, pointcloud
    for name in ("cfp_depth_unproject", "cfp_points_compact", "cfp_points_compact_ws_bytes"):
        assert hasattr(lib, name)
    text = open(os.path.join(ROOT, "include", "cfpnet_hip.h")).read()
    assert "int cfp_depth_unproject(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi," in text
    assert "size_t cfp_points_compact_ws_bytes(int B, int H, int W, int stride);" in text and "int cfp_points_compact(const float* points" in text
    for cited in ("evaluate_all.py:40-41", "zjuL5.py:66-71", "rx = ((float)x - cx) / fx", "T_x = (d1 - d0) * r_m + (d1 + d0) * (0.5f * k / fx) * e_1",
                  "n = normalize(T_y x T_x)", "finite and that fx, fy are not 0", "row-major pixel order", "TRUE number kept"):
        assert cited in text, cited
    assert len(hip.SIGNATURES["cfp_depth_unproject"][1]) == 13 and len(hip.SIGNATURES["cfp_points_compact"][1]) == 22
    assert len(hip.SIGNATURES["cfp_points_compact_ws_bytes"][1]) == 4 and hip.SIGNATURES["cfp_points_compact_ws_bytes"][0] is ctypes.c_size_t
    mk = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "Makefile")).read()
    assert " pointcloud.hip " in mk and "pointcloud.o: metrics_pred.h" in mk
    src = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "pointcloud.hip")).read()
    assert '#include "metrics_pred.h"' in src and "met_pred(" in src and "met_plane(" in src and "atomic" not in src.replace("no atomics", "")
    assert pointcloud.ZJUL5_INTRINSICS == R.ZJUL5 == (611.2, 609.6, 323.4, 244.9)


def test_ws_bytes(lib):
    ws = lib.cfp_points_compact_ws_bytes
    for bad in ((0, 8, 8, 1), (-1, 8, 8, 1), (1, 0, 8, 1), (1, 8, -2, 1), (1, 8, 8, 0), (1, 8, 8, -1)):
        assert ws(*bad) == 0, bad
    assert ws(1, 1, 1, 1) == 8
    sizes = [(1, 1), (7, 9), (37, 53), (240, 320), (480, 640), (1080, 1920)]
    for B in (1, 2, 3, 8):
        for stride in (1, 2, 3, 7):
            got = [ws(B, h, w, stride) for h, w in sizes]
            assert all(v > 0 and v % 8 == 0 for v in got)
            assert all(a <= b for a, b in zip(got, got[1:])), (B, stride, got)
            assert got[-1] > got[0]
            assert all(ws(B, h, w, stride) <= ws(B + 1, h, w, stride) for h, w in sizes)
            assert all(ws(B, h, w, stride) >= ws(B, h, w, stride + 1) for h, w in sizes)
    assert ws(8, 480, 640, 1) > ws(4, 480, 640, 1) > ws(4, 480, 640, 2) > ws(4, 480, 640, 4)
    # one int per chunk of at most 2^10 candidates is plenty; at least one per image
    assert ws(2, 480, 640, 1) >= 2 * 4 * (480 * 640 // 1024) and ws(5, 3, 3, 1) >= 5 * 4


def test_unproject_refuses_bad_arguments_with_a_message(lib):
    """16 = a non-null, 16-byte aligned dummy device pointer: every case fails a check before anything is dereferenced or launched."""
    from cfpnet_amd import hip
    P = 16

    def call(pred=P, hp=8, wp=8, h=8, w=8, b=1, interp=0, lo=1e-3, hi=10.0, k=P, points=P, normals=0):
        rc = lib.cfp_depth_unproject(pred, hp, wp, h, w, b, interp, lo, hi, k, points, normals, 0)
        return rc, hip.last_error()

    for name in ("pred", "k", "points"):
        rc, msg = call(**{name: 0})
        assert rc == EINVAL and "cfp_depth_unproject: null pointer" in msg, (name, rc, msg)
    for kw in (dict(b=0), dict(h=0), dict(w=-1), dict(hp=0), dict(wp=-3)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "non-positive" in msg, (kw, rc, msg)
    for kw in (dict(hp=4, wp=4), dict(hp=8, wp=4), dict(h=16, w=16)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "sizes differ" in msg, (kw, rc, msg)
    rc, msg = call(h=70000, w=70000, interp=1)
    assert rc == ESHAPE and "too large" in msg
    for lo, hi in ((2.0, 1.0), (1.0, 1.0), (float("nan"), 1.0), (0.0, float("nan"))):
        rc, msg = call(lo=lo, hi=hi)
        assert rc == EINVAL and "empty depth range" in msg, (lo, hi, rc, msg)
    with pytest.raises(RuntimeError, match="cfp_depth_unproject failed"):
        hip.call("cfp_depth_unproject", P, 4, 4, 8, 8, 1, 0, 1e-3, 10.0, P, P, 0, 0)


def test_compact_refuses_bad_arguments_with_a_message(lib):
    from cfpnet_amd import hip
    P, BIG = 16, 1 << 40

    def call(points=P, normals=0, h=8, w=8, b=1, stride=1, near=0.5, far=5.0, unc=0, hu=4, wu=4, ustride=48, ulo=0.0, uhi=1.0, cap=64,
             out_points=P, out_normals=0, out_index=P, counts=P, ws=P, nbytes=BIG):
        rc = lib.cfp_points_compact(points, normals, h, w, b, stride, near, far, unc, hu, wu, ustride, ulo, uhi, cap, out_points, out_normals,
                                    out_index, counts, ws, nbytes, 0)
        return rc, hip.last_error()

    for name in ("points", "out_points", "out_index", "counts", "ws"):
        rc, msg = call(**{name: 0})
        assert rc == EINVAL and "cfp_points_compact: null pointer" in msg, (name, rc, msg)
    for kw in (dict(b=0), dict(h=0), dict(w=-1)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "non-positive" in msg, (kw, rc, msg)
    for kw in (dict(unc=P, hu=0), dict(unc=P, wu=-1)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "non-positive" in msg and "uncertainty" in msg, (kw, rc, msg)
    rc, msg = call(unc=0, hu=0, wu=0, ulo=1.0, uhi=0.0, nbytes=0)                  # no plane: its size and interval are not looked at
    assert rc == EINVAL and "workspace too small" in msg
    rc, msg = call(b=70000)
    assert rc == ESHAPE and "too large" in msg
    for stride in (0, -2):
        rc, msg = call(stride=stride)
        assert rc == EINVAL and "stride must be at least 1" in msg
    for cap in (0, -5):
        rc, msg = call(cap=cap)
        assert rc == EINVAL and "cap must be at least 1" in msg
    for near, far in ((2.0, 1.0), (1.0, 1.0), (float("nan"), 1.0), (1.0, float("nan"))):
        rc, msg = call(near=near, far=far)
        assert rc == EINVAL and "empty depth range" in msg, (near, far, rc, msg)
    for ulo, uhi in ((0.5, 0.25), (float("nan"), 1.0), (0.0, float("nan"))):
        rc, msg = call(unc=P, ulo=ulo, uhi=uhi)
        assert rc == EINVAL and "empty uncertainty interval" in msg, (ulo, uhi, rc, msg)
    rc, msg = call(unc=P, ustride=-1)
    assert rc == EINVAL and "stride" in msg
    for kw in (dict(normals=P), dict(out_normals=P)):
        rc, msg = call(**kw)
        assert rc == EINVAL and "given together" in msg, (kw, rc, msg)
    rc, msg = call(nbytes=lib.cfp_points_compact_ws_bytes(1, 8, 8, 1) - 1)
    assert rc == EINVAL and "workspace too small" in msg
    rc, msg = call(h=480, w=640, b=2, nbytes=lib.cfp_points_compact_ws_bytes(2, 480, 640, 2))        # sized for another stride
    assert rc == EINVAL and "workspace too small" in msg
    rc, msg = call(ws=20)
    assert rc == EINVAL and "8-byte aligned" in msg
    with pytest.raises(RuntimeError, match="cfp_points_compact failed"):
        hip.call("cfp_points_compact", P, 0, 8, 8, 1, 1, 0.5, 5.0, 0, 0, 0, 0, 0.0, 1.0, 0, P, 0, P, P, P, BIG, 0)


def test_python_api_refuses_before_anything_runs(tmp_path):
    import torch
    from cfpnet_amd import hip, pointcloud as PC
    assert list(inspect.signature(PC.unproject).parameters) == ["pred", "intrinsics", "size", "lo", "hi", "normals", "out"]
    sig = inspect.signature(PC.point_cloud)
    assert list(sig.parameters) == ["pred", "intrinsics", "size", "lo", "hi", "depth_range", "unc", "unc_plane", "unc_range", "stride",
                                    "normals", "capacity", "colors", "out"]
    assert sig.parameters["unc_plane"].default == hip.UNC_STD == 0 and sig.parameters["stride"].default == 1
    assert sig.parameters["normals"].default is True and sig.parameters["unc_range"].default == (float("-inf"), float("inf"))
    host = torch.ones(1, 4, 6)
    for fn in (PC.unproject, PC.point_cloud):
        with pytest.raises(ValueError, match="float32 device tensor"):
            fn(host, PC.ZJUL5_INTRINSICS)                                # a host tensor
        with pytest.raises(ValueError, match="float32 device tensor"):
            fn(host.double(), PC.ZJUL5_INTRINSICS)
        with pytest.raises(ValueError, match="float32 device tensor"):
            fn(np.ones((1, 4, 6), np.float32), PC.ZJUL5_INTRINSICS)
    # the helpers behind the remaining refusals take no device
    for bad in ((1.0, 2.0, 3.0), (0.0, 1.0, 2.0, 3.0), (1.0, 0.0, 2.0, 3.0), (float("nan"), 1.0, 2.0, 3.0), (1.0, 1.0, float("inf"), 3.0), 5.0):
        with pytest.raises(ValueError, match="intrinsics"):
            PC._intrinsics(bad, 2, "cpu")
    for bad in (torch.ones(2, 3), torch.ones(3, 4), torch.ones(2, 4, dtype=torch.float64)):
        with pytest.raises(ValueError, match="intrinsics"):
            PC._intrinsics(bad, 2, "cpu")
    k = PC._intrinsics((611.2, -609.6, 323.4, 244.9), 3, "cpu")
    assert k.dtype == torch.float32 and k.tolist() == [[np.float32(611.2), np.float32(-609.6), np.float32(323.4), np.float32(244.9)]] * 3
    assert PC._size(None, 120, 160) == (240, 320) and PC._size((5, 7), 120, 160) == (5, 7)
    for bad in ((0, 4), (4, -1), 7, (1, 2, 3), "ab"):
        with pytest.raises(ValueError, match="size"):
            PC._size(bad, 4, 4)
    for bad in (torch.ones(4, 6), torch.ones(1, 2, 4, 6), torch.ones(0, 4, 6)):
        with pytest.raises(ValueError):
            PC._pred3(bad.to(torch.float32))
    # the result object on host tensors: split trims to the counts and refuses an overflow
    pts = torch.arange(2 * 5 * 3, dtype=torch.float32).reshape(2, 5, 3)
    idx = torch.arange(10, dtype=torch.int32).reshape(2, 5)
    pc = PC.PointCloud(pts, None, idx, None, torch.tensor([2, 5], dtype=torch.int32), 5, (4, 4))
    parts = pc.split()
    assert [p["points"].shape[0] for p in parts] == [2, 5] and torch.equal(parts[0]["index"], idx[0, :2]) and parts[0]["normals"] is None
    pc.counts = torch.tensor([2, 6], dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r"overflow.*\(1, 6\).*capacity 5"):
        pc.split()
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        PC.write_ply(str(tmp_path / "x.ply"), np.zeros((4, 2), np.float32))
    with pytest.raises(ValueError, match="normals"):
        PC.write_ply(str(tmp_path / "x.ply"), np.zeros((4, 3), np.float32), normals=np.zeros((3, 3), np.float32))
    assert not os.path.exists(str(tmp_path / "x.ply"))


def test_evaluate_all_takes_the_switches_off_argv():
    import evaluate_all
    argv = ["--synthetic", "2", "--save_points", "--points_stride", "4", "--points_max_std", "0.25", "--points_normals", "--intrinsics",
            "600,601.5,320,240", "--save_dir", "out"]
    assert evaluate_all._pop(argv, "--save_points", False, None) is True
    assert evaluate_all._pop(argv, "--points_stride", None, int) == 4
    assert evaluate_all._pop(argv, "--points_max_std", None, float) == 0.25
    assert evaluate_all._pop(argv, "--points_normals", False, None) is True
    assert evaluate_all._pop(argv, "--intrinsics", None, evaluate_all._intrinsics) == (600.0, 601.5, 320.0, 240.0)
    assert argv == ["--synthetic", "2", "--save_dir", "out"]              # the reference's own flags stay for its parser
    assert evaluate_all._pop(argv, "--points_stride", None, int) is None
    with pytest.raises(ValueError, match="fx,fy,cx,cy"):
        evaluate_all._intrinsics("600,600,320")
    src = inspect.getsource(evaluate_all.main)
    for flag in ("--save_points", "--points_stride", "--points_max_std", "--points_normals", "--intrinsics"):
        assert f'_pop(argv, "{flag}"' in src, flag
    assert "points_{n_img + b}.ply" in src and "IMAGENET_MEAN" in src and "file=sys.stderr" in src
    # --points_* without --save_points is an error, raised before a device or a model is touched
    for extra in (["--points_stride", "4"], ["--points_max_std", "0.2"], ["--points_normals"], ["--intrinsics", "1,1,0,0"]):
        with pytest.raises(ValueError, match="need --save_points"):
            evaluate_all.main(["--synthetic", "2"] + extra)


def test_ply_round_trip(tmp_path):
    from cfpnet_amd import pointcloud as PC
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(37, 3)).astype(np.float32)
    nrm = rng.normal(size=(37, 3)).astype(np.float32)
    col = rng.random((37, 3)).astype(np.float32)
    col[0], col[1] = (-0.5, 0.0, 0.2), (1.0, 1.5, 0.998)

    def parse(path):
        raw = open(path, "rb").read()
        end = raw.index(b"end_header\n") + len(b"end_header\n")
        lines = raw[:end].decode("ascii").splitlines()
        assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == "end_header"
        n = int(lines[2].split()[-1])
        assert lines[2] == f"element vertex {n}"
        props = [l.split()[1:] for l in lines[3:-1]]
        assert all(l.startswith("property ") for l in lines[3:-1])
        dt = np.dtype([(name, {"float": "<f4", "uchar": "u1"}[t]) for t, name in props])
        assert len(raw) - end == n * dt.itemsize
        return [name for _, name in props], np.frombuffer(raw[end:], dtype=dt)

    f = str(tmp_path / "a.ply")
    assert PC.write_ply(f, pts) == 37
    names, v = parse(f)
    assert names == ["x", "y", "z"] and np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), pts)
    import torch
    assert PC.write_ply(f, torch.from_numpy(pts), torch.from_numpy(nrm), torch.from_numpy(col)) == 37
    names, v = parse(f)
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"] and v.dtype.itemsize == 27
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), pts) and np.array_equal(np.stack([v["nx"], v["ny"], v["nz"]], 1), nrm)
    rgb = np.stack([v["red"], v["green"], v["blue"]], 1)
    assert rgb.dtype == np.uint8 and np.array_equal(rgb, np.clip(np.rint(col.astype(np.float64) * 255), 0, 255).astype(np.uint8))
    assert rgb[0].tolist() == [0, 0, 51] and rgb[1].tolist() == [255, 255, 254]
    u8 = (rng.random((37, 3)) * 255).astype(np.uint8)
    PC.write_ply(f, pts, colors=u8)
    names, v = parse(f)
    assert names == ["x", "y", "z", "red", "green", "blue"] and np.array_equal(np.stack([v["red"], v["green"], v["blue"]], 1), u8)
    assert PC.write_ply(f, np.zeros((0, 3), np.float32)) == 0 and parse(f)[1].size == 0


# ---- the restatement against itself and against the metric oracle -------------------------------------------------------------------------

def test_float32_depth_is_the_protocol_of_the_metric_oracle():
    """`depth` restates met_pred; on finite inputs it agrees with the oracle's clip + F.interpolate(align_corners=True) within the
    project's bound (ATen rounds the blend in another order)."""
    from oracle import metrics_oracle as MO
    for name in ("odd_19x27_to_37x53", "full_240x320_to_480x640"):
        c = R.UNPROJECT_CASES[name]
        pred = R.unproject_inputs(name)[0][0]
        d = R.depth(pred, c["H"], c["W"], 1)
        _, want = MO.protocol_evaluate_all(pred.copy(), np.ones((c["H"], c["W"]), np.float32), R.LO, R.HI)
        assert np.isfinite(d).all() and d.dtype == np.float32
        assert (np.abs(d.ravel() - want) <= R.RTOL * np.maximum(np.abs(want), 1e-3)).all()
        assert d.min() >= np.float32(R.LO) and d.max() <= np.float32(R.HI)
    same = R.unproject_inputs("same_24x40_direct")[0][0]
    assert np.array_equal(R.depth(same, 24, 40, 0), R.depth(same, 24, 40, 1))          # finite after the clip: weights (1, 0) change nothing


@pytest.mark.parametrize("name", list(R.UNPROJECT_CASES))
def test_float64_closed_form_tangents_are_the_point_differences(name):
    c = R.UNPROJECT_CASES[name]
    pred, K = R.unproject_inputs(name)
    for b in range(pred.shape[0]):
        d = R.depth(pred[b], c["H"], c["W"], c["interp"], dt=np.float64)
        ok = R._finite5(d)
        P = R.points(d, K[b])
        n = R.normals(d, K[b])
        for closed, diff in zip(R.tangents_closed(d, K[b]), R.tangents_diff(d, K[b])):
            scale = np.linalg.norm(diff[ok], axis=-1)
            err = np.linalg.norm(closed[ok] - diff[ok], axis=-1)
            assert (err[scale == 0] == 0).all()
            nz = scale > 0
            assert nz.any() or min(c["H"], c["W"]) == 1
            if nz.any():
                print(f"{name} image {b}: closed form vs difference, worst relative {float((err[nz] / scale[nz]).max()):.3e}")
                assert (err[nz] <= 1e-12 * scale[nz]).all()
        nonzero = (n != 0).any(-1)
        assert np.array_equal(nonzero, ok & (min(c["H"], c["W"]) > 1))
        if min(c["H"], c["W"]) == 1:
            assert not nonzero.any()
            continue
        assert np.abs(np.linalg.norm(n[nonzero], axis=-1) - 1.0).max() <= 1e-14
        assert ((n[nonzero] * P[nonzero]).sum(-1) < 0).all()                              # faces the camera
    if name == "plane_48x72":
        inner = n[1:-1, 1:-1].reshape(-1, 3)
        worst = float(R.angle(inner, np.broadcast_to(np.array(R.PLANE_N), inner.shape)).max())
        print(f"plane: float64 normals of the float32 depth samples vs the plane's normal, worst {worst:.3e} rad (bound {R.PLANE_ANGLE_BOUND:.3e})")
        assert worst <= R.PLANE_ANGLE_BOUND and c["K"][0][0] == 60.0 and pred.max() / pred.min() < 2
    if name == "batch3_nonfinite":
        assert (~ok).sum() > 40 and ok.sum() > 1500 and np.isnan(P[..., 2]).sum() > 10


# ---- the two measurements the GPU tolerances rest on --------------------------------------------------------------------------------------

def test_measured_normal_angle_between_the_float32_and_the_float64_restatement():
    """Over the GPU tests' own inputs.  The figure is dominated by the 480 x 640 case: the float32 source coordinate sx * x of the
    protocol's blend is off by up to an ulp of 319, which moves a depth by ~1e-5 of the local contrast, seen over a baseline of
    2 d / fx between the neighbours.  The GPU tolerance is 4 x this (the margin for a kernel that orders the cross product's terms
    differently), so it must stay a small angle for the GPU comparison to mean something."""
    a = R.normal_angle_measured()
    print(f"NORMAL_ANGLE_MEASURED = {a:.4e} rad; GPU tolerance 4 x = {4 * a:.4e} rad = {np.degrees(4 * a):.3f} degrees")
    assert R.NORMAL_ANGLE_MEASURED == a and 0.0 < a and 4 * a < np.radians(1.0)
    for name in R.UNPROJECT_CASES:                                                       # zero normals at the same pixels in both forms
        n32, n64 = R.unproject_reference(name)[1], R.unproject_reference(name, np.float64)[1]
        assert np.array_equal((n32 == 0).all(-1), (n64 == 0).all(-1))
        p32, p64 = R.unproject_reference(name)[0], R.unproject_reference(name, np.float64)[0]
        assert np.array_equal(np.isnan(p32), np.isnan(p64))


@pytest.mark.parametrize("name", list(R.COMPACT_CASES))
def test_no_reference_value_lies_within_the_guard_band_of_a_threshold(name):
    """Then the float32 kernel and the float64 reference cannot disagree about a pixel (their values differ by ~1e-5 relative at most,
    see above), `counts` and `index` are compared exactly and no pixel is excluded from a comparison."""
    c = R.COMPACT_CASES[name]
    s = R.COMPACT_SHAPES[c["shape"]]
    keep, guard = R.compact_reference(name)
    print(f"{name}: kept {keep.sum((1, 2)).tolist()} of {-(-s['H'] // c['stride']) * -(-s['W'] // c['stride'])}, guard band {guard:.3e}")
    assert guard >= R.GUARD
    # the float32 restatement decides every pixel the same way
    pred, K, unc = R.compact_inputs(c["shape"])
    for b in range(2):
        z = R.depth(pred[b], s["H"], s["W"], 1)
        u = None if c["unc"] is None else R.plane_to_grid(unc[b, 0], s["H"], s["W"])
        assert np.array_equal(R.keep_mask(z, c["stride"], c["near"], c["far"], u, c["unc"]), keep[b])
    off = np.ones(keep.shape[1:], bool)
    off[::c["stride"], ::c["stride"]] = False
    assert not keep[:, off].any()
    if name == "full_none_kept":
        assert not keep.any()
    elif name == "small_all_kept":
        assert keep[0].all() and keep[0].sum() == 37 * 53 and 0 < keep[1].sum() < 37 * 53        # image 1 holds a NaN patch
    else:
        assert all(0 < k.sum() < off.size - off.sum() for k in keep)
