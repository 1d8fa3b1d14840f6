"""`cfp_tsdf_integrate_rgb` / `cfp_tsdf_shade` / `cfp_tsdf_surface_rgb` without a GPU: the symbols, the header, every argument check
(dummy pointers: no kernel is launched), the Python API's own refusals and signatures, the numpy restatement (`tsdf_color_ref.py`)
against closed forms, the excluded set the GPU tests' exact comparisons rest on, and the end-to-end colour error of the float64
restatement against the analytic texture."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import pointcloud_ref as P
import tsdf_color_ref as C
import tsdf_ref as S
import tsdf_surface_ref as S2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE = -1, -2
INF, NAN = float("inf"), float("nan")
ID = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)


@pytest.fixture(scope="module")
def lib():
    from cfpnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.load()


def test_symbols_header_and_makefile(lib):
    from cfpnet_amd import hip
    for name in ("cfp_tsdf_integrate_rgb", "cfp_tsdf_shade", "cfp_tsdf_surface_rgb"):
        assert hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "cfpnet_hip.h")).read()
    assert "int cfp_tsdf_integrate_rgb(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi," in text
    assert "int cfp_tsdf_shade(const float* color /* [B][Dz][Dy][Dx][4] */, int Dx, int Dy, int Dz, int B, float ox, float oy, float oz, float voxel," in text
    assert "int cfp_tsdf_surface_rgb(const float* volume /* [B][Dz][Dy][Dx][2] */, const float* color /* [B][Dz][Dy][Dx][4] */" in text
    for cited in ("float [B,Dz,Dy,Dx,4] ON THE DEVICE, 16-byte aligned", "Empty is (0, 0, 0, 0)", "not Wt", "sdf > trunc: nothing",
                  "c_k = rgb[b][k][pix] * cstd[k] + mean[k]", "skipped unless all three are finite",
                  "C_k' = (C_k * Wc + c_k * w) / (Wc + w)", "Wc' = fminf(Wc + w, w_max)", "neither read nor written",
                  "{valid depth seen, updated, behind the surface, coloured}", "bit for\n *           bit what cfp_tsdf_integrate writes",
                  "tw = (wx * wy) * wz", "out_k = num_k / den", "no corner of the cell has Wc > 0", "x fastest, then y, then",
                  "n = e / 3, a = e - 3 * n", "t = F(p) / (F(p) - F(q))", "(1 - t) * C(p) + t * C(q)", "reads nothing",
                  "rows at or beyond min(count, cap) are not written", "CFP_TSDF_COLOURED = 3"):
        assert cited in text, cited
    assert len(hip.SIGNATURES["cfp_tsdf_integrate_rgb"][1]) == 33 and len(hip.SIGNATURES["cfp_tsdf_shade"][1]) == 16
    assert len(hip.SIGNATURES["cfp_tsdf_surface_rgb"][1]) == 11
    assert len(hip.SIGNATURES["cfp_tsdf_integrate"][1]) == 29                         # the plain entry point is what it was
    mk = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "Makefile")).read()
    assert " tsdf_color.hip " in mk and "tsdf_color.o: common.h" in mk
    src = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "tsdf.hip")).read()
    assert "template <bool COLOR>\n__global__ __launch_bounds__(256) void tsdf_integrate_kernel(IntegrateP p)" in src
    assert "tsdf_integrate_kernel<true>" in src and "tsdf_integrate_kernel<false>" in src
    assert src.count("atomicAdd(") == 1 and "atomicAdd(p.counts" in src and "hipMemset" not in src.replace("hipMemsetAsync of these", "")
    col = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "tsdf_color.hip")).read()
    assert "atomic" not in col.replace("no atomics", "") and "float4" in col and "hipMalloc" not in col and "Synchronize" not in col


def _three(*v):
    return (ctypes.c_float * 3)(*v)


def test_integrate_rgb_refuses_bad_arguments_with_a_message(lib):
    """16 = a non-null, 16-byte aligned dummy device pointer: every case fails a check before anything is dereferenced or launched."""
    from cfpnet_amd import hip
    Q = 16
    ok3 = _three(0.4, 0.5, 0.6)

    def call(pred=Q, hp=8, wp=8, h=8, w=8, b=1, interp=0, lo=1e-3, hi=10.0, std=0, hu=8, wu=8, sstride=64, floor=1e-3, k=Q, t=Q, vol=Q,
             dx=4, dy=4, dz=4, ox=0.0, oy=0.0, oz=0.0, voxel=0.05, trunc=0.15, z_near=1e-3, w_max=1e6, rgb=Q, mean=ok3, cstd=ok3, color=Q,
             counts=Q):
        rc = lib.cfp_tsdf_integrate_rgb(pred, hp, wp, h, w, b, interp, lo, hi, std, hu, wu, sstride, floor, k, t, vol, dx, dy, dz, ox, oy, oz,
                                        voxel, trunc, z_near, w_max, rgb, mean, cstd, color, counts, 0)
        return rc, hip.last_error()

    for name in ("pred", "k", "t", "vol", "counts", "rgb", "color"):
        rc, msg = call(**{name: 0})
        assert rc == EINVAL and "cfp_tsdf_integrate_rgb: null pointer" in msg, (name, rc, msg)
    for name in ("mean", "cstd"):
        rc, msg = call(**{name: None})
        assert rc == EINVAL and "cfp_tsdf_integrate_rgb: null pointer" in msg, (name, rc, msg)
        for bad in (NAN, INF, -INF):
            for pos in range(3):
                v = [0.4, 0.5, 0.6]
                v[pos] = bad
                rc, msg = call(**{name: _three(*v)})
                assert rc == EINVAL and "mean and cstd must be finite" in msg, (name, bad, pos, rc, msg)
    for bad in (20, 24, 17):
        rc, msg = call(color=bad)
        assert rc == EINVAL and "color must be 16-byte aligned" in msg, (bad, rc, msg)
    # everything cfp_tsdf_integrate refuses, under this entry point's name
    for kw in (dict(b=0), dict(h=0), dict(w=-1), dict(hp=0), dict(wp=-3), dict(dx=0), dict(dy=-1), dict(dz=0), dict(std=Q, hu=0),
               dict(std=Q, wu=-1)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "cfp_tsdf_integrate_rgb: non-positive" in msg, (kw, rc, msg)
    for kw in (dict(hp=4, wp=4), dict(hp=8, wp=4), dict(h=16, w=16)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "sizes differ" in msg, (kw, rc, msg)
    for kw in (dict(h=70000, w=70000, interp=1), dict(hp=70000, wp=70000, interp=1), dict(b=70000), dict(h=1, w=(1 << 24) + 1, interp=1),
               dict(dx=2048, dy=2048, dz=512), dict(dx=1 << 16, dy=1 << 16, dz=1), dict(dx=(1 << 24) + 1, dy=1, dz=1),
               dict(std=Q, hu=70000, wu=70000)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "too large" in msg, (kw, rc, msg)
    for lo, hi in ((2.0, 1.0), (1.0, 1.0), (NAN, 1.0), (0.0, NAN)):
        rc, msg = call(lo=lo, hi=hi)
        assert rc == EINVAL and "empty depth range" in msg, (lo, hi, rc, msg)
    for word, key in (("voxel", "voxel"), ("trunc", "trunc"), ("z_near", "z_near"), ("std_floor", "floor"), ("w_max", "w_max")):
        for bad in (0.0, -1.0, NAN, INF):
            rc, msg = call(**{key: bad})
            assert rc == EINVAL and f"cfp_tsdf_integrate_rgb: {word} must be positive and finite" in msg, (key, bad, rc, msg)
    rc, msg = call(std=Q, sstride=-1)
    assert rc == EINVAL and "stride" in msg
    for kw in (dict(ox=NAN), dict(oy=INF), dict(oz=-INF)):
        rc, msg = call(**kw)
        assert rc == EINVAL and "origin must be finite" in msg, (kw, rc, msg)
    rc, msg = call(vol=20)
    assert rc == EINVAL and "volume must be 8-byte aligned" in msg
    with pytest.raises(RuntimeError, match="cfp_tsdf_integrate_rgb failed"):
        hip.call("cfp_tsdf_integrate_rgb", Q, 8, 8, 8, 8, 1, 0, 1e-3, 10.0, 0, 0, 0, 0, 1e-3, Q, Q, Q, 4, 4, 4, 0.0, 0.0, 0.0, 0.05, 0.15, 1e-3,
                 1e6, 0, ok3, ok3, Q, Q, 0)


def test_shade_refuses_bad_arguments_with_a_message(lib):
    from cfpnet_amd import hip
    Q = 16

    def call(color=Q, dx=4, dy=4, dz=4, b=1, ox=0.0, oy=0.0, oz=0.0, voxel=0.05, k=Q, t=Q, hd=8, wd=8, depth=Q, out=Q):
        rc = lib.cfp_tsdf_shade(color, dx, dy, dz, b, ox, oy, oz, voxel, k, t, hd, wd, depth, out, 0)
        return rc, hip.last_error()

    for name in ("color", "k", "t", "depth", "out"):
        rc, msg = call(**{name: 0})
        assert rc == EINVAL and "cfp_tsdf_shade: null pointer" in msg, (name, rc, msg)
    for kw in (dict(b=0), dict(dx=0), dict(dy=-1), dict(dz=0), dict(hd=0), dict(wd=-2)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "non-positive" in msg, (kw, rc, msg)
    for kw in (dict(dx=2048, dy=2048, dz=512), dict(dx=(1 << 24) + 1, dy=1, dz=1), dict(hd=70000, wd=70000), dict(hd=1, wd=(1 << 24) + 1),
               dict(b=70000)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "too large" in msg, (kw, rc, msg)
    for bad in (0.0, -1.0, NAN, INF):
        rc, msg = call(voxel=bad)
        assert rc == EINVAL and "voxel must be positive and finite" in msg, (bad, rc, msg)
    for kw in (dict(ox=NAN), dict(oy=INF), dict(oz=-INF)):
        rc, msg = call(**kw)
        assert rc == EINVAL and "origin must be finite" in msg, (kw, rc, msg)
    rc, msg = call(color=24)
    assert rc == EINVAL and "color must be 16-byte aligned" in msg
    with pytest.raises(RuntimeError, match="cfp_tsdf_shade failed"):
        hip.call("cfp_tsdf_shade", Q, 4, 4, 4, 1, 0.0, 0.0, 0.0, 0.05, Q, Q, 8, 8, 0, Q, 0)


def test_surface_rgb_refuses_bad_arguments_with_a_message(lib):
    from cfpnet_amd import hip
    Q = 16

    def call(vol=Q, color=Q, dx=4, dy=4, dz=4, b=1, index=Q, counts=Q, cap=8, colors=Q):
        rc = lib.cfp_tsdf_surface_rgb(vol, color, dx, dy, dz, b, index, counts, cap, colors, 0)
        return rc, hip.last_error()

    for name in ("vol", "color", "index", "counts", "colors"):
        rc, msg = call(**{name: 0})
        assert rc == EINVAL and "cfp_tsdf_surface_rgb: null pointer" in msg, (name, rc, msg)
    for kw in (dict(b=0), dict(dx=0), dict(dy=-1), dict(dz=0)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "non-positive" in msg, (kw, rc, msg)
    for kw in (dict(dx=1024, dy=1024, dz=683), dict(dx=1 << 16, dy=1 << 16, dz=1), dict(b=70000)):      # 3 * 1024 * 1024 * 683 >= 2^31
        rc, msg = call(**kw)
        assert rc == ESHAPE and "too large" in msg, (kw, rc, msg)
    assert call(dx=1024, dy=1024, dz=682, vol=20)[0] == EINVAL                        # the largest volume passes the size check
    for bad in (0, -1):
        rc, msg = call(cap=bad)
        assert rc == EINVAL and "cap must be at least 1" in msg, (bad, rc, msg)
    rc, msg = call(vol=20)
    assert rc == EINVAL and "volume must be 8-byte aligned" in msg
    rc, msg = call(color=24)
    assert rc == EINVAL and "color must be 16-byte aligned" in msg
    with pytest.raises(RuntimeError, match="cfp_tsdf_surface_rgb failed"):
        hip.call("cfp_tsdf_surface_rgb", Q, Q, 4, 4, 4, 1, Q, Q, 0, Q, 0)


def test_python_api_signatures_and_refusals_before_anything_runs(tmp_path):
    import torch
    from cfpnet_amd import render, tracking, tsdf as TS
    names = lambda f: list(inspect.signature(f).parameters)
    # frozen
    assert names(TS.TsdfVolume.integrate) == ["self", "pred", "unc", "pose"]
    assert names(TS.TsdfVolume.raycast) == ["self", "pose", "intrinsics", "size", "t_range", "step", "normals", "out"]
    assert names(TS.TsdfVolume.surface_points) == ["self", "capacity", "w_min", "max_jump", "normals", "out"]
    assert names(TS.TsdfVolume.surface_count) == ["self", "w_min", "max_jump"]
    assert names(TS.TsdfVolume.write_ply) == ["self", "path_pattern", "options"]
    assert inspect.signature(TS.TsdfVolume.write_ply).parameters["options"].kind == inspect.Parameter.VAR_KEYWORD
    assert names(tracking.Tracker.track) == ["self", "pred", "unc"] and names(tracking.Tracker.update) == ["self", "pred", "unc", "integrate"]
    assert names(TS.SurfacePoints.__init__) == ["self", "points", "normals", "std", "index", "counts", "capacity", "colors"]
    assert inspect.signature(TS.SurfacePoints.__init__).parameters["colors"].default is None
    # new
    ps = inspect.signature(TS.TsdfVolume.integrate_rgb).parameters
    assert list(ps) == ["self", "pred", "rgb", "unc", "pose", "mean", "std"]
    assert (ps["unc"].default, ps["pose"].default, ps["mean"].default, ps["std"].default) == (None, None, render.IMAGENET_MEAN, render.IMAGENET_STD)
    ps = inspect.signature(TS.TsdfVolume.shade).parameters
    assert list(ps) == ["self", "depth", "pose", "intrinsics", "out"] and all(ps[k].default is None for k in ("pose", "intrinsics", "out"))
    ps = inspect.signature(TS.TsdfVolume.surface_colors).parameters
    assert list(ps) == ["self", "sp", "out"] and ps["out"].default is None
    ps = inspect.signature(tracking.Tracker.update_rgb).parameters
    assert list(ps) == ["self", "pred", "rgb", "unc", "integrate", "mean", "std"]
    assert (ps["unc"].default, ps["integrate"].default, ps["mean"].default, ps["std"].default) == (None, True, render.IMAGENET_MEAN, render.IMAGENET_STD)
    assert TS.COUNT_NAMES == ("seen", "updated", "behind") and TS.COLOR_COUNT_NAMES == ("seen", "updated", "behind", "coloured")
    sp = TS.SurfacePoints(1, 2, 3, 4, 5, 6)
    assert sp.colors is None and sp.capacity == 6
    v = TS.TsdfVolume((4, 5, 6), 0.05, (0, 0, 1), P.ZJUL5)
    assert v.color is None and v.color_counts is None
    with pytest.raises(AttributeError):
        v.color = 1                                                                   # read-only
    host, img = torch.ones(1, 4, 6), torch.ones(1, 3, 8, 12)
    for bad in (img, img.double(), img[0], None, img.numpy()):                        # a host, float64, 3-d tensor, nothing, an array
        with pytest.raises(ValueError, match="rgb must be a float32 device tensor"):
            v.integrate_rgb(host, bad)
    with pytest.raises(ValueError, match="nothing was coloured yet"):
        v.shade(host)
    with pytest.raises(ValueError, match="nothing was coloured yet"):
        v.surface_colors(sp)
    with pytest.raises(ValueError, match="nothing was coloured yet"):
        v.write_ply(str(tmp_path / "map_{}.ply"), colors=True)
    with pytest.raises(ValueError, match="nothing was integrated"):                   # the default goes the way it always went
        v.write_ply(str(tmp_path / "map_{}.ply"))
    with pytest.raises(ValueError, match="nothing was integrated"):
        v.write_ply(str(tmp_path / "map_{}.ply"), colors=False)
    v.reset()
    assert v.color is None and not list(tmp_path.iterdir())
    tr = tracking.Tracker(v)
    with pytest.raises(ValueError, match="rgb must be a float32 device tensor"):
        tr.update_rgb(host, img)


# ---- the restatement against closed forms --------------------------------------------------------------------------------------------------

K0 = (30.0, 29.0, 15.5, 10.5)
DIMS0, ORG0, VOX0, TR0 = (9, 7, 21), (-0.2, -0.15, 1.0), 0.05, 0.15
M0, S0 = (0.25, 0.5, 0.125), (0.25, 0.5, 2.0)                                       # float32 numbers, like every number of the frames below
X1, X2 = (0.75, -0.5, 0.125), (-0.5, 0.25, 0.25)
CONST = np.array(M0) + np.array(S0) * np.array(X1)                                   # c = x * std + mean of the first image


def _zs():
    return float(np.float32(ORG0[2])) + float(np.float32(VOX0)) * np.arange(DIMS0[2])


def _frame(Z, std, x=X1, H=21, W=31):
    d = np.full((H, W), Z, np.float64)
    img = np.stack([np.full((H, W), v, np.float64) for v in x])
    return d, (None if std is None else np.full((H, W), std, np.float64)), img


def _run(vol, col, Z, std, x=X1, w_max=S.F32_MAX):
    d, s, img = _frame(Z, std, x)
    return C.integrate_rgb(vol, col, d, s, img, M0, S0, K0, ID, DIMS0, ORG0, VOX0, TR0, w_max=w_max)


def test_one_observation_of_a_fronto_parallel_plane_with_a_constant_image():
    """Exactly the voxels with |sdf| <= trunc take the constant, with Wc = w; the geometry is tsdf_ref.integrate's."""
    Z, std = 1.52, 0.04
    r = _run(S.empty_volume(DIMS0, np.float64), C.empty_color(DIMS0, np.float64), Z, std)
    g = S.integrate(S.empty_volume(DIMS0, np.float64), *_frame(Z, std)[:2], K0, ID, DIMS0, ORG0, VOX0, TR0)
    assert r["vol"].tobytes() == g["vol"].tobytes() and C.counts_of(r)[:3] == S.counts_of(g)
    tr = float(np.float32(TR0))
    want = np.broadcast_to((np.abs(Z - _zs()) <= tr)[:, None, None], r["coloured"].shape)
    assert np.array_equal(r["coloured"], want) and want[:, 0, 0].sum() == 6 and (r["updated"] & ~r["coloured"]).any()
    assert C.counts_of(r)[3] == int(want.sum())
    col = r["col"]
    assert np.abs(col[want][:, :3] - CONST).max() < 1e-12 and np.abs(col[want][:, 3] - 1 / std ** 2).max() < 1e-9
    assert (col[~want] == 0).all()                                                    # free space and what lies behind stay empty


def test_two_observations_average_by_weight_and_w_max_caps():
    vol0, col0 = S.empty_volume(DIMS0, np.float64), C.empty_color(DIMS0, np.float64)
    x1, x2 = X1, X2
    a = _run(vol0, col0, 1.50, 1.0, x1)                                                # w = 1
    s3 = 1.0 / np.sqrt(3.0)
    b = _run(a["vol"], a["col"], 1.50, s3, x2)                                        # w = 3
    both = a["coloured"] & b["coloured"]
    c1 = np.array(M0) + np.array(S0) * np.array(x1)
    c2 = np.array(M0) + np.array(S0) * np.array(x2)
    assert both.sum() > 100 and np.abs(b["col"][both][:, :3] - (c1 + 3 * c2) / 4).max() < 1e-12      # the 1 : 3 mean
    assert np.abs(b["col"][both][:, 3] - 4.0).max() < 1e-9
    c = _run(a["vol"], a["col"], 1.50, s3, x2, w_max=2.5)
    assert (c["col"][both][:, 3] == 2.5).all() and np.array_equal(c["col"][..., :3], b["col"][..., :3])      # the cap binds the weight only
    n = _run(vol0, col0, 1.50, None, x1)
    assert (n["col"][n["coloured"]][:, 3] == 1.0).all()                               # no std: w = 1
    nan = _run(vol0, col0, 1.50, 1.0, (0.75, NAN, 0.125))                               # one channel NaN: no colour, the geometry still updates
    assert not nan["coloured"].any() and (nan["col"] == 0).all() and np.array_equal(nan["updated"], a["updated"]) and nan["band"].any()
    # a second observation further back colours other voxels; where only one coloured, that colour stays
    far = _run(a["vol"], a["col"], 1.70, 1.0, x2)
    only_a, only_b = a["coloured"] & ~far["coloured"], far["coloured"] & ~a["coloured"]
    assert only_a.any() and only_b.any()
    assert np.abs(far["col"][only_a][:, :3] - c1).max() < 1e-12 and np.abs(far["col"][only_b][:, :3] - c2).max() < 1e-12


def test_shading_the_plane_returns_the_constant_and_an_edge_with_one_uncoloured_end_takes_the_other():
    Z = 1.52
    r = _run(S.empty_volume(DIMS0, np.float64), C.empty_color(DIMS0, np.float64), Z, 0.04)
    ray = S.raycast(r["vol"], K0, ID, 21, 31, ORG0, VOX0, 0.5, 2.5, 0.075)
    hit = ray["hit"] >= 0
    rgb = C.shade(r["col"], K0, ID, ray["depth"], ORG0, VOX0)
    assert 20 < hit.sum() < hit.size and np.abs(rgb[hit] - CONST).max() < 1e-12 and np.isnan(rgb[~hit]).all()
    # a depth in free space, more than a cell in front of the band: inside the grid, but no corner has a colour
    free = C.shade(r["col"], K0, ID, np.full((21, 31), 1.2), ORG0, VOX0)
    assert np.isnan(free).all()
    # a depth at the front rim of the band: only the far corners of the cell have a colour, and the blend is renormalised over them
    rim = C.shade(r["col"], K0, ID, np.full((21, 31), 1.36), ORG0, VOX0)
    inside = ~np.isnan(rim).any(-1)
    assert inside.sum() > 20 and np.abs(rim[inside] - CONST).max() < 1e-12
    # surface colours: the plane's crossings have two coloured ends; emptying one end leaves the other's colour; both: NaN
    s = S2.surface(r["vol"], ORG0, VOX0)
    got = C.surface_rgb(r["vol"], r["col"], s["index"])
    assert len(s["index"]) > 20 and (got["ends"] == 2).all() and np.abs(got["colors"] - CONST).max() < 1e-12
    col = r["col"].copy()
    marked = np.array([0.1, 0.2, 0.7])
    n = s["index"] // 3
    q = n + np.where(s["axis"] == 0, 1, np.where(s["axis"] == 1, DIMS0[0], DIMS0[0] * DIMS0[1]))
    col.reshape(-1, 4)[q, :3] = marked                                                # q's colour differs from p's ...
    col.reshape(-1, 4)[n[::2]] = 0                                                    # ... and every other p has none
    got = C.surface_rgb(r["vol"], col, s["index"])
    assert (got["ends"][::2] == 1).all() and np.abs(got["colors"][::2] - marked).max() < 1e-12
    t = s["t"][1::2, None]
    assert (got["ends"][1::2] == 2).all() and np.abs(got["colors"][1::2] - ((1 - t) * CONST + t * marked)).max() < 1e-12
    col.reshape(-1, 4)[q] = 0
    got = C.surface_rgb(r["vol"], col, s["index"])
    assert (got["ends"][::2] == 0).all() and np.isnan(got["colors"][::2]).all() and (got["ends"][1::2] == 1).all()
    bad = C.surface_rgb(r["vol"], col, np.array([-7, 3 * np.prod(DIMS0), 2 ** 31 - 1, 3 * (DIMS0[0] - 1)]))      # the last: +x leaves the grid
    assert (bad["ends"] == -1).all() and np.isnan(bad["colors"]).all()


# ---- the cases of the GPU tests ------------------------------------------------------------------------------------------------------------

def test_the_images_hold_what_the_gpu_tests_need():
    imgs = C.images()
    assert len(imgs) == len(S.POSES) and all(i.shape == (S.B, 3) + S.GRID and i.dtype == np.float32 for i in imgs)
    b, k, rows, cols = C.NAN_PATCH
    nan = np.isnan(imgs[0])
    assert nan[b, k, rows, cols].all() and nan.sum() == nan[b, k, rows, cols].size and not any(np.isnan(i).any() for i in imgs[1:])
    assert {int(C.render(0, bb)[1].min()) for bb in range(S.B)} == {C.WALL} and all((C.render(0, bb)[1] == C.SPHERE).mean() > 0.05 for bb in range(S.B))
    back = imgs[1] * np.array(C.CSTD, np.float32)[:, None, None] + np.array(C.MEAN, np.float32)[:, None, None]
    assert back.min() > 0.09 and back.max() < 0.91 and np.abs(back[0] - C.render(1, 0)[0]).max() < 1e-6
    assert all(abs(m) > 0.1 for m in C.MEAN) and all(abs(s - 1) > 0.1 for s in C.CSTD) and min(C.LIPSCHITZ) > 0.3
    pi = C.pix_image()
    assert np.array_equal(C.pix_of(pi[1, 0].ravel()), np.arange(S.GRID[0] * S.GRID[1]))


@pytest.mark.parametrize("name", list(S.TSDF_CASES))
def test_at_most_one_percent_of_a_step_is_excluded_and_the_rest_agrees_on_what_is_coloured(name):
    worst = 0.0
    for f in range(len(S.POSES)):
        for b in range(S.B):
            a, d, ex = C.step_reference(name, f, b), C.step_reference(name, f, b, np.float64), C.step_excluded(name, f, b)
            differ = a["coloured"] != d["coloured"]
            n = C.counts_of(d)
            worst = max(worst, float(ex.mean()))
            print(f"{name} frame {f} image {b}: counts {n}, excluded {ex.mean():.5f}, float32 and float64 differ at {int(differ.sum())} voxels, "
                  f"{int((differ & ~ex).sum())} outside the excluded set")
            assert ex.mean() <= C.MAX_EXCLUDED and not (differ & ~ex).any()
            assert (ex >= S.step_excluded(name, f, b)).all()
            assert a["vol"].tobytes() == S.step_reference(name, f, b)["vol"].tobytes()             # the geometry is tsdf_ref's, bit for bit
            if name == "outside_the_view":
                assert n == [0, 0, 0, 0] and a["col"].tobytes() == C.color_states(name)[f][b].tobytes()
            else:
                assert 3000 < n[3] < n[1] and (d["updated"] & ~d["band"]).sum() > 5000             # free space in front is updated, not coloured
                assert not (d["coloured"] & ~d["updated"]).any()
    print(f"{name}: at most {100 * worst:.3f} % of a step excluded (cap {100 * C.MAX_EXCLUDED:.0f} %)")
    if name != "outside_the_view":
        b, k, rows, cols = C.NAN_PATCH                                                # the NaN patch is read, colours nothing, and the geometry updates
        d = C.step_reference(name, 0, b, np.float64)
        H, W = S.GRID
        patch = np.zeros((H, W), bool)
        patch[rows, cols] = True
        reads = (d["pix"] >= 0) & patch.ravel()[np.maximum(d["pix"], 0)]
        assert (reads & d["band"]).sum() > 50 and not (reads & d["coloured"]).any() and (reads & d["updated"]).sum() > 50


def test_every_surface_point_has_a_colour_and_some_only_one_coloured_end():
    for name in S2.STATE_CASES:
        for b in range(S.B):
            r, r64 = C.surface_reference(name, b), C.surface_reference(name, b, dt=np.float64)
            e = r["ends"]
            print(f"{name} image {b}: {e.size} points, {100 * (e == 2).mean():.1f} % with both ends coloured, {int((e == 1).sum())} with one")
            assert e.size > 1000 and (e >= 1).all() and (e == 1).any() and 0.85 < (e == 2).mean() < 0.99
            assert not np.isnan(r["colors"]).any() and np.array_equal(e, r64["ends"])
            assert np.abs(r["colors"] - r64["colors"]).max() < 1e-5
            jump = C.surface_reference(name, b, 0.0, S2.JUMP)
            assert 0 < jump["ends"].size <= e.size and (jump["ends"] >= 1).all()


def _aside(X, b, radius, slack):
    """Points set aside: some frame has, within `radius` pixels of the point's projection, a pixel of the OTHER surface than the one the
    point is nearest to whose true depth lies within `slack` of the point's camera depth -- a sample that can have coloured a voxel the
    point blends.  These are the points next to the sphere's silhouette; a wall point the sphere merely hides in a frame is kept."""
    H, W = S.GRID
    out = np.zeros(len(X), bool)
    near = C.label_of(X)
    xs, ys = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    for f in range(len(S.POSES)):
        fx, fy, cx, cy = (float(np.float32(v)) for v in S.K_GRID[b])
        M = np.asarray(S.POSES[f][b], np.float64).reshape(3, 4)
        Pc = X @ M[:, :3].T + M[:, 3]
        u, v = np.rint(fx * Pc[:, 0] / Pc[:, 2] + cx).astype(int), np.rint(fy * Pc[:, 1] / Pc[:, 2] + cy).astype(int)
        lab, d0 = C.render(f, b)[1], S.scene_depth(S.K_GRID[b], S.POSES[f][b], xs, ys)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                uu, vv = u + dx, v + dy
                inside = (uu >= 0) & (uu < W) & (vv >= 0) & (vv < H)
                uc, vc = np.clip(uu, 0, W - 1), np.clip(vv, 0, H - 1)
                out |= inside & (lab[vc, uc] != near) & (np.abs(d0[vc, uc] - Pc[:, 2]) <= slack)
    return out


def test_end_to_end_colour_error_against_the_analytic_texture():
    """The float64 restatement, `direct_48x64`, three frames: the colour of every extracted surface point and of every shaded raycast
    hit against the analytic texture at the nearest scene point, per channel.

    The bound.  A point X takes a convex combination (inverse-variance means per voxel, then 0 <= t <= 1 along the edge or the
    non-negative trilinear weights of the cell) of image samples, so its error is at most the largest |texture(sample) - texture(N(X))|,
    N(X) the nearest scene point, and that is at most LIPSCHITZ[k] * |sample - N(X)| as long as both lie on the same surface (points for
    which they may not are set aside, below).  Where a sample sits: a coloured voxel V with camera coordinates r(u, v) * Zc read the pixel
    px with |(u, v) - px| <= 1/2 in both coordinates, whose prediction d obeys |d - Zc| <= trunc; the image was rendered at the true hit
    point r(px) * d0 with |d - d0| <= noise, the largest |pred - scene| of the case's frames (the prediction is on the grid itself here,
    so nothing is blended).  Hence
        |V - sample| <= |r(u, v) - r(px)| * Zc + |r(px)| * |Zc - d0| <= 1/2 * sqrt(1 / fx^2 + 1 / fy^2) * (d_max + trunc) + |r|_max * (trunc + noise)
    with fx, fy the smallest focal lengths and |r|_max = |(rx, ry, 1)| at the grid's corners for the cases' intrinsics: half a pixel's
    footprint plus the band along the ray.  X lies within `reach` of the voxels it blends: a voxel for a point on a lattice edge,
    sqrt(3) voxels (a cell's diagonal) for a raycast hit.  And |X - N(X)| <= |X - sample| because the sample is a scene point.  Together
        |sample - N(X)| <= |sample - X| + |X - N(X)| <= 2 * (reach + |V - sample|).
    Set aside: points within a voxel or so of the sphere's silhouette, where samples of both surfaces mix.  A voxel within `reach` of X
    projects within f_max * reach / z_min + 1/2 pixels of X's projection and its camera depth is within `reach` of X's; it takes a
    pixel's colour only if the pixel's depth is within trunc + noise of its own.  So X is set aside iff in some frame a pixel of the
    other surface than the one X is nearest to lies inside that window with a true depth within trunc + noise + reach of X's.  In this
    scene the wall is 0.45 m behind the sphere's rim, more than that depth slack, so the rule sets no point aside: a voxel next to the
    silhouette is either behind the sphere's pixels or in free space in front of the wall's, and takes no colour from the wrong one.
    That is the colour band at work, and the test says so by asserting the bound for every point."""
    name = "direct_48x64"
    H, W = S.GRID
    noise = d_max = 0.0
    z_min = np.inf
    for f, (pred, _, _) in enumerate(S.frames(name)):
        for b in range(S.B):
            truth = S.scene_depth(S.K_GRID[b], S.POSES[f][b], np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
            fin = np.isfinite(pred[b])
            noise = max(noise, float(np.abs(pred[b][fin] - truth[fin]).max()))
            d_max, z_min = max(d_max, float(pred[b][fin].max())), min(z_min, float(pred[b][fin].min()))
    fx, fy = min(k[0] for k in S.K_GRID), min(k[1] for k in S.K_GRID)
    f_max = max(max(k[0], k[1]) for k in S.K_GRID)
    r_max = max(np.sqrt(1 + (max(k[2], W - 1 - k[2]) / k[0]) ** 2 + (max(k[3], H - 1 - k[3]) / k[1]) ** 2) for k in S.K_GRID)
    at_voxel = 0.5 * np.sqrt(1 / fx ** 2 + 1 / fy ** 2) * (d_max + S.TRUNC) + r_max * (S.TRUNC + noise)
    L = np.array(C.LIPSCHITZ)
    col = C.final_color64(name)
    results = {}
    for what, reach in (("surface points", S.VOXEL), ("raycast hits", np.sqrt(3.0) * S.VOXEL)):
        bound = L * 2.0 * (reach + at_voxel) + 1e-6                                   # 1e-6: the image is stored in float32
        radius = int(np.ceil(f_max * reach / (z_min - S.TRUNC) + 0.5))
        errs, aside, total = [], 0, 0
        for b in range(S.B):
            if what == "surface points":
                ref = S2.reference(name, b, dt=np.float64)
                X = ref["points"]
                got = C.surface_rgb(S.states(name)[-1][b].astype(np.float64), col[b], ref["index"])["colors"]
            else:
                rc = S.RAYCAST_CASES["direct_to_37x53"]
                ray = S.raycast_reference("direct_to_37x53", b, np.float64)
                rgb = C.shade(col[b], rc["K"][b], rc["T"][b], ray["depth"], S.TSDF_CASES[name]["origin"], S.VOXEL)
                hit = ~np.isnan(ray["depth"])
                assert not np.isnan(rgb[hit]).any() and np.isnan(rgb[~hit]).all()     # every hit has a colour
                fxr, fyr, cxr, cyr = (float(np.float32(v)) for v in rc["K"][b])
                M = np.asarray(rc["T"][b], np.float64).reshape(3, 4)
                ys, xs = np.nonzero(hit)
                dd = ray["depth"][hit]
                X = (np.stack([(xs - cxr) / fxr * dd, (ys - cyr) / fyr * dd, dd], -1) - M[:, 3]) @ M[:, :3]
                got = rgb[hit]
            assert not np.isnan(got).any()
            skip = _aside(X, b, radius, S.TRUNC + noise + reach)
            want = C.texture(C.nearest_scene_point(X), C.label_of(X))
            err = np.abs(got - want)[~skip]
            errs.append(err)
            aside += int(skip.sum())
            total += len(X)
        err = np.concatenate(errs)
        results[what] = (float(np.median(err)), err.max(0))
        print(f"{name} {what}: {total} points, {aside} set aside (window radius {radius} px), colour error median {np.median(err):.4f}, "
              f"maximum per channel {np.round(err.max(0), 4).tolist()}, bound {np.round(bound, 4).tolist()} "
              f"(|V - sample| <= {at_voxel:.3f} m, noise {noise:.4f} m, |r|_max {r_max:.3f})")
        assert aside < 0.25 * total and len(err) > 2000
        assert (err.max(0) <= bound).all(), (what, err.max(0), bound)
        assert (bound < 0.8).all()                                                    # the texture spans 0.1 .. 0.9: the bound says something
