"""`cfp_tsdf_surface` without a GPU: the symbols, the header, every argument check (dummy pointers: no kernel is launched), the workspace
sizes, the Python API's own refusals, the numpy restatement of the definition (`tsdf_surface_ref.py`) against two closed forms, the
float32 restatement against the float64 one on every input of the GPU tests, and the extracted points against the analytic scene.

Bounds of float32 against float64 (the figures are printed): the index lists and the NaN-normal rows are identical; the normals differ by
at most 2e-6 rad, a tenth of what the GPU test allows against the float64 restatement; the points by at most 1e-6 m, four units in the last
place of a 2 m coordinate for the three rounded operations of `o + voxel * (idx + t)`; the std by at most 1e-5 relative, half the project's
2e-5 (the blend `(1 - t) * Wt(p) + t * Wt(q)` loses up to eps * max(Wt) / min(Wt) when the weights differ by three orders of magnitude).
Measured: 8.4e-7 rad, 2.7e-7 m, 2.1e-6."""
import inspect
import os

import numpy as np
import pytest

import tsdf_ref as S
import tsdf_surface_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE = -1, -2
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from cfpnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.load()


def test_symbols_header_and_makefile(lib):
    import ctypes as C
    from cfpnet_amd import hip
    assert hasattr(lib, "cfp_tsdf_surface") and hasattr(lib, "cfp_tsdf_surface_ws_bytes")
    p, i, f, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    assert hip.SIGNATURES["cfp_tsdf_surface_ws_bytes"] == (sz, [i, i, i, i])
    assert hip.SIGNATURES["cfp_tsdf_surface"] == (i, [p, i, i, i, i, f, f, f, f, f, f, i, p, p, p, p, p, p, sz, p])
    assert lib.cfp_tsdf_surface.argtypes == hip.SIGNATURES["cfp_tsdf_surface"][1] and lib.cfp_tsdf_surface_ws_bytes.restype is sz
    text = open(os.path.join(ROOT, "include", "cfpnet_hip.h")).read()
    assert "size_t cfp_tsdf_surface_ws_bytes(int B, int Dx, int Dy, int Dz);" in text
    assert "int cfp_tsdf_surface(const float* volume /* [B][Dz][Dy][Dx][2] */, int Dx, int Dy, int Dz, int B, float ox, float oy, float oz," in text
    for cited in ("e = 3 * n + a", "n = (k * Dy + j) * Dx + i", "Wt(p) > 0 && Wt(q) > 0 && Wt(p) >= w_min && Wt(q) >= w_min",
                  "(F(p) < 0 && F(q) >= 0) || (F(p) >= 0 && F(q) < 0)", "fabsf(F(p) - F(q)) <= max_jump", "t = F(p) / (F(p) - F(q))",
                  "o_a + voxel * ((float)idx_a + t)", "1 / sqrtf((1 - t) * Wt(p) + t * Wt(q))", "g = (1 - t) * g(p) + t * g(q)",
                  "len = sqrtf((gx * gx + gy * gy) + gz * gz)", "(NaN, NaN, NaN)", "the true number kept, also when it exceeds cap",
                  "are not written", "the call only", "no atomics", "Nothing is zeroed"):
        assert cited in text, cited
    mk = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "Makefile")).read()
    assert " tsdf_surface.hip " in mk and "pointcloud.o tsdf_surface.o: chunk_scan.h" in mk
    src = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "tsdf_surface.hip")).read()
    assert "atomicAdd" not in src and "hipMemset" not in src and "float2" in src and '#include "chunk_scan.h"' in src


def test_refuses_bad_arguments_with_a_message(lib):
    """16 = a non-null, 16-byte aligned dummy device pointer: every case fails a check before anything is dereferenced or launched."""
    from cfpnet_amd import hip
    Q16 = 16

    def call(vol=Q16, dx=4, dy=4, dz=4, b=1, ox=0.0, oy=0.0, oz=0.0, voxel=0.05, w_min=0.0, max_jump=INF, cap=8, points=Q16, normals=Q16,
             std=Q16, index=Q16, counts=Q16, ws=Q16, ws_bytes=1 << 20):
        rc = lib.cfp_tsdf_surface(vol, dx, dy, dz, b, ox, oy, oz, voxel, w_min, max_jump, cap, points, normals, std, index, counts, ws,
                                  ws_bytes, 0)
        return rc, hip.last_error()

    for name in ("vol", "counts", "ws"):
        rc, msg = call(**{name: 0})
        assert rc == EINVAL and "cfp_tsdf_surface: null pointer" in msg, (name, rc, msg)
    rc, msg = call(index=0)
    assert rc == EINVAL and "points and index" in msg
    for kw in (dict(points=0, index=0, std=0), dict(points=0, index=0, normals=0)):
        rc, msg = call(**kw)
        assert rc == EINVAL and "normals and std need points" in msg, (kw, rc, msg)
    for kw in (dict(b=0), dict(b=-1), dict(dx=0), dict(dy=-1), dict(dz=0)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "non-positive" in msg, (kw, rc, msg)
    for kw in (dict(dx=1024, dy=1024, dz=683), dict(dx=895, dy=895, dz=894), dict(dx=1 << 16, dy=1 << 16, dz=1), dict(dx=(1 << 30), dy=1, dz=1),
               dict(b=65536)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "too large" in msg, (kw, rc, msg)
    for kw in (dict(ox=NAN), dict(oy=INF), dict(oz=-INF)):
        rc, msg = call(**kw)
        assert rc == EINVAL and "origin must be finite" in msg, (kw, rc, msg)
    for bad in (0.0, -1.0, NAN, INF):
        rc, msg = call(voxel=bad)
        assert rc == EINVAL and "voxel must be positive and finite" in msg, (bad, rc, msg)
    for bad in (-1.0, NAN, -INF):
        rc, msg = call(w_min=bad)
        assert rc == EINVAL and "w_min must not be negative" in msg, (bad, rc, msg)
        rc, msg = call(max_jump=bad)
        assert rc == EINVAL and "max_jump must not be negative" in msg, (bad, rc, msg)
    for bad in (0, -5):
        rc, msg = call(cap=bad)
        assert rc == EINVAL and "cap must be at least 1" in msg, (bad, rc, msg)
    rc, msg = call(vol=20)
    assert rc == EINVAL and "volume must be 8-byte aligned" in msg
    rc, msg = call(ws=20)
    assert rc == EINVAL and "workspace must be 8-byte aligned" in msg
    rc, msg = call(ws_bytes=0)
    assert rc == EINVAL and "workspace too small" in msg
    rc, msg = call(dx=67, dy=33, dz=31, b=2, ws_bytes=lib.cfp_tsdf_surface_ws_bytes(2, 67, 33, 31) - 1)
    assert rc == EINVAL and "workspace too small" in msg
    with pytest.raises(RuntimeError, match="cfp_tsdf_surface failed"):
        hip.call("cfp_tsdf_surface", Q16, 4, 4, 4, 1, 0.0, 0.0, 0.0, 0.0, 0.0, INF, 8, Q16, 0, Q16, Q16, Q16, Q16, 1 << 20, 0)


def test_ws_bytes(lib):
    """One int per chunk of 256 voxels and one per tile of 256 chunks, per image, rounded up to 8 bytes."""
    ws = lib.cfp_tsdf_surface_ws_bytes

    def want(B, voxels):
        chunks = -(-voxels // 256)
        return (B * (chunks + -(-chunks // 256)) + 1) // 2 * 8

    assert ws(1, 1, 1, 1) == 8 and ws(1, 256, 1, 1) == 8 and ws(1, 257, 1, 1) == 16 and ws(3, 257, 1, 1) == 40
    assert ws(2, 67, 33, 31) == 2 * (268 + 2) * 4 and ws(3, 31, 25, 29) == (3 * (88 + 1) + 1) // 2 * 8
    assert ws(1, 256, 256, 256) == (65536 + 256) * 4 and ws(1, 894, 894, 894) == want(1, 894 ** 3) and ws(7, 130, 5, 3) == want(7, 1950)
    for bad in ((0, 4, 4, 4), (-1, 4, 4, 4), (1, 0, 4, 4), (1, 4, -1, 4), (1, 4, 4, 0), (1, 895, 895, 894), (1, 1 << 16, 1 << 16, 1), (65536, 4, 4, 4)):
        assert ws(*bad) == 0, bad


def test_python_api_refuses_before_anything_runs():
    from cfpnet_amd import tsdf as TS
    import pointcloud_ref as P
    ps = inspect.signature(TS.TsdfVolume.surface_points).parameters
    assert list(ps) == ["self", "capacity", "w_min", "max_jump", "normals", "out"]
    assert (ps["capacity"].default, ps["w_min"].default, ps["max_jump"].default, ps["normals"].default, ps["out"].default) == (None, 0.0, None, True, None)
    assert list(inspect.signature(TS.TsdfVolume.surface_count).parameters) == ["self", "w_min", "max_jump"]
    assert list(inspect.signature(TS.TsdfVolume.write_ply).parameters) == ["self", "path_pattern", "options"]
    assert "tracker.volume.surface_points()" in TS.TsdfVolume.surface_points.__doc__
    v = TS.TsdfVolume((4, 5, 6), 0.05, (0, 0, 1), P.ZJUL5)
    for fn in (v.surface_points, v.surface_count, lambda: v.write_ply("x_{}.ply")):
        with pytest.raises(ValueError, match="nothing was integrated"):
            fn()
    sp = TS.SurfacePoints(None, None, None, None, None, 3)
    assert sp.capacity == 3 and sp.normals is None


# ---- the restatement against closed forms --------------------------------------------------------------------------------------------------

DIMS0, ORG0, VOX0, TR0 = (9, 7, 21), (-0.2, -0.15, 1.0), 0.05, 0.15


def _centres(dims, origin, voxel):
    Dx, Dy, Dz = dims
    o = [float(np.float32(v)) for v in origin]
    vx = float(np.float32(voxel))
    zz, yy, xx = np.meshgrid(o[2] + vx * np.arange(Dz), o[1] + vx * np.arange(Dy), o[0] + vx * np.arange(Dx), indexing="ij")
    return np.stack([xx, yy, zz], -1)


def test_a_plane_crosses_the_z_edges_only():
    """F = (Z - z) / trunc, Wt constant: one crossing per (i, j) column, on the z edge that holds Z, at z = Z exactly (F is linear), the
    normal (0, 0, -1) towards increasing F wherever the six neighbours exist, std = 1 / sqrt(Wt)."""
    Z, wt = 1.52, 625.0
    c = _centres(DIMS0, ORG0, VOX0)
    vol = np.stack([(Z - c[..., 2]) / TR0, np.full(c.shape[:3], wt)], -1)
    r = Q.surface(vol, ORG0, VOX0)
    Dx, Dy, Dz = DIMS0
    assert r["index"].size == Dx * Dy and (r["axis"] == 2).all() and (np.diff(r["index"]) > 0).all()
    k0 = int(np.floor((Z - float(np.float32(ORG0[2]))) / float(np.float32(VOX0))))
    n = r["index"] // 3
    assert (n // (Dx * Dy) == k0).all() and np.array_equal(n % (Dx * Dy), np.arange(Dx * Dy))
    assert np.abs(r["points"][:, 2] - Z).max() < 1e-12 and np.abs(r["points"][:, :2] - c[0, :, :, :2].reshape(-1, 2)).max() < 1e-12
    assert np.abs(r["std"] - 1 / np.sqrt(wt)).max() < 1e-12
    i, j = n % Dx, (n // Dx) % Dy
    inner = (i >= 1) & (i <= Dx - 2) & (j >= 1) & (j <= Dy - 2)
    assert np.array_equal(~np.isnan(r["normals"]).any(-1), inner) and np.abs(r["normals"][inner] - np.array([0.0, 0.0, -1.0])).max() < 1e-12
    # w_min above the weight keeps nothing; max_jump below voxel / trunc keeps nothing, at it everything
    assert Q.surface(vol, ORG0, VOX0, w_min=626.0)["index"].size == 0 and Q.surface(vol, ORG0, VOX0, w_min=625.0)["index"].size == Dx * Dy
    assert Q.surface(vol, ORG0, VOX0, max_jump=0.3)["index"].size == 0 and Q.surface(vol, ORG0, VOX0, max_jump=0.34)["index"].size == Dx * Dy
    # an unobserved layer under the surface: no crossing at all; -0.0 on the surface layer counts as non-negative
    hole = vol.copy()
    hole[k0 + 1, :, :, 1] = 0.0
    assert Q.surface(hole, ORG0, VOX0)["index"].size == 0
    zero = vol.copy()
    zero[k0, :, :, 0] = -0.0
    rz = Q.surface(zero, ORG0, VOX0)
    assert rz["index"].size == Dx * Dy and (rz["t"] == 0).all() and np.abs(rz["points"][:, 2] - c[k0, 0, 0, 2]).max() < 1e-12


def test_a_sphere_gives_points_on_it_and_radial_normals():
    """F = (|P - C| - r) / trunc, unclipped.  Along an edge of length h the distance is convex with a second derivative of at most
    1 / (r - h), so the linear interpolant is off by at most h^2 / (8 (r - h)) and so is the point's distance to the sphere (the distance
    has slope at most 1).  The central differences and the blend along the edge are second-order too: the angle to the radial direction
    stays below (h / (r - h))^2."""
    dims, org, h, r0 = (21, 19, 17), (-0.5, -0.45, 1.1), 0.05, 0.3
    C = np.array([0.02, -0.01, 1.52])
    c = _centres(dims, org, h)
    dist = np.linalg.norm(c - C, axis=-1)
    vol = np.stack([(dist - r0) / TR0, np.full(dist.shape, 100.0)], -1)
    r = Q.surface(vol, org, h)
    off = np.abs(np.linalg.norm(r["points"] - C, axis=-1) - r0)
    ok = ~np.isnan(r["normals"]).any(-1)
    radial = (r["points"] - C) / np.linalg.norm(r["points"] - C, axis=-1, keepdims=True)
    ang = Q.angle(r["normals"][ok], radial[ok])
    print(f"sphere: {r['index'].size} points, {np.bincount(r['axis']).tolist()} per axis, worst distance to the sphere {off.max():.3e} m "
          f"(bound {h * h / (8 * (r0 - h)):.3e}), worst angle to the radial direction {ang.max():.3e} rad (bound {(h / (r0 - h)) ** 2:.3e})")
    assert r["index"].size > 300 and (np.bincount(r["axis"]) > 80).all() and ok.all() and (np.diff(r["index"]) > 0).all()
    assert off.max() <= h * h / (8 * (r0 - h)) and ang.max() <= (h / (r0 - h)) ** 2
    assert np.abs(r["std"] - 0.1).max() < 1e-12


# ---- the inputs of the GPU tests -----------------------------------------------------------------------------------------------------------

def test_the_inputs_hold_every_required_shape():
    assert Q.STATE_CASES == ("direct_48x64", "blend_24x32", "no_std") and Q.RANDOM_B >= 2 and S.B == 3
    assert Q.RANDOM_DIMS == ((1, 1, 1), (2, 1, 1), (1, 1, 2), (64, 1, 1), (65, 3, 2), (130, 5, 3), (67, 33, 31))
    for name, lo, hi in (("direct_48x64", 1138, 1148), ("blend_24x32", 1491, 1556), ("no_std", 1501, 1580)):
        n = [Q.reference(name, b)["index"].size for b in range(S.B)]
        per_axis = sum(np.bincount(Q.reference(name, b)["axis"], minlength=3) for b in range(S.B))
        assert min(n) == lo and max(n) == hi and per_axis.argmin() == 1, (name, n, per_axis)      # the y axis has the fewest
    vol = Q.random_volume((67, 33, 31))
    F, Wt = vol[..., 0], vol[..., 1]
    assert abs((Wt == 0).mean() - 0.15) < 0.01 and Wt[Wt > 0].min() >= 0.5 and Wt.max() <= 900.0 and np.nanmin(F) >= -1 and np.nanmax(F) <= 1
    neg0 = (F == 0) & np.signbit(F)
    assert abs(np.isnan(F).mean() - 0.02) < 0.004 and abs(neg0.mean() - 0.02) < 0.004 and abs(((F == 0) & ~neg0).mean() - 0.02) < 0.004
    assert [Q.reference("random_1x1x1", b)["index"].tolist() for b in range(2)] == [[], []]
    assert [Q.reference("random_2x1x1", b)["index"].tolist() for b in range(2)] == [[0], [0]]
    assert [Q.reference("random_1x1x2", b)["index"].tolist() for b in range(2)] == [[2], [2]]
    assert Q.reference("random_2x1x1", 1)["t"][0] == 0 and np.signbit(Q.random_volume((2, 1, 1))[1, 0, 0, 0, 0])      # -0.0 crosses as non-negative
    for dims, nchunks in (((65, 3, 2), 2), ((130, 5, 3), 8), ((67, 33, 31), 268)):
        Dx, Dy, Dz = dims
        name = "random_%dx%dx%d" % dims
        assert -(-Dx * Dy * Dz // 256) == nchunks
        for b in range(Q.RANDOM_B):
            r = Q.reference(name, b)
            n, a = r["index"] // 3, r["index"] % 3
            assert ((a == 0) & (n % 64 == 63)).any(), (name, b)                       # an x edge whose far voxel belongs to the next wave
            assert (n // 256 == 0).any() and (n // 256 == nchunks - 1).any()          # the first and the last chunk
            assert all((a == c).sum() > 50 for c in range(3))
            # a row end inside a wave whose wrap-around pair (the next row's first voxel) would pass as a crossing: never an edge
            v = Q.random_volume(dims)[b].reshape(-1, 2)
            last = np.arange(Dx - 1, Dx * Dy * Dz - 1, Dx)
            last = last[last % 64 != 63]
            fp, fq, wp, wq = v[last, 0], v[last + 1, 0], v[last, 1], v[last + 1, 1]
            wrap = (wp > 0) & (wq > 0) & (((fp < 0) & (fq >= 0)) | ((fp >= 0) & (fq < 0)))
            assert wrap.any() and not np.isin(3 * last[wrap], r["index"]).any(), (name, b)
    assert 268 > 256                                                                  # more chunks than the scan workgroup has threads
    n = [Q.reference("random_67x33x31", b)["index"].size for b in range(2)]
    assert min(n) > 60000                                                             # about a third of all edges: every rank path is busy
    for name in ("random_130x5x3", "random_67x33x31"):                               # w_min binds and does not bind everywhere
        for b in range(2):
            assert 0 < Q.reference(name, b, Q.W_MIN_BINDS)["index"].size < 0.5 * Q.reference(name, b)["index"].size
    for name in Q.STATE_CASES:
        for b in range(S.B):
            assert 0.5 * Q.reference(name, b)["index"].size < Q.reference(name, b, 0.0, Q.JUMP)["index"].size < Q.reference(name, b)["index"].size


def test_float32_agrees_with_float64_on_every_input():
    worst = dict(angle=0.0, point=0.0, std=0.0)
    for name, (vol, _, _) in Q.inputs().items():
        for b in range(vol.shape[0]):
            a, d = Q.reference(name, b), Q.reference(name, b, dt=np.float64)
            assert np.array_equal(a["index"], d["index"]) and (np.diff(a["index"]) > 0).all(), (name, b)
            nan = np.isnan(a["normals"]).any(-1)
            assert np.array_equal(nan, np.isnan(d["normals"]).any(-1)) and np.array_equal(nan, np.isnan(a["normals"]).all(-1)), (name, b)
            assert a["points"].dtype == np.float32 and d["points"].dtype == np.float64
            if a["index"].size:
                worst["point"] = max(worst["point"], float(np.abs(a["points"] - d["points"]).max()))
                worst["std"] = max(worst["std"], float((np.abs(a["std"] - d["std"]) / d["std"]).max()))
            if (~nan).any():
                worst["angle"] = max(worst["angle"], float(Q.angle(a["normals"][~nan], d["normals"][~nan]).max()))
    print(f"float32 against float64 over every input: worst normal angle {worst['angle']:.3e} rad, point {worst['point']:.3e} m, "
          f"std {worst['std']:.3e} relative")
    assert 0 < worst["angle"] <= 2e-6 and 0 < worst["point"] <= 1e-6 and 0 < worst["std"] <= 1e-5


def test_the_extracted_points_meet_the_analytic_scene():
    """The table of DESIGN 4.31.  On direct_48x64 the median distance is below half a voxel, and with max_jump = 2 * voxel / trunc no
    point of images 0 and 1 is farther than that.  (blend_24x32 and no_std integrate a half-resolution prediction whose bilinear blend
    puts flying pixels at the sphere's rim: a third of their points lie off the surface, which max_jump removes most of -- printed, a
    property of the input.)"""
    half = S.VOXEL / 2
    for name in Q.STATE_CASES:
        for b in range(S.B):
            full, filt = Q.reference(name, b, dt=np.float64), Q.reference(name, b, 0.0, Q.JUMP, np.float64)
            da, df = Q.scene_distance(full["points"]), Q.scene_distance(filt["points"])
            print(f"{name} image {b}: {da.size} points, median {1e3 * np.median(da):.1f} mm, max {1e3 * da.max():.1f} mm, "
                  f"{100 * (da > half).mean():.1f} % beyond {1e3 * half:.0f} mm | max_jump {Q.JUMP:.3f}: {df.size} points, median "
                  f"{1e3 * np.median(df):.1f} mm, max {1e3 * df.max():.1f} mm, {100 * (df > half).mean():.1f} % beyond")
            if name == "direct_48x64":
                assert np.median(da) < half
                if b < 2:
                    assert df.max() <= half < da.max()
