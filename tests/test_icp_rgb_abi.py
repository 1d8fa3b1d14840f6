"""`cfp_luma` and `cfp_icp_rgb_step` without a GPU: the symbols, the header, every argument check (dummy pointers: no kernel is launched),
the Python API's own refusals, the numpy restatement (`icp_rgb_ref.py`) against closed forms and a finite difference, and the
measurements the GPU tests rest on: the painted scene's shortest period, the pixels each case excludes (at most 1 %), the
float32-vs-float64 gap of the 60 sums and of one step's pose, the wall that geometry refuses and the image resolves, and the convergence
of the float64 restatement on the painted scene."""
import inspect
import os

import numpy as np
import pytest

import icp_ref as I
import icp_rgb_ref as C

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
    from cfpnet_amd import hip
    assert hasattr(lib, "cfp_luma") and hasattr(lib, "cfp_icp_rgb_step") and hasattr(lib, "cfp_icp_rgb_ws_bytes")
    text = open(os.path.join(ROOT, "include", "cfpnet_hip.h")).read()
    for cited in ("size_t cfp_icp_rgb_ws_bytes(int B, int H, int W, int stride);", "int cfp_luma(const float* rgb, int layout,",
                  "int cfp_icp_rgb_step(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,",
                  "Y = (0.299f * R + 0.587f * G) + 0.114f * B", "x0 = floorf(u), y0 = floorf(v)", "x0 + 1 <= Wm - 1", "top = I00 + ax * (I10 - I00)",
                  "Im = top + ay * (bot - top)", "gx = (I10 - I00) + ay * ((I11 - I01) - (I10 - I00))", "gy = bot - top", "|rI| <= photo_max",
                  "-((gfx * (X' / Z') + gfy * (Y' / Z')) / Z')", "JI = (P' x a, a)", "A = A_geo + A_photo", "GEOMETRIC count", "ONE row of 60 doubles",
                  "4 zeros", "photo_rms", "given together or not at all", "One image level"):
        assert cited in text, cited
    assert len(hip.SIGNATURES["cfp_icp_rgb_step"][1]) == 42 and len(hip.SIGNATURES["cfp_icp_rgb_ws_bytes"][1]) == 4
    assert hip.SIGNATURES["cfp_icp_rgb_step"][1][:36] == hip.SIGNATURES["cfp_icp_step"][1][:36]       # the arguments of cfp_icp_step, then its own
    assert len(hip.SIGNATURES["cfp_luma"][1]) == 9
    mk = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "Makefile")).read()
    assert " icp_rgb.hip " in mk and "icp.o icp_rgb.o: icp_core.h" in mk and "icp_rgb.o: metrics_pred.h" in mk
    for name in ("icp.hip", "icp_rgb.hip"):                                           # one definition of the pair and of the solve
        src = open(os.path.join(ROOT, "cfpnet_amd", "csrc", name)).read()
        assert '#include "icp_core.h"' in src and "icp_pair(" in src and "icp_update_pose(" in src and "bool icp_solve(" not in src
        assert "atomic" not in src.replace("no atomics", "").replace("No atomics", "")
    core = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "icp_core.h")).read()
    assert "bool icp_solve(" in core and "void icp_pair(" in core and "met_pred(" in core and "__shfl_xor" in core


def test_workspace_size(lib):
    assert lib.cfp_icp_rgb_ws_bytes(3, 48, 64, 1) == 3 * 12 * 60 * 8 == 2 * lib.cfp_icp_ws_bytes(3, 48, 64, 1)
    assert lib.cfp_icp_rgb_ws_bytes(3, 48, 64, 2) == 3 * 3 * 60 * 8 and lib.cfp_icp_rgb_ws_bytes(2, 480, 640, 1) == 2 * 128 * 60 * 8
    for bad in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, -1, 1), (1, 8, 8, 0)):
        assert lib.cfp_icp_rgb_ws_bytes(*bad) == 0


def test_step_refuses_bad_arguments_with_a_message(lib):
    """16 = a non-null, 16-byte aligned dummy device pointer: every case fails a check before anything is dereferenced or launched."""
    from cfpnet_amd import hip
    Q = 16

    def call(pred=Q, hp=8, wp=8, h=8, w=8, b=1, interp=0, lo=1e-3, hi=10.0, std=0, hu=8, wu=8, sstride=64, floor=1e-3, nsrc=0, cos_min=0.5,
             ks=Q, md=Q, mn=Q, ms=0, hm=8, wm=8, km=Q, stride=1, z_near=1e-3, dist_max=0.25, min_pairs=100, min_pivot=1e-6, t=Q, tref=0,
             tworld=0, index=0, sums=0, stats=Q, ws=Q, ws_bytes=1 << 20, sl=Q, ml=Q, weight=625.0, photo_max=0.25, residual=0):
        rc = lib.cfp_icp_rgb_step(pred, hp, wp, h, w, b, interp, lo, hi, std, hu, wu, sstride, floor, nsrc, cos_min, ks, md, mn, ms, hm, wm, km,
                                  stride, z_near, dist_max, min_pairs, min_pivot, t, tref, tworld, index, sums, stats, ws, ws_bytes, sl, ml,
                                  weight, photo_max, residual, 0)
        return rc, hip.last_error()

    # its own checks: every one has to fail here, since the call with the defaults would launch
    for kw in (dict(sl=0), dict(ml=0)):
        rc, msg = call(**kw)
        assert rc == EINVAL and "cfp_icp_rgb_step: src_luma and mdl_luma are given together" in msg, (kw, rc, msg)
    rc, msg = call(sl=0, ml=0)
    assert rc == EINVAL and "cfp_icp_step is the entry" in msg, (rc, msg)
    for bad in (0.0, -1.0, NAN, INF):
        rc, msg = call(weight=bad)
        assert rc == EINVAL and "photo_weight must be positive and finite" in msg, (bad, rc, msg)
    for bad in (0.0, -0.5, NAN):
        rc, msg = call(photo_max=bad)
        assert rc == EINVAL and "photo_max must be positive" in msg, (bad, rc, msg)
    # the checks of cfp_icp_step, under this entry's name
    for name in ("pred", "ks", "md", "mn", "km", "t", "stats", "ws"):
        rc, msg = call(**{name: 0})
        assert rc == EINVAL and "cfp_icp_rgb_step: null pointer" in msg, (name, rc, msg)
    for kw in (dict(b=0), dict(h=0), dict(w=-1), dict(hp=0), dict(wp=-3), dict(hm=0), dict(wm=-1), dict(std=Q, hu=0), dict(std=Q, wu=-1)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "cfp_icp_rgb_step: non-positive" in msg, (kw, rc, msg)
    for kw in (dict(hp=4, wp=4), dict(hp=8, wp=4), dict(h=16, w=16)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "sizes differ" in msg, (kw, rc, msg)
    for kw in (dict(h=70000, w=70000, interp=1), dict(hp=70000, wp=70000, interp=1), dict(b=70000), dict(h=1, w=(1 << 24) + 1, interp=1),
               dict(hm=70000, wm=70000), dict(hm=1, wm=(1 << 24) + 1), dict(std=Q, hu=70000, wu=70000)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "too large" in msg, (kw, rc, msg)
    for lo, hi in ((2.0, 1.0), (1.0, 1.0), (NAN, 1.0), (0.0, NAN)):
        rc, msg = call(lo=lo, hi=hi)
        assert rc == EINVAL and "empty depth range" in msg, (lo, hi, rc, msg)
    for bad in (0, -2):
        rc, msg = call(stride=bad)
        assert rc == EINVAL and "stride must be at least 1" in msg, (bad, rc, msg)
    for word, key in (("z_near", "z_near"), ("dist_max", "dist_max"), ("std_floor", "floor")):
        for bad in (0.0, -1.0, NAN, INF):
            rc, msg = call(**{key: bad})
            assert rc == EINVAL and f"{word} must be positive and finite" in msg, (key, bad, rc, msg)
    for bad in (-1e-3, 1.0, 2.0, NAN):
        rc, msg = call(min_pivot=bad)
        assert rc == EINVAL and "min_pivot must lie in [0, 1)" in msg, (bad, rc, msg)
    for bad in (5, 0, -1):
        rc, msg = call(min_pairs=bad)
        assert rc == EINVAL and "min_pairs must be at least 6" in msg, (bad, rc, msg)
    for bad in (-1.5, 1.01, NAN):
        rc, msg = call(cos_min=bad)
        assert rc == EINVAL and "cos_min must lie in [-1, 1]" in msg, (bad, rc, msg)
    for kw in (dict(tref=Q), dict(tworld=Q)):
        rc, msg = call(**kw)
        assert rc == EINVAL and "T_ref and T_world are given together" in msg, (kw, rc, msg)
    rc, msg = call(std=Q, sstride=-1)
    assert rc == EINVAL and "stride" in msg
    rc, msg = call(ws_bytes=lib.cfp_icp_rgb_ws_bytes(1, 8, 8, 1) - 1)                 # what cfp_icp_step asks for is half of it: too small
    assert rc == EINVAL and "workspace too small" in msg
    rc, msg = call(ws_bytes=lib.cfp_icp_ws_bytes(1, 8, 8, 1))
    assert rc == EINVAL and "workspace too small" in msg
    rc, msg = call(ws=20)
    assert rc == EINVAL and "8-byte aligned" in msg
    rc, msg = call(sums=20)
    assert rc == EINVAL and "8-byte aligned" in msg


def test_luma_refuses_bad_arguments_with_a_message(lib):
    import ctypes
    from cfpnet_amd import hip
    Q = 16
    three = lambda *v: (ctypes.c_float * 3)(*v)
    m, s = three(0.485, 0.456, 0.406), three(0.229, 0.224, 0.225)

    def call(rgb=Q, layout=0, mean=m, std=s, h=8, w=8, b=1, out=Q):
        return lib.cfp_luma(rgb, layout, mean, std, h, w, b, out, 0), hip.last_error()

    for kw in (dict(rgb=0), dict(out=0)):
        rc, msg = call(**kw)
        assert rc == EINVAL and "cfp_luma: null pointer" in msg, (kw, rc, msg)
    for bad in (-1, 2):
        rc, msg = call(layout=bad)
        assert rc == EINVAL and "layout must be 0" in msg, (bad, rc, msg)
    for kw in (dict(mean=None), dict(std=None)):
        rc, msg = call(**kw)
        assert rc == EINVAL and "needs mean and std" in msg, (kw, rc, msg)
    for kw in (dict(h=0), dict(w=-1), dict(b=0)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "non-positive" in msg, (kw, rc, msg)
    for kw in (dict(h=70000, w=70000), dict(b=70000)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "too large" in msg, (kw, rc, msg)
    for kw in (dict(mean=three(0.5, NAN, 0.5)), dict(std=three(INF, 1.0, 1.0))):
        rc, msg = call(**kw)
        assert rc == EINVAL and "must be finite" in msg, (kw, rc, msg)


def test_python_api_refuses_before_anything_runs():
    import torch
    from cfpnet_amd import tracking as TR, tsdf as TS
    import pointcloud_ref as P
    base, ps = inspect.signature(TR.icp).parameters, inspect.signature(TR.icp_rgb).parameters
    extra = ["rgb", "model_rgb", "photo_std", "photo_max", "mean", "std", "residual"]
    assert list(ps) == list(base) + extra and all(ps[k].default == base[k].default for k in base)
    assert [ps[k].default for k in ("rgb", "model_rgb", "photo_std", "photo_max", "residual")] == [None, None, 0.04, 0.25, False]
    assert TR.IcpResult._fields[:7] == ("pose", "world", "stats", "sums", "index", "ws", "residual")
    assert TR.IcpResult._field_defaults == dict(residual=None, src_luma=None, mdl_luma=None)
    assert TR.STAT_NAMES_RGB == TR.STAT_NAMES + ("photo_pairs", "photo_rms")
    assert "NOT measured" in TR.icp_rgb.__doc__ and "10 / 255" in TR.icp_rgb.__doc__
    assert "ONE image level" in TR.__doc__ and "image pyramid is a later step" in TR.__doc__
    host = torch.ones(1, 4, 6)
    for kw in (dict(rgb=host), dict(model_rgb=host)):
        with pytest.raises(ValueError, match="given together or not at all"):
            TR.icp_rgb(host, P.ZJUL5, host, host, **kw)
    with pytest.raises(ValueError, match="float32 device tensor"):                    # neither: `icp` itself
        TR.icp_rgb(host, P.ZJUL5, host, host)
    with pytest.raises(ValueError, match="residual needs"):
        TR.icp_rgb(host, P.ZJUL5, host, host, residual=True)
    for kw, word in ((dict(photo_std=0.0), "photo_std"), (dict(photo_std=INF), "photo_std"), (dict(photo_std=NAN), "photo_std"),
                     (dict(photo_std=1e-30), "photo_std"), (dict(photo_max=0.0), "photo_max"), (dict(photo_max=NAN), "photo_max")):
        with pytest.raises(ValueError, match=word):
            TR.icp_rgb(host, P.ZJUL5, host, host, rgb=host, model_rgb=host, **kw)
    v = TS.TsdfVolume((4, 5, 6), 0.05, (0, 0, 1), P.ZJUL5)
    t = TR.Tracker(v)
    assert t.photo_std is None and t.photo_max == 0.25 and "photo_std" not in t.options
    t = TR.Tracker(v, photo_std=0.04, photo_max=INF, stride=2)
    assert t.photo_std == 0.04 and t.photo_max == INF and t.options["stride"] == 2 and set(t.options) == set(TR._TRACKER_OPTIONS)
    for kw, word in ((dict(photo_std=0.0), "photo_std"), (dict(photo_std=INF), "photo_std"), (dict(photo_max=-1.0), "photo_max"),
                     (dict(photo_weight=1.0), "unknown icp option")):
        with pytest.raises(ValueError, match=word):
            TR.Tracker(v, **kw)
    assert "photo_std" in TR.Tracker.__doc__ and "photo_std" in TR.Tracker.update_rgb.__doc__


# ---- the restatement against closed forms --------------------------------------------------------------------------------------------------

def test_luma_of_the_restatement():
    grey = np.full((1, 2, 3, 3), 0.5, np.float32)
    assert np.abs(C.luma(grey, 1) - 0.5).max() < 1e-7                                 # the three weights add up to 1
    rgb = np.zeros((1, 1, 1, 3), np.float32)
    for k, wt in enumerate((0.299, 0.587, 0.114)):
        rgb[:] = 0
        rgb[..., k] = 1
        assert C.luma(rgb, 1)[0, 0, 0] == np.float32(wt)
    planar = C.to_rgb(np.full((1, 2, 2), 0.6))                                        # [1,3,2,2] normalised
    want = 0.6 * (0.299 * C.TINT[0] + 0.587 * C.TINT[1] + 0.114 * C.TINT[2])
    assert np.abs(C.luma(planar, 0) - want).max() < 2e-7 and abs(C.tint_luma(0.6) - want) < 1e-15
    bad = planar.copy()
    bad[0, 1, 0, 0], bad[0, 2, 1, 1] = np.nan, np.inf
    y = C.luma(bad, 0)
    assert np.isnan(y[0, 0, 0]) and np.isnan(y[0, 1, 1]) and np.isfinite(y[0, 0, 1]) and np.isfinite(y[0, 1, 0])


def test_the_interpolant_is_exact_on_a_bilinear_image_and_refuses_outside():
    ys, xs = np.mgrid[0:5, 0:7].astype(np.float64)
    ml = 0.1 + 0.02 * xs + 0.03 * ys + 0.004 * xs * ys
    u, v = np.array([0.0, 2.25, 5.999, 6.0, -0.01, 3.0, np.nan]), np.array([0.0, 1.5, 3.999, 1.0, 1.0, 4.0, 1.0])
    ok, Im, gx, gy, x0, y0 = C.bilinear(ml, u, v)
    assert ok.tolist() == [True, True, True, False, False, False, False]              # x0 + 1 <= Wm - 1: the last column and row are taps only
    f = lambda a, b: 0.1 + 0.02 * a + 0.03 * b + 0.004 * a * b
    assert np.abs(Im[:3] - f(u[:3], v[:3])).max() < 1e-15
    assert np.abs(gx[:3] - (0.02 + 0.004 * v[:3])).max() < 1e-15 and np.abs(gy[:3] - (0.03 + 0.004 * u[:3])).max() < 1e-15
    hole = ml.copy()
    hole[2, 3] = np.nan
    assert C.bilinear(hole, np.array([2.5, 3.5, 1.5]), np.array([1.5, 2.5, 1.5]))[0].tolist() == [False, False, True]


def test_the_painted_scene():
    """Amplitude at most 0.25 around 0.5, and no period below 8 pixels on any surface from any camera the tests use."""
    rng = np.random.default_rng(5)
    a = C.albedo(rng.uniform(-4, 4, (4000, 3)))
    assert sum(w[0] for w in C.WAVES) <= 0.25 and a.min() >= 0.25 and a.max() <= 0.75 and a.std() > 0.05
    assert sum(w[0] for w in C.WALL_WAVES) <= 0.25
    worst = np.inf
    for b in range(I.B):
        cams = [(I.K_GRID[b], I.T_REF, *I.GRID), (I.K_MODEL_37x53[b], I.T_REF, 37, 53)]
        cams += [(I.K_GRID[b], I.current_pose(I.motion(m, b)), *I.GRID) for m in range(3)]
        cams += [(I.K_GRID[b], I.track_pose(f, b), *I.GRID) for f in range(I.TRACK_FRAMES)]
        worst = min([worst] + [C.min_period(*c) for c in cams])
    wall = min(2 * np.pi / np.linalg.norm(k) * min(K[0], K[1]) / C.WALL_Z for _, k, _ in C.WALL_WAVES for K in I.K_GRID)
    print(f"shortest period on the painted scene {worst:.2f} px, on the wall {wall:.1f} px")
    assert worst >= 8.0 and wall >= 8.0


def test_the_photometric_jacobian_against_a_central_difference():
    """JI is the derivative of rI under exp(xi) o T for the six axes: 200 photometric pairs away from a cell border, float64, h = 1e-5."""
    name, b, h = "model_37x53", 1, 1e-5
    geo, (sl, ml) = C.case_maps(name, b, np.float64)
    Km = [float(v) for v in geo[7]]
    pr = C.case_pairs(name, b, np.float64)
    inner = lambda a: (a - np.floor(a) > 1e-3) & (a - np.floor(a) < 1 - 1e-3)
    ok = pr["photo"] & ~C.case_excluded(name, b) & inner(pr["u"]) & inner(pr["v"])
    pick = np.random.default_rng(11).choice(np.flatnonzero(ok.ravel()), 200, replace=False)
    Pp = np.stack([pr[k].ravel()[pick] for k in ("Xp", "Yp", "Zp")], -1)
    JI, Is = pr["JI"].reshape(-1, 6)[pick], sl.ravel()[pick]

    def residual(xi):
        Re, te = I.exp_se3(xi)
        Q = Pp @ Re.T + te
        good, Im, *_ = C.bilinear(ml, Km[0] * (Q[:, 0] / Q[:, 2]) + Km[2], Km[1] * (Q[:, 1] / Q[:, 2]) + Km[3])
        assert good.all()
        return Im - Is

    assert np.array_equal(residual(np.zeros(6)), pr["rI"].ravel()[pick])
    fd = np.stack([(residual(h * np.eye(6)[k]) - residual(-h * np.eye(6)[k])) / (2 * h) for k in range(6)], -1)
    rel = np.abs(fd - JI).max(1) / np.linalg.norm(JI, axis=1)
    print(f"worst |JI - finite difference| / |JI| over 200 pairs = {rel.max():.3e}")
    assert rel.max() <= 1e-5 and np.linalg.norm(JI, axis=1).min() > 0


# ---- the measurements the GPU tests rest on ------------------------------------------------------------------------------------------------

def test_the_cases_cover_every_path():
    c = [I.ICP_CASES[n] for n in C.CASES]
    assert {v["stride"] for v in c} >= {1, 2} and {v["normals"] for v in c} == {True, False} and {v["std"] for v in c} == {True, False}
    assert any((v["h"], v["w"]) == (24, 32) for v in c) and any((v["Hm"], v["Wm"]) == (37, 53) for v in c)
    sl, ml = C.lumas("stride1_plain")
    assert np.isnan(ml[0]).any() and np.isnan(sl[1]).any() and np.isinf(sl[1]).any() and sl.dtype == np.float32
    assert sl.shape == (I.B,) + I.GRID and C.lumas("model_37x53")[1].shape == (I.B, 37, 53)


@pytest.mark.parametrize("name", C.CASES)
def test_at_most_one_percent_of_a_case_is_excluded_and_the_rest_agrees(name):
    for b in range(I.B):
        a, d, ex = C.case_pairs(name, b), C.case_pairs(name, b, np.float64), C.case_excluded(name, b)
        differ = (a["photo"] != d["photo"]) | (a["index"] != d["index"])
        share = ex.sum() / d["on"].sum()
        n, g = int(d["photo"].sum()), int((d["index"] >= 0).sum())
        print(f"{name} image {b}: {n} photometric of {g} geometric pairs, excluded share {share:.5f}, float32 and float64 differ at "
              f"{int(differ.sum())} pixels, {int((differ & ~ex).sum())} outside the excluded set")
        assert share <= I.MAX_EXCLUDED and not (differ & ~ex).any()
        assert not (d["photo"] & (d["index"] < 0)).any() and 0.8 * g < n < g          # most pairs see the picture; its border, NaNs and the gate drop some
    sl, ml = C.lumas(name)
    assert not C.case_pairs(name, 1, np.float64)["photo"][~np.isfinite(sl[1])].any()


@pytest.mark.parametrize("name", C.CASES)
def test_the_float32_gap_of_sums_and_step(name):
    gg, gp, gt = C.step_gap(name)
    print(f"{name}: worst |sum32 - sum64| / (sum of |terms|): geometric {gg:.3e}, photometric {gp:.3e} (RTOL / 2 = {I.RTOL / 2:.1e}); worst "
          f"|T'32 - T'64| = {gt:.3e}")
    assert gg <= I.RTOL / 2 and gp <= I.RTOL / 2                                      # so the GPU test's bound is RTOL itself
    assert gt <= 5e-7                                                                 # so the GPU test's bound is the 1e-6 floor


def test_the_wall_is_refused_by_geometry_and_resolved_by_the_image():
    x = C.wall_inputs()
    for b in range(I.B):
        deg, tr = I.pose_error(I.ID12, x["T_true"][b])
        assert 1.5 < deg < 2.0 and 0.02 < tr < 0.04 and all(0.01 <= abs(v) <= 0.03 for v in C.WALL_SHIFTS[b])      # (1, 1, 1) degrees, 1 to 3 cm
    for b, (T, st, (deg, tr)) in enumerate(C.wall_reference(False)):
        assert not st[:, 5].any() and (st[:, 0] > 2500).all() and np.array_equal(T, I.ID12)
    for b, (T, st, (deg, tr)) in enumerate(C.wall_reference(True)):
        print(f"wall image {b}: {int(st[-1, 6])} photometric pairs, photo rms {st[0, 7]:.4f} -> {st[-1, 7]:.5f}, error {deg:.4f} deg / "
              f"{1e3 * tr:.3f} mm")
        assert st[:, 5].all() and deg < 0.05 and tr < 1e-3 and st[-1, 7] < 0.05 * st[0, 7]


def test_the_float64_restatement_converges_on_the_painted_scene():
    """The bound on the translation is a quarter of a pixel's footprint at the scene's depth (1 cm of 4 cm at 2.5 m and f = 60): one
    level of a bilinear picture with occlusion edges in it is not to be trusted further, and the GPU test inherits twice the figure."""
    for stride in (1, 2):
        for b, (T, st, (deg, tr)) in enumerate(C.converge_reference(stride)):
            print(f"stride {stride} image {b}: {int(st[-1, 0])} + {int(st[-1, 6])} pairs, error {deg:.4f} deg / {1e3 * tr:.3f} mm, photo rms "
                  f"{st[0, 7]:.4f} -> {st[-1, 7]:.5f}")
            assert deg <= 0.1 and tr <= 1e-2 and st[:, 5].all() and st[-1, 7] < st[0, 7] and st[-1, 2] < st[0, 2]
