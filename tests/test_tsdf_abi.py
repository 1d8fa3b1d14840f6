"""`cfp_tsdf_integrate` / `cfp_tsdf_raycast` without a GPU: the symbols, the header, every argument check (dummy pointers: no kernel is
launched), the Python API's own refusals, the numpy restatement of the definitions (`tsdf_ref.py`) against closed forms and against the
analytic scene, and the measurements the GPU tests' exact comparisons rest on: GUARD, the voxels and rays each case excludes (at most
1 %), the agreement of the float32 and the float64 restatement outside them, and the normals' angle."""
import inspect
import os

import numpy as np
import pytest

import pointcloud_ref as P
import tsdf_ref as S

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
    assert hasattr(lib, "cfp_tsdf_integrate") and hasattr(lib, "cfp_tsdf_raycast")
    text = open(os.path.join(ROOT, "include", "cfpnet_hip.h")).read()
    assert "int cfp_tsdf_integrate(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi," in text
    assert "int cfp_tsdf_raycast(const float* volume /* [B][Dz][Dy][Dx][2] */, int Dx, int Dy, int Dz, int B, float ox, float oy, float oz," in text
    for cited in ("Pc = R Pw + t", "Xw = ox + voxel * (float)i", "Xc = (T[0] * Xw + T[1] * Yw) + T[2] * Zw + T[3]", "u = fx * (Xc / Zc) + cx",
                  "(floorf(u + 0.5f), floorf(v + 0.5f))", "before any", "sdf = d - Zc", "f = fminf(1, sdf / trunc)", "w = 1 / (sf * sf)",
                  "F' = (F * Wt + f * w) / (Wt + w)", "Wt' = fminf(Wt + w, w_max)", "neither read nor written",
                  "{valid depth seen, updated, behind the surface}", "no floating-point atomics", "F = 1, Wt = 0",
                  "t_k = t_min + (float)k * step", "a product, not a running sum", "Xw = (T[0] * q.x + T[4] * q.y) + T[8] * q.z",
                  "all 8 corners have Wt > 0", "x first,", "depth = t_prev + step * (F_prev / (F_prev - F_cur))", "F_prev < 0 < F_cur",
                  "1 / sqrtf(trilinear Wt)", "n . P < 0", "(0, 0, -1)", "(NaN, NaN, NaN)", "the per-sample test still decides"):
        assert cited in text, cited
    assert len(hip.SIGNATURES["cfp_tsdf_integrate"][1]) == 29 and len(hip.SIGNATURES["cfp_tsdf_raycast"][1]) == 20
    mk = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "Makefile")).read()
    assert " tsdf.hip " in mk and "tsdf.o: metrics_pred.h" in mk
    src = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "tsdf.hip")).read()
    assert '#include "metrics_pred.h"' in src and "met_pred(" in src and "met_plane(" in src and "float2" in src
    assert src.count("atomicAdd(") == 1 and "atomicAdd(p.counts" in src              # one integer sum, no floating-point atomics


def test_integrate_refuses_bad_arguments_with_a_message(lib):
    """16 = a non-null, 16-byte aligned dummy device pointer: every case fails a check before anything is dereferenced or launched."""
    from cfpnet_amd import hip
    Q = 16

    def call(pred=Q, hp=8, wp=8, h=8, w=8, b=1, interp=0, lo=1e-3, hi=10.0, std=0, hu=8, wu=8, sstride=64, floor=1e-3, k=Q, t=Q, vol=Q,
             dx=4, dy=4, dz=4, ox=0.0, oy=0.0, oz=0.0, voxel=0.05, trunc=0.15, z_near=1e-3, w_max=1e6, counts=Q):
        rc = lib.cfp_tsdf_integrate(pred, hp, wp, h, w, b, interp, lo, hi, std, hu, wu, sstride, floor, k, t, vol, dx, dy, dz, ox, oy, oz,
                                    voxel, trunc, z_near, w_max, counts, 0)
        return rc, hip.last_error()

    for name in ("pred", "k", "t", "vol", "counts"):
        rc, msg = call(**{name: 0})
        assert rc == EINVAL and "cfp_tsdf_integrate: null pointer" in msg, (name, rc, msg)
    for kw in (dict(b=0), dict(h=0), dict(w=-1), dict(hp=0), dict(wp=-3), dict(dx=0), dict(dy=-1), dict(dz=0), dict(std=Q, hu=0),
               dict(std=Q, wu=-1)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "non-positive" in msg, (kw, rc, msg)
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
            assert rc == EINVAL and f"{word} must be positive and finite" in msg, (key, bad, rc, msg)
    rc, msg = call(std=Q, sstride=-1)
    assert rc == EINVAL and "stride" in msg
    for kw in (dict(ox=NAN), dict(oy=INF), dict(oz=-INF)):
        rc, msg = call(**kw)
        assert rc == EINVAL and "origin must be finite" in msg, (kw, rc, msg)
    rc, msg = call(vol=20)
    assert rc == EINVAL and "8-byte aligned" in msg
    with pytest.raises(RuntimeError, match="cfp_tsdf_integrate failed"):
        hip.call("cfp_tsdf_integrate", Q, 8, 8, 8, 8, 1, 0, 1e-3, 10.0, 0, 0, 0, 0, 1e-3, Q, Q, Q, 4, 4, 4, 0.0, 0.0, 0.0, 0.0, 0.15, 1e-3,
                 1e6, Q, 0)


def test_raycast_refuses_bad_arguments_with_a_message(lib):
    from cfpnet_amd import hip
    Q = 16

    def call(vol=Q, dx=4, dy=4, dz=4, b=1, ox=0.0, oy=0.0, oz=0.0, voxel=0.05, k=Q, t=Q, hd=8, wd=8, t_min=0.1, t_max=3.0, step=0.05,
             depth=Q, normal=0, std=0):
        rc = lib.cfp_tsdf_raycast(vol, dx, dy, dz, b, ox, oy, oz, voxel, k, t, hd, wd, t_min, t_max, step, depth, normal, std, 0)
        return rc, hip.last_error()

    for name in ("vol", "k", "t", "depth"):
        rc, msg = call(**{name: 0})
        assert rc == EINVAL and "cfp_tsdf_raycast: null pointer" in msg, (name, rc, msg)
    for kw in (dict(b=0), dict(dx=0), dict(dy=-1), dict(dz=0), dict(hd=0), dict(wd=-2)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "non-positive" in msg, (kw, rc, msg)
    for kw in (dict(dx=2048, dy=2048, dz=512), dict(dx=(1 << 24) + 1, dy=1, dz=1), dict(hd=70000, wd=70000), dict(hd=1, wd=(1 << 24) + 1),
               dict(b=70000), dict(t_min=0.0, t_max=1e6, step=1e-3)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "too large" in msg, (kw, rc, msg)
    for word, key in (("voxel", "voxel"), ("step", "step")):
        for bad in (0.0, -1.0, NAN, INF):
            rc, msg = call(**{key: bad})
            assert rc == EINVAL and f"{word} must be positive and finite" in msg, (key, bad, rc, msg)
    for t0, t1 in ((1.0, 1.0), (2.0, 1.0), (NAN, 1.0), (0.0, NAN), (0.0, INF), (-INF, 1.0)):
        rc, msg = call(t_min=t0, t_max=t1)
        assert rc == EINVAL and "t_min < t_max" in msg, (t0, t1, rc, msg)
    rc, msg = call(ox=NAN)
    assert rc == EINVAL and "origin must be finite" in msg
    rc, msg = call(vol=20)
    assert rc == EINVAL and "8-byte aligned" in msg
    with pytest.raises(RuntimeError, match="cfp_tsdf_raycast failed"):
        hip.call("cfp_tsdf_raycast", Q, 4, 4, 4, 1, 0.0, 0.0, 0.0, 0.05, Q, Q, 8, 8, 1.0, 0.5, 0.05, Q, 0, 0, 0)


def test_python_api_refuses_before_anything_runs():
    import torch
    from cfpnet_amd import tsdf as TS
    ps = inspect.signature(TS.TsdfVolume).parameters
    assert list(ps) == ["dims", "voxel", "origin", "intrinsics", "size", "trunc", "w_max", "lo", "hi", "std_floor", "z_near"]
    assert (ps["size"].default, ps["trunc"].default, ps["w_max"].default) == (None, None, None)
    assert (ps["lo"].default, ps["hi"].default, ps["std_floor"].default, ps["z_near"].default) == (1e-3, 10.0, 1e-3, 1e-3)
    assert list(inspect.signature(TS.TsdfVolume.integrate).parameters) == ["self", "pred", "unc", "pose"]
    assert list(inspect.signature(TS.TsdfVolume.raycast).parameters) == ["self", "pose", "intrinsics", "size", "t_range", "step", "normals", "out"]
    assert inspect.signature(TS.TsdfVolume.raycast).parameters["normals"].default is True
    assert TS.COUNT_NAMES == ("seen", "updated", "behind") and "point_cloud(depth, K, size=(Hd, Wd), lo=-inf, hi=inf)" in TS.TsdfVolume.raycast.__doc__
    v = TS.TsdfVolume((4, 5, 6), 0.05, (0, 0, 1), P.ZJUL5)
    assert v.trunc == pytest.approx(0.15) and v.w_max == S.F32_MAX and v.dims == (4, 5, 6) and v.volume is None
    assert TS.TsdfVolume((4, 5, 6), 0.05, (0, 0, 1), P.ZJUL5, w_max=INF).w_max == S.F32_MAX
    assert TS.TsdfVolume((4, 5, 6), 0.05, (0, 0, 1), P.ZJUL5, trunc=0.2, w_max=50).w_max == 50.0
    for kw, word in ((dict(dims=(4, 5)), "dims"), (dict(dims=(4, 0, 6)), "dims"), (dict(dims=(2048, 2048, 512)), "dims"), (dict(dims="ab"), "dims"),
                     (dict(voxel=0.0), "voxel"), (dict(voxel=NAN), "voxel"), (dict(origin=(0, 0)), "origin"), (dict(origin=(0, NAN, 0)), "origin"),
                     (dict(trunc=-1.0), "trunc"), (dict(trunc=INF), "trunc"), (dict(w_max=0.0), "w_max"), (dict(w_max=NAN), "w_max"),
                     (dict(lo=2.0, hi=1.0), "empty depth range"), (dict(std_floor=0.0), "std_floor"), (dict(z_near=-1.0), "z_near"),
                     (dict(intrinsics=(1.0, 0.0, 2.0, 3.0)), "intrinsics")):
        args = dict(dims=(4, 5, 6), voxel=0.05, origin=(0, 0, 1), intrinsics=P.ZJUL5)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            TS.TsdfVolume(**args)
    host = torch.ones(1, 4, 6)
    with pytest.raises(ValueError, match="float32 device tensor"):
        v.integrate(host)
    with pytest.raises(ValueError, match="float32 device tensor"):
        v.integrate(host, host)
    with pytest.raises(ValueError, match="nothing was integrated"):
        v.raycast()
    v.reset()                                                                         # nothing to empty yet: no error


# ---- the restatement against closed forms --------------------------------------------------------------------------------------------------

K0 = (30.0, 29.0, 15.5, 10.5)
DIMS0, ORG0, VOX0, TR0 = (9, 7, 21), (-0.2, -0.15, 1.0), 0.05, 0.15


def _zs():
    """The z of the voxel layers as the restatement sees them: the origin and the edge are the float32 numbers the library receives."""
    return float(np.float32(ORG0[2])) + float(np.float32(VOX0)) * np.arange(DIMS0[2])


def _plane_frame(Z, std, dt=np.float64, H=21, W=31):
    return np.full((H, W), Z, dt), (None if std is None else np.full((H, W), std, dt))


def test_one_observation_of_a_fronto_parallel_plane():
    """F = (Z - z) / trunc clipped at 1 in front, untouched more than trunc behind; Wt = 1 / std^2."""
    Z, std = 1.52, 0.04
    d, s = _plane_frame(Z, std)
    r = S.integrate(S.empty_volume(DIMS0, np.float64), d, s, K0, ID, DIMS0, ORG0, VOX0, TR0)
    z = _zs()
    assert r["seen"].all() and r["front"].all()
    want_upd = (Z - z) >= -float(np.float32(TR0))
    assert np.array_equal(r["updated"], np.broadcast_to(want_upd[:, None, None], r["updated"].shape)) and 3 < want_upd.sum() < 20
    assert np.array_equal(r["behind"], ~r["updated"]) and S.counts_of(r) == [r["seen"].size, int(r["updated"].sum()), int(r["behind"].sum())]
    F, Wt = r["vol"][..., 0], r["vol"][..., 1]
    want_F = np.minimum(1.0, (Z - z) / float(np.float32(TR0)))
    assert np.abs(F[want_upd] - want_F[want_upd, None, None]).max() < 1e-12 and (F[~want_upd] == 1).all() and (Wt[~want_upd] == 0).all()
    assert np.abs(Wt[want_upd] - 1 / std ** 2).max() < 1e-9 and (F[want_upd] < 1).any() and (F[want_upd] == 1).any() and (F < 0).any()


def test_two_observations_average_and_w_max_caps():
    d1, s1 = _plane_frame(1.50, 0.05)
    d2, s2 = _plane_frame(1.56, 0.05)
    a = S.integrate(S.empty_volume(DIMS0, np.float64), d1, s1, K0, ID, DIMS0, ORG0, VOX0, TR0)
    b = S.integrate(a["vol"], d2, s2, K0, ID, DIMS0, ORG0, VOX0, TR0)
    both = a["updated"] & b["updated"]
    z = np.broadcast_to(_zs()[:, None, None], both.shape)
    tr = float(np.float32(TR0))
    mean = 0.5 * (np.minimum(1, (1.50 - z) / tr) + np.minimum(1, (1.56 - z) / tr))
    assert both.sum() > 100 and np.abs(b["vol"][..., 0][both] - mean[both]).max() < 1e-12          # equal variances: the mean
    assert np.abs(b["vol"][..., 1][both] - 2 / 0.05 ** 2).max() < 1e-9                               # and twice the weight
    c = S.integrate(a["vol"], d2, s2, K0, ID, DIMS0, ORG0, VOX0, TR0, w_max=500.0)
    assert (c["vol"][..., 1][both] == 500.0).all() and np.array_equal(c["vol"][..., 0], b["vol"][..., 0])      # the cap binds the weight only
    n = S.integrate(S.empty_volume(DIMS0, np.float64), d1, None, K0, ID, DIMS0, ORG0, VOX0, TR0)   # no std: w = 1
    assert (n["vol"][..., 1][n["updated"]] == 1.0).all() and np.array_equal(n["updated"], a["updated"])
    nan_std = S.integrate(S.empty_volume(DIMS0, np.float64), d1, np.full_like(d1, np.nan), K0, ID, DIMS0, ORG0, VOX0, TR0)
    assert np.abs(nan_std["vol"][..., 1][a["updated"]] - 1 / float(np.float32(1e-3)) ** 2).max() < 1e-3     # a NaN std takes the floor
    inf_std = S.integrate(S.empty_volume(DIMS0, np.float64), d1, np.full_like(d1, np.inf), K0, ID, DIMS0, ORG0, VOX0, TR0)
    assert not inf_std["updated"].any() and inf_std["seen"].all() and not np.isnan(inf_std["vol"]).any()


def test_raycasting_a_plane_returns_its_depth_and_normal():
    Z = 1.52
    d, s = _plane_frame(Z, 0.04)
    vol = S.integrate(S.empty_volume(DIMS0, np.float64), d, s, K0, ID, DIMS0, ORG0, VOX0, TR0)["vol"]
    r = S.raycast(vol, K0, ID, 21, 31, ORG0, VOX0, 0.5, 2.5, 0.075)
    hit = r["hit"] >= 0
    assert 20 < hit.sum() < hit.size                                                  # the volume covers the middle of the view
    assert np.abs(r["depth"][hit] - Z).max() < 1e-9 and np.isnan(r["depth"][~hit]).all()
    assert np.abs(r["std"][hit] - 0.04).max() < 1e-9
    ok = ~np.isnan(r["normal"]).any(-1)
    assert ok.sum() > 10 and not (ok & ~hit).any() and np.abs(r["normal"][ok] - np.array([0.0, 0.0, -1.0])).max() < 1e-9
    # from behind: the ray meets F < 0 first and then F > 0 -- a back face, no hit
    back = (-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 3.2)                                   # a camera at z = 3.2 looking down -z
    rb = S.raycast(vol, K0, back, 21, 31, ORG0, VOX0, 0.5, 2.5, 0.075)
    assert (rb["hit"] == -1).all() and np.isfinite(rb["fmin"]).any()
    assert S.hit_step_of(r["depth"], 0.5, 0.075).tolist() == r["hit"].tolist()


# ---- the cases of the GPU tests ------------------------------------------------------------------------------------------------------------

def test_the_case_tables_hold_every_required_shape():
    assert S.DIMS == (31, 25, 29) and (S.VOXEL, S.TRUNC, S.B, S.GRID) == (0.05, 0.15, 3, (48, 64))
    c = S.TSDF_CASES
    assert (c["blend_24x32"]["h"], c["blend_24x32"]["w"]) == (24, 32) and (c["direct_48x64"]["h"], c["direct_48x64"]["w"]) == (48, 64)
    assert not c["no_std"]["std"] and c["w_max_binds"]["w_max"] is not None and len(S.POSES) == 3
    pred, std, T = S.frames("blend_24x32")[0]
    assert np.isnan(pred[2]).any() and np.isinf(pred[2]).any() and np.isnan(std[2]).any() and (std[1] == 0).any() and T.shape == (3, 12)
    assert S.frames("no_std")[0][1] is None
    sizes = {(r["Hd"], r["Wd"]) for r in S.RAYCAST_CASES.values()}
    assert sizes == {(37, 53), (24, 32)} and S.RAYCAST_CASES["blend_to_37x53"]["K"] != S.K_GRID
    for poses in S.POSES + (S.POSE_VIEW,):                                            # rotated about two axes, never the identity
        for T in poses:
            Rm = np.array(T).reshape(3, 4)[:, :3]
            assert abs(Rm[1, 2]) > 5e-3 and abs(Rm[0, 2]) > 5e-3 and np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-6
    wt = S.states("w_max_binds")[-1][..., 1]
    assert (wt == 900.0).sum() > 1000 and ((wt > 0) & (wt < 900.0)).sum() > 1000      # the cap binds, and not everywhere
    assert S.states("blend_24x32")[-1][..., 1].max() > 900.0


def test_guard_measured():
    g = S.guard_measured()
    print(f"GUARD_MEASURED = {g:.4e} px = 4 x the worst |u32 - u64|, |v32 - v64| over the voxels of the GPU tests")
    assert S.GUARD_MEASURED == g and 0.0 < g < 2e-3                                   # far below a pixel, or the exclusion means nothing


@pytest.mark.parametrize("name", list(S.TSDF_CASES))
def test_at_most_one_percent_of_a_step_is_excluded_and_the_rest_agrees(name):
    outside = unseen = 0
    for f in range(len(S.POSES)):
        for b in range(S.B):
            a, d, ex = S.step_reference(name, f, b), S.step_reference(name, f, b, np.float64), S.step_excluded(name, f, b)
            differ = (a["seen"] != d["seen"]) | (a["updated"] != d["updated"]) | (a["behind"] != d["behind"]) | (a["pix"] != d["pix"])
            fe = np.abs(a["vol"][..., 0].astype(np.float64) - d["vol"][..., 0])[d["updated"] & ~ex]
            print(f"{name} frame {f} image {b}: counts {S.counts_of(d)}, excluded {ex.mean():.4f}, float32 and float64 differ at "
                  f"{int(differ.sum())} voxels, {int((differ & ~ex).sum())} outside the excluded set, worst |F32 - F64| {fe.max() if fe.size else 0:.2e}")
            assert ex.mean() <= S.MAX_EXCLUDED
            assert not (differ & ~ex).any()                                           # what the GPU comparison relies on, for numpy's float32
            if name == "outside_the_view":
                assert S.counts_of(d) == [0, 0, 0] and a["vol"].tobytes() == S.states(name)[0][b].tobytes()
            else:
                n = S.counts_of(d)
                assert n[0] == n[1] + n[2] and n[1] > 5000 and n[2] > 1000
                outside += int((d["pix"] < 0).sum())
                unseen += int(((d["pix"] >= 0) & ~d["seen"]).sum())
    if name != "outside_the_view":
        assert outside > 100                                                          # voxels that project outside the image
        assert unseen > 10                                                            # and voxels that read the NaN / Inf patch


@pytest.mark.parametrize("name", list(S.RAYCAST_CASES))
def test_raycast_hits_agree_and_meet_the_analytic_scene(name):
    c = S.RAYCAST_CASES[name]
    for b in range(S.B):
        a, d, ex = S.raycast_reference(name, b), S.raycast_reference(name, b, np.float64), S.raycast_excluded(name, b)
        hits = d["hit"] >= 0
        differ = a["hit"] != d["hit"]
        truth = S.scene_depth(c["K"][b], c["T"][b], np.arange(c["Wd"], dtype=np.float64), np.arange(c["Hd"], dtype=np.float64))
        med = float(np.median(np.abs(d["depth"] - truth)[hits]))
        print(f"{name} image {b}: {int(hits.sum())} of {hits.size} rays hit, {int(ex.sum())} excluded, hit steps differ at {int(differ.sum())} "
              f"({int((differ & ~ex).sum())} outside), median |raycast - scene| = {med:.4f} m (voxel / 2 = {S.VOXEL / 2})")
        assert ex.mean() <= S.MAX_EXCLUDED and not (differ & ~ex).any()
        assert hits.mean() > 0.15 and (~hits).any() and med < S.VOXEL / 2
        assert np.array_equal(S.hit_step_of(a["depth"], c["t_range"][0], c["step"])[~ex], d["hit"][~ex])      # how the GPU test reads the step
        assert np.array_equal(np.isnan(a["std"]), np.isnan(d["std"])) and np.array_equal(np.isnan(a["normal"]), np.isnan(d["normal"]))
        keep = hits & ~ex
        assert (np.abs(a["depth"][keep] - d["depth"][keep]) <= S.RTOL * np.maximum(np.abs(d["depth"][keep]), 1e-3)).all()
        ok = ~np.isnan(d["normal"]).any(-1)
        assert ok.sum() > 0.5 * hits.sum() and (np.isnan(d["normal"]).any(-1) & hits).any()      # normals, and hits at the rim without one
        pts = P.points(d["depth"], c["K"][b])
        assert ((d["normal"][ok] * pts[ok]).sum(-1) < 0).all()                        # facing the camera, like cfp_depth_unproject's


def test_normal_angle_measured():
    ang = S.normal_angle_measured()
    print(f"NORMAL_ANGLE_MEASURED = {ang:.3e} rad between the float32 and the float64 restatement (record: {S.NORMAL_ANGLE_F32_VS_F64:.1e})")
    assert S.NORMAL_ANGLE_MEASURED == ang and 0.0 < ang <= 1.25 * S.NORMAL_ANGLE_F32_VS_F64 and ang > 0.5 * S.NORMAL_ANGLE_F32_VS_F64
