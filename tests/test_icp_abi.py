"""`cfp_icp_step` without a GPU: the symbols, the header, every argument check (dummy pointers: no kernel is launched), the Python API's own
refusals, the numpy restatement of the definition (`icp_ref.py`) against closed forms, and the measurements the GPU tests rest on:
GUARD, the source pixels each case excludes (at most 1 %), the float32-vs-float64 gap of the sums and of one step's pose, the scene's
eigenvalue ratio, the convergence of the float64 restatement from the three motions, and the CPU chain of the `Tracker` test."""
import inspect
import os

import numpy as np
import pytest

import icp_ref as I
import pointcloud_ref as P

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
    assert hasattr(lib, "cfp_icp_step") and hasattr(lib, "cfp_icp_ws_bytes")
    text = open(os.path.join(ROOT, "include", "cfpnet_hip.h")).read()
    assert "size_t cfp_icp_ws_bytes(int B, int H, int W, int stride);" in text
    assert "int cfp_icp_step(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi," in text
    for cited in ("Pm = R P + t", "the camera did not move", "x % stride == 0 && y % stride == 0", "d is finite and d > 0",
                  "X' = (T[0] * X + T[1] * Y) + T[2] * Z + T[3]", "Z' >= z_near", "u = fxm * (X' / Z') + cxm", "(floorf(u + 0.5f), floorf(v + 0.5f))",
                  "before any conversion to int", "> 0.25f", "Q = (((float)xm - cxm) / fxm * dm, ((float)ym - cym) / fym * dm, dm)",
                  "<= dist_max * dist_max", ">= cos_min", "r = (n.x * D.x + n.y * D.y) + n.z * D.z", "J = (P' x n, n)", "LEFT increment",
                  "w = 1 / (sf * sf + sm * sm)", "a NaN s gives the", "an infinite std", "w = 1.", "ym * Wm + xm", "fully written",
                  "upper triangle", "ONE row of 30 doubles", "at most 128", "2 zeros", "LDL^T", "min_pivot * (largest diagonal entry of A)",
                  "bit for bit as it was", "theta^2 < 1e-12", "(1, 1/2, 1/6)", "T' = exp(xi) o T", "Gram-Schmidt", "row 0 x row 1",
                  "R_cur = R^T R_ref, t_cur = R^T (t_ref - t)", "refused or not", "accepted (1 / 0)", "no atomics", "identical bits"):
        assert cited in text, cited
    assert len(hip.SIGNATURES["cfp_icp_step"][1]) == 37 and len(hip.SIGNATURES["cfp_icp_ws_bytes"][1]) == 4
    mk = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "Makefile")).read()
    assert " icp.hip " in mk and "icp.o: metrics_pred.h" in mk
    src = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "icp.hip")).read()
    assert '#include "metrics_pred.h"' in src and "met_pred(" in src and "met_plane(" in src and "__shfl_xor" in src
    assert "atomic" not in src.replace("no atomics", "").replace("No atomics", "")    # neither floating-point nor integer


def test_workspace_size(lib):
    assert lib.cfp_icp_ws_bytes(3, 48, 64, 1) == 3 * 12 * 30 * 8                      # 3072 pixels: 12 workgroups of 256
    assert lib.cfp_icp_ws_bytes(3, 48, 64, 2) == 3 * 3 * 30 * 8 and lib.cfp_icp_ws_bytes(1, 5, 7, 3) == 30 * 8
    assert lib.cfp_icp_ws_bytes(2, 480, 640, 1) == 2 * 128 * 30 * 8                   # capped
    for bad in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, -1, 1), (1, 8, 8, 0)):
        assert lib.cfp_icp_ws_bytes(*bad) == 0


def test_step_refuses_bad_arguments_with_a_message(lib):
    """16 = a non-null, 16-byte aligned dummy device pointer: every case fails a check before anything is dereferenced or launched."""
    from cfpnet_amd import hip
    Q = 16

    def call(pred=Q, hp=8, wp=8, h=8, w=8, b=1, interp=0, lo=1e-3, hi=10.0, std=0, hu=8, wu=8, sstride=64, floor=1e-3, nsrc=0, cos_min=0.5,
             ks=Q, md=Q, mn=Q, ms=0, hm=8, wm=8, km=Q, stride=1, z_near=1e-3, dist_max=0.25, min_pairs=100, min_pivot=1e-6, t=Q, tref=0,
             tworld=0, index=0, sums=0, stats=Q, ws=Q, ws_bytes=1 << 20):
        rc = lib.cfp_icp_step(pred, hp, wp, h, w, b, interp, lo, hi, std, hu, wu, sstride, floor, nsrc, cos_min, ks, md, mn, ms, hm, wm, km,
                              stride, z_near, dist_max, min_pairs, min_pivot, t, tref, tworld, index, sums, stats, ws, ws_bytes, 0)
        return rc, hip.last_error()

    for name in ("pred", "ks", "md", "mn", "km", "t", "stats", "ws"):
        rc, msg = call(**{name: 0})
        assert rc == EINVAL and "cfp_icp_step: null pointer" in msg, (name, rc, msg)
    for kw in (dict(b=0), dict(h=0), dict(w=-1), dict(hp=0), dict(wp=-3), dict(hm=0), dict(wm=-1), dict(std=Q, hu=0), dict(std=Q, wu=-1)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "non-positive" in msg, (kw, rc, msg)
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
        assert rc == EINVAL and "given together" in msg, (kw, rc, msg)
    rc, msg = call(std=Q, sstride=-1)
    assert rc == EINVAL and "stride" in msg
    rc, msg = call(ws_bytes=lib.cfp_icp_ws_bytes(1, 8, 8, 1) - 1)
    assert rc == EINVAL and "workspace too small" in msg
    rc, msg = call(ws=20)
    assert rc == EINVAL and "8-byte aligned" in msg
    rc, msg = call(sums=20)
    assert rc == EINVAL and "8-byte aligned" in msg
    with pytest.raises(RuntimeError, match="cfp_icp_step failed"):
        hip.call("cfp_icp_step", Q, 8, 8, 8, 8, 1, 0, 1e-3, 10.0, 0, 0, 0, 0, 1e-3, 0, 0.5, Q, Q, Q, 0, 8, 8, Q, 0, 1e-3, 0.25, 100, 1e-6, Q, 0,
                 0, 0, 0, Q, Q, 1 << 20, 0)


def test_python_api_refuses_before_anything_runs():
    import torch
    from cfpnet_amd import tracking as TR, tsdf as TS
    ps = inspect.signature(TR.icp).parameters
    assert list(ps) == ["pred", "intrinsics", "model_depth", "model_normals", "pose0", "unc", "model_std", "model_intrinsics", "size",
                        "src_normals", "cos_min", "iters", "stride", "dist_max", "z_near", "lo", "hi", "std_floor", "min_pairs", "min_pivot",
                        "ref_pose", "index", "out"]
    assert [ps[k].default for k in ("cos_min", "iters", "stride", "dist_max", "z_near", "lo", "hi", "std_floor", "min_pairs", "min_pivot",
                                    "index")] == [0.5, 10, 1, 0.25, 1e-3, 1e-3, 10.0, 1e-3, 100, 1e-6, False]
    assert TR.IcpResult._fields[:5] == ("pose", "world", "stats", "sums", "index") and "information matrix" in TR.IcpResult.__doc__
    assert TR.STAT_NAMES == ("pairs", "weight", "rms", "rotation", "translation", "accepted")
    assert list(inspect.signature(TR.Tracker.track).parameters) == ["self", "pred", "unc"]
    assert list(inspect.signature(TR.Tracker.update).parameters) == ["self", "pred", "unc", "integrate"]
    assert inspect.signature(TR.Tracker.update).parameters["integrate"].default is True
    assert "lost frame is still integrated" in TR.Tracker.__doc__ and "integrate=False" in TR.Tracker.__doc__
    assert "no relocalisation" in TR.__doc__ and "visual-inertial" in TR.__doc__
    host = torch.ones(1, 4, 6)
    with pytest.raises(ValueError, match="float32 device tensor"):
        TR.icp(host, P.ZJUL5, host, host)
    v = TS.TsdfVolume((4, 5, 6), 0.05, (0, 0, 1), P.ZJUL5)
    assert v.camera is None and v.grid_size is None                                   # read-only views of what the first integrate sets
    for name in ("camera", "grid_size"):
        with pytest.raises(AttributeError):
            setattr(v, name, 1)
    with pytest.raises(ValueError, match="TsdfVolume"):
        TR.Tracker(object())
    for kw, word in ((dict(iters=0), "iters"), (dict(iters=2.5), "iters"), (dict(stride=0), "stride"), (dict(dist_max=0.0), "dist_max"),
                     (dict(dist_max=INF), "dist_max"), (dict(min_pairs=5), "min_pairs"), (dict(min_pivot=1.0), "min_pivot"),
                     (dict(min_pivot=-0.1), "min_pivot"), (dict(cos_min=1.5), "cos_min"), (dict(lo=1.0), "unknown icp option"),
                     (dict(pose0=np.full((3, 4), NAN)), "finite"), (dict(pose0=np.eye(3)), "pose must be")):
        with pytest.raises(ValueError, match=word):
            TR.Tracker(v, **kw)
    t = TR.Tracker(v, stride=2, iters=4)
    assert t.options["stride"] == 2 and t.options["iters"] == 4 and t.options["dist_max"] == 0.25 and t.pose is None
    with pytest.raises(ValueError, match="float32 device tensor"):
        t.update(host)
    with pytest.raises(ValueError, match="nothing to track against"):
        t.track(host)
    for kw, word in ((dict(lo=2.0, hi=1.0), "empty depth range"), (dict(z_near=0.0), "z_near"), (dict(std_floor=NAN), "std_floor")):
        args = dict(cos_min=0.5, iters=10, stride=1, dist_max=0.25, z_near=1e-3, lo=1e-3, hi=10.0, std_floor=1e-3, min_pairs=100, min_pivot=1e-6)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            TR._icp_numbers(**args)


# ---- the restatement against closed forms --------------------------------------------------------------------------------------------------

def test_exp_of_zero_is_the_identity_and_of_a_rotation_is_rodrigues():
    Re, te = I.exp_se3(np.zeros(6))
    assert np.array_equal(Re, np.eye(3)) and np.array_equal(te, np.zeros(3))
    T, ok, xi = I.step(np.concatenate([np.eye(6)[np.triu_indices(6)] * 1000.0, np.zeros(6), [0.0, 1000.0, 1000.0]]), I.ID12)
    assert ok and np.array_equal(xi, np.zeros(6)) and np.array_equal(T, I.ID12)       # g = 0: the step is zero and T stays
    Re, te = I.exp_se3([0.0, 0.0, np.pi / 2, 1.0, 0.0, 0.0])                          # a quarter turn about z while moving along x
    assert np.abs(Re - np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])).max() < 1e-15
    assert np.abs(te - np.array([2 / np.pi, 2 / np.pi, 0.0])).max() < 1e-15           # the chord of the quarter circle of that arc
    small, _ = I.exp_se3([1e-7, 0.0, 0.0, 0.0, 0.0, 0.0])
    assert abs(small[2, 1] - 1e-7) < 1e-20 and np.abs(small @ small.T - np.eye(3)).max() < 1e-13


def test_a_translation_along_a_wall_normal_is_recovered_in_one_step_and_nothing_else_is():
    """A fronto-parallel wall at 2 m seen from 5 cm further back: r = +0.05 everywhere, J = (P' x n, n) with n = (0, 0, -1); the system is
    singular (a plane constrains three degrees of freedom): the step is refused.  With a second and third wall (the corner of a room)
    the translation is recovered in one step."""
    K, H, W = (60.0, 60.0, 31.5, 23.5), 48, 64
    md = np.full((H, W), 2.0)
    mn = np.broadcast_to(np.array([0.0, 0.0, -1.0]), (H, W, 3)).copy()
    d = np.full((H, W), 2.05)                                                         # the camera is 5 cm further from the wall
    pr = I.pairs(d, None, None, K, md, mn, None, K, I.ID12)
    s, _ = I.sums(pr)
    assert s[29] == H * W and np.abs(pr["r"] + 0.05).max() < 1e-12 and abs(s[27] - H * W * 0.0025) < 1e-9
    assert I.solve(s) is None and I.step(s, I.ID12)[1] is False                       # zero pivots
    A, g = I.unpack(s)
    assert abs(A[5, 5] - H * W) < 1e-9 and abs(g[5] - 0.05 * H * W) < 1e-9 and np.linalg.eigvalsh(A)[2] < 1e-9 * A[5, 5]
    assert abs(-g[5] / A[5, 5] + 0.05) < 1e-12                                        # the one equation the wall does give: t_z = -5 cm
    # a corner: three mutually orthogonal planes through the model camera's view, the current camera shifted by (0.02, -0.03, -0.05)
    shift = np.array([0.02, -0.03, -0.05])
    planes = ((np.array([0.0, 0.0, -1.0]), 2.0), (np.array([0.0, -1.0, 0.0]), 0.5), (np.array([1.0, 0.0, 0.0]), 0.6))      # n, distance

    def corner(c0):
        rx, ry = P._rays(K, H, W, np.float64)
        rays = np.stack(np.broadcast_arrays(rx[None, :], ry[:, None], 1.0), -1)
        ts = np.stack([(-dist - n @ c0) / (rays @ n) for n, dist in planes])       # the planes n . P = -dist, seen from c0
        ts = np.where(ts > 0, ts, np.inf)
        k = ts.argmin(0)
        return np.take_along_axis(ts, k[None], 0)[0], np.stack([p[0] for p in planes])[k]

    md, mn = corner(np.zeros(3))
    d, _ = corner(shift)                                                              # Pm = P + shift: the current camera sits at shift
    T = I.ID12
    for _ in range(2):
        T, ok, xi = I.step(I.sums(I.pairs(d, None, None, K, md, mn, None, K, T))[0], T)
        assert ok
    assert np.abs(I.mat(T)[1] - shift).max() < 2e-3 and np.abs(I.mat(T)[0] - np.eye(3)).max() < 2e-3


def test_t_world_against_a_matrix_inverse():
    rng = np.random.default_rng(3)
    for _ in range(5):
        T = I.rot(*rng.uniform(-0.3, 0.3, 3), tuple(rng.uniform(-0.5, 0.5, 3))).astype(np.float32)
        Tr = I.rot(*rng.uniform(-0.3, 0.3, 3), tuple(rng.uniform(-0.5, 0.5, 3))).astype(np.float32)
        M, Mr = np.eye(4), np.eye(4)
        M[:3], Mr[:3] = T.reshape(3, 4), Tr.reshape(3, 4)
        want = (np.linalg.inv(M) @ Mr)[:3].ravel()                                    # P_cur = T^-1 P_mdl = T^-1 T_ref P_w
        assert np.abs(I.world(T, Tr).astype(np.float64) - want).max() < 2e-6          # R^T for the inverse: R is orthonormal to float32
        assert np.abs(I.current_pose(T.astype(np.float64), Tr.astype(np.float64)) - want).max() < 2e-6
        back = I.relative(I.current_pose(T.astype(np.float64), Tr.astype(np.float64)), Tr.astype(np.float64))
        assert np.abs(back - T).max() < 2e-6


# ---- the measurements the GPU tests rest on ------------------------------------------------------------------------------------------------

def test_the_case_table_holds_every_required_shape():
    c = I.ICP_CASES
    assert {v["stride"] for v in c.values()} == {1, 2, 3} and {v["normals"] for v in c.values()} == {True, False}
    assert {v["std"] for v in c.values()} == {True, False} and (c["model_37x53"]["Hm"], c["model_37x53"]["Wm"]) == (37, 53)
    assert c["model_37x53"]["Km"] != I.K_GRID and (c["blend_24x32"]["h"], c["blend_24x32"]["w"]) == (24, 32) and I.B == 3 and I.GRID == (48, 64)
    x = I.inputs("stride1_normals_std")
    assert np.isnan(x["pred"][2]).any() and np.isinf(x["pred"][2]).any() and np.isnan(x["std"][2]).any() and np.isinf(x["std"][0]).any()
    assert np.isnan(x["md"][1]).any() and np.isnan(x["mn"][1]).any() and (x["mn"][0] == 0).all(-1).any() and np.isnan(x["ms"][1]).any()
    assert (x["nsrc"][2] == 0).all(-1).any() and x["T"].shape == (3, 12) and x["T"].dtype == np.float32
    assert I.inputs("stride1_plain")["std"] is None and I.inputs("stride1_plain")["nsrc"] is None
    assert I.K_GRID[0] == (60.0, 60.0, 31.5, 23.5)
    for m, (deg, cm) in enumerate(((2.2, 5.4), (4.1, 8.8), (6.4, 16.0))):
        ang, t = I.pose_error(I.motion(m), np.eye(4)[:3].ravel())
        assert abs(ang - deg) < 0.1 and abs(100 * t - cm) < 0.3, (m, ang, t)


def test_guard_measured():
    g = I.guard_measured()
    print(f"GUARD_MEASURED = {g:.4e} px = 4 x the worst |u32 - u64|, |v32 - v64| over the source pixels of the GPU tests")
    assert I.GUARD_MEASURED == g and 0.0 < g < 2e-3                                   # far below a pixel, or the exclusion means nothing


@pytest.mark.parametrize("name", list(I.ICP_CASES))
def test_at_most_one_percent_of_a_case_is_excluded_and_the_rest_agrees(name):
    kinds = set()
    for b in range(I.B):
        a, d, ex = I.case_pairs(name, b), I.case_pairs(name, b, np.float64), I.case_excluded(name, b)
        differ = a["index"] != d["index"]
        share = ex.sum() / d["on"].sum()
        n = int((d["index"] >= 0).sum())
        print(f"{name} image {b}: {n} pairs of {int(d['on'].sum())} stride-grid pixels, excluded share {share:.5f}, float32 and float64 "
              f"differ at {int(differ.sum())} pixels, {int((differ & ~ex).sum())} outside the excluded set")
        assert share <= I.MAX_EXCLUDED and not (differ & ~ex).any() and not (d["index"][~d["on"]] >= 0).any()
        assert 0.5 * d["on"].sum() < n < d["on"].sum()                                # most pixels pair, some gate or patch drops others
    x = I.inputs(name)
    d2 = I.case_pairs(name, 2, np.float64)
    assert (d2["index"][np.isnan(x["pred"][2]) if x["pred"].shape[1:] == I.GRID else np.zeros(I.GRID, bool)] == -1).all()
    d1 = I.case_pairs(name, 1, np.float64)["index"]
    assert not np.isin(d1[d1 >= 0], np.flatnonzero(np.isnan(x["md"][1]))).any()       # nothing pairs with the model's NaN block


@pytest.mark.parametrize("name", list(I.ICP_CASES))
def test_the_float32_gap_of_sums_and_step(name):
    gs, gt = I.step_gap(name)
    print(f"{name}: worst |sum32 - sum64| / (sum of |terms|) = {gs:.3e} (RTOL / 2 = {I.RTOL / 2:.1e}); worst |T'32 - T'64| = {gt:.3e}")
    assert gs <= I.RTOL / 2                                                           # so the GPU test's bound is RTOL itself
    assert gt <= 5e-7                                                                 # so the GPU test's bound is the 1e-6 floor


def test_the_scene_constrains_all_six_degrees_of_freedom():
    for b in range(I.B):
        x = I.converge_inputs(0)
        d = P.depth(x["pred"][b], *I.GRID, 0, dt=np.float64)
        s, _ = I.sums(I.pairs(d, None, None, x["K"][b], x["md"][b].astype(np.float64), x["mn"][b].astype(np.float64), None, x["K"][b],
                              x["T_true"][b].astype(np.float32)))
        ev = np.linalg.eigvalsh(I.unpack(s)[0])
        print(f"image {b}: {int(s[29])} pairs at the true pose, smallest / largest eigenvalue of A = {ev[0] / ev[-1]:.3e}")
        assert ev[0] / ev[-1] >= 1e-3 and I.solve(s) is not None
    which = I.scene(I.K_GRID[0], I.T_REF, *I.GRID)[2]
    assert all((which == k).sum() > 100 for k in (0, 1, 3))                           # back wall, floor and sphere in view


@pytest.mark.parametrize("m", range(3))
def test_the_float64_restatement_converges(m):
    for stride in (1, 2):
        for b, (T, st, (deg, tr)) in enumerate(I.converge_reference(m, stride, 12)):
            print(f"motion {m} stride {stride} image {b}: {int(st[-1, 0])} pairs, rms {st[0, 2]:.4f} -> {st[-1, 2]:.5f} m, error "
                  f"{deg:.4f} deg / {1e3 * tr:.3f} mm")
            assert deg <= 0.1 and tr <= 5e-3 and st[-1, 2] < st[0, 2] and st[:, 5].all()
            assert (450 if stride == 2 else 1800) <= st[-1, 0] <= (740 if stride == 2 else 2950)
    for b, (T, st, (deg, tr)) in enumerate(I.converge_reference(m, 1, 12, half=True)):
        print(f"motion {m} at 24 x 32, f = 30, image {b}: error {deg:.4f} deg / {1e3 * tr:.3f} mm")
        assert tr <= 5e-3


def test_the_tracker_chain_on_the_cpu():
    """What the GPU test of `Tracker` rests on: the model raycast of frame 0 shows all three planes and the sphere with normals, the
    float64 chain (tsdf_ref + icp_ref) stays near the truth, and twice its error plus the margins is tighter than half a voxel and
    0.5 degrees."""
    ref = I.track_reference()
    depth, normal, which = ref["first"]
    seen = [int((~np.isnan(normal).any(-1) & (which == k)).sum()) for k in range(4)]
    print("model normals of frame 0 on", dict(zip(I.SURFACES, seen)))
    assert all(n > 100 for n in seen)
    assert ref["poses"].shape == (I.TRACK_FRAMES, I.B, 12) and ref["poses"][0].tobytes() == I.track_frames()[0][2].tobytes()
    for f in range(1, I.TRACK_FRAMES):
        for b in range(I.B):
            deg, tr = ref["errors"][f, b]
            step_deg, step_tr = I.pose_error(I.track_pose(f, b), I.track_pose(f - 1, b))
            print(f"frame {f} image {b}: moved {step_deg:.2f} deg / {100 * step_tr:.1f} cm, CPU chain error {deg:.4f} deg / {1e3 * tr:.3f} mm")
            assert 1.0 < step_deg < 4.0 and 0.02 < step_tr < 0.08                      # a few degrees and centimetres per frame
            assert 2 * deg + 0.02 < 0.5 and 2 * tr + 2e-4 < 0.5 * I.TRACK_VOXEL
