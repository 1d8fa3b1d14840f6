"""numpy restatement of the definitions of `cfp_tsdf_integrate` and `cfp_tsdf_raycast` (include/cfpnet_hip.h) -- TEST INFRASTRUCTURE.

Written for two dtypes: float32 with the header's order of operations (numpy rounds every float32 operation once, like the library built
without fused multiply-adds) -- what the GPU's F, Wt, depth and std are compared with -- and float64, which decides the discrete results:
which voxels an integration updates, which pixel each of them reads, at which step a ray hits.  A discrete result can differ between
the float32 kernel and the float64 reference only next to a boundary: a voxel whose projection lies within `GUARD` pixels of a
half-integer (four times the worst distance between the float32 and the float64 projections over these very inputs, as in
reproject_ref.py), a voxel whose sdf lies within SDF_BAND relative of -trunc, a ray with a valid sample of |F| < F_BAND up to its hit.
Those are excluded from the exact comparisons -- at most MAX_EXCLUDED of a case, asserted on the CPU (test_tsdf_abi.py).  Every
integration step of a case starts from one common float32 state (the float32 restatement's), so nothing carries over between frames.

The scene is analytic: a slanted wall with a sphere in front of it, ray-cast in float64 from every pose.  Also the inputs the GPU tests
use, so that the CPU tests can examine the same tensors.

NORMAL_ANGLE_F32_VS_F64: the worst angle between the float32 and the float64 restatement's raycast normals over every raycast of
RAYCAST_CASES, measured by normal_angle_measured() (test_tsdf_abi.py prints and bounds it): 2.8e-6 rad.  The GPU tests allow twice the
figure measured in the same session, not this record."""
import functools

import numpy as np

import pointcloud_ref as P
import reproject_ref as R

RTOL = P.RTOL            # 2e-5, tests/test_metrics.py
F_ATOL = 2e-5            # F is a normalised quantity in [-1, 1] with cancellation around 0: the relative bound times its scale of 1
LO, HI = P.LO, P.HI
Z_NEAR, STD_FLOOR = 1e-3, 1e-3
SDF_BAND = 1e-4          # a voxel whose sdf is within this relative distance of -trunc: whether it updates is not compared
F_BAND = 1e-5            # a ray with a valid sample of |F| below this up to its hit: its hit step is not compared
MAX_EXCLUDED = R.MAX_EXCLUDED
F32_MAX = float(np.finfo(np.float32).max)
GUARD_MEASURED = None    # pixels; set by guard_measured()
NORMAL_ANGLE_F32_VS_F64 = 2.8e-6      # radians; the record of normal_angle_measured()
NORMAL_ANGLE_MEASURED = None

DIMS = (31, 25, 29)      # Dx, Dy, Dz: odd and pairwise different
VOXEL, TRUNC = 0.05, 0.15
ORIGIN = (-0.7437, -0.6113, 1.0219)


# ---- the scene ---------------------------------------------------------------------------------------------------------------------------

WALL_N = np.array([0.2, -0.1, 1.0]) / np.linalg.norm([0.2, -0.1, 1.0])
WALL_C = float(WALL_N @ np.array([0.0, 0.0, 2.0]))    # n . Pw = c
SPHERE_C, SPHERE_R = np.array([0.1, -0.05, 1.55]), 0.3


def scene_depth(K, T, xs, ys):
    """Camera depth (float64) of the scene along the rays through the grid coordinates xs [W], ys [H] of the camera K at pose T
    (camera-from-world [R|t]); the nearer of the wall and the sphere."""
    fx, fy, cx, cy = (float(np.float32(v)) for v in K)
    M = np.asarray(T, np.float64).reshape(3, 4)
    Rm, t = M[:, :3], M[:, 3]
    rays = np.stack(np.broadcast_arrays(((xs - cx) / fx)[None, :], ((ys - cy) / fy)[:, None], 1.0), -1)      # camera frame, z = 1
    dw = rays @ Rm                                    # R^T r per pixel
    c0 = -Rm.T @ t                                    # the camera centre in the world
    wall = (WALL_C - WALL_N @ c0) / (dw @ WALL_N)
    oc = c0 - SPHERE_C
    a, b, c = (dw * dw).sum(-1), 2.0 * (dw @ oc), oc @ oc - SPHERE_R ** 2
    disc = b * b - 4 * a * c
    with np.errstate(invalid="ignore"):
        sph = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
    sph = np.where(sph > 0, sph, np.inf)
    return np.minimum(np.where(wall > 0, wall, np.inf), sph)


# ---- integrate ---------------------------------------------------------------------------------------------------------------------------

def project_voxels(K, T, dims, origin, voxel, dt):
    """-> (Zc, u, v) [Dz,Dy,Dx] in dt, the header's order of operations."""
    Dx, Dy, Dz = dims
    fx, fy, cx, cy = (dt(np.float32(v)) for v in K)
    t = [dt(np.float32(v)) for v in np.asarray(T).ravel()[:12]]
    ox, oy, oz = (dt(np.float32(v)) for v in origin)
    vx = dt(np.float32(voxel))
    Xw = (ox + vx * np.arange(Dx).astype(dt))[None, None, :]
    Yw = (oy + vx * np.arange(Dy).astype(dt))[None, :, None]
    Zw = (oz + vx * np.arange(Dz).astype(dt))[:, None, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        Xc = (t[0] * Xw + t[1] * Yw) + t[2] * Zw + t[3]
        Yc = (t[4] * Xw + t[5] * Yw) + t[6] * Zw + t[7]
        Zc = (t[8] * Xw + t[9] * Yw) + t[10] * Zw + t[11]
        u = fx * (Xc / Zc) + cx
        v = fy * (Yc / Zc) + cy
    assert Zc.dtype == np.dtype(dt) and u.dtype == np.dtype(dt)
    return Zc, u, v


def integrate(vol, d, s, K, T, dims, origin, voxel, trunc, z_near=Z_NEAR, std_floor=STD_FLOOR, w_max=F32_MAX):
    """vol [Dz,Dy,Dx,2] and the depth d [H,W] (P.depth) and std s [H,W] (P.plane_to_grid; None: w = 1) on the grid, all in one dtype
    -> dict: vol (new), seen, updated, behind [Dz,Dy,Dx] bool, pix [Dz,Dy,Dx] int (row * W + column the voxel reads, -1: none),
    u, v, sdf."""
    dt = vol.dtype.type
    H, W = d.shape
    Zc, u, v = project_voxels(K, T, dims, origin, voxel, dt)
    tr, zn, sf0, wm = (dt(np.float32(x)) for x in (trunc, z_near, std_floor, w_max))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        front = np.isfinite(Zc) & (Zc >= zn)
        col, row = np.floor(u + dt(0.5)), np.floor(v + dt(0.5))
        inside = front & (col >= 0) & (col < W) & (row >= 0) & (row < H)            # on the float values; NaN fails
        pix = np.where(inside, row, 0).astype(np.int64) * W + np.where(inside, col, 0).astype(np.int64)
        dv = d.ravel()[pix]
        seen = inside & np.isfinite(dv) & (dv > 0)
        sdf = dv - Zc
        behind = seen & (sdf < -tr)
        f = np.minimum(dt(1), sdf / tr)
        if s is None:
            w = np.ones_like(Zc)
        else:
            sv = s.ravel()[pix]
            sf = np.where(sv > sf0, sv, sf0)
            w = dt(1) / (sf * sf)
        updated = seen & ~behind & (w > 0) & np.isfinite(w)
        F, Wt = vol[..., 0], vol[..., 1]
        tot = Wt + w
        Fn = (F * Wt + f * w) / tot
        Wn = np.minimum(tot, wm)
    out = vol.copy()
    out[..., 0] = np.where(updated, Fn, F)
    out[..., 1] = np.where(updated, Wn, Wt)
    assert out.dtype == vol.dtype
    return dict(vol=out, seen=seen, updated=updated, behind=behind, pix=np.where(inside, pix, -1), u=u, v=v, sdf=sdf, front=front)


def counts_of(r, keep=None):
    k = np.ones(r["seen"].shape, bool) if keep is None else keep
    return [int((r["seen"] & k).sum()), int((r["updated"] & k).sum()), int((r["behind"] & k).sum())]


def empty_volume(dims, dt=np.float32):
    Dx, Dy, Dz = dims
    vol = np.zeros((Dz, Dy, Dx, 2), dt)
    vol[..., 0] = 1
    return vol


# ---- raycast -----------------------------------------------------------------------------------------------------------------------------

def _sample(vol, gx, gy, gz):
    """Trilinear (ok, F, Wt) at the grid coordinates, x first, then y, then z."""
    dt = vol.dtype.type
    Dz, Dy, Dx = vol.shape[:3]
    with np.errstate(invalid="ignore"):
        x0, y0, z0 = np.floor(gx), np.floor(gy), np.floor(gz)
        ok = (x0 >= 0) & (x0 <= Dx - 2) & (y0 >= 0) & (y0 <= Dy - 2) & (z0 >= 0) & (z0 <= Dz - 2)
    i, j, k = (np.where(ok, a, 0).astype(np.int64) for a in (x0, y0, z0))
    with np.errstate(invalid="ignore"):
        a, b, c = gx - x0, gy - y0, gz - z0
        ha, hb, hc = dt(1) - a, dt(1) - b, dt(1) - c
        v = [[[vol[k + dk, j + dj, i + di] if (Dx > 1 and Dy > 1 and Dz > 1) else np.zeros(i.shape + (2,), dt) for di in (0, 1)]
              for dj in (0, 1)] for dk in (0, 1)]
        for dk in (0, 1):
            for dj in (0, 1):
                for di in (0, 1):
                    ok = ok & (v[dk][dj][di][..., 1] > 0)
        res = []
        for ch in (0, 1):
            e = [hb * (ha * v[dk][0][0][..., ch] + a * v[dk][0][1][..., ch]) + b * (ha * v[dk][1][0][..., ch] + a * v[dk][1][1][..., ch])
                 for dk in (0, 1)]
            res.append(hc * e[0] + c * e[1])
    return ok, res[0], res[1]


def _ray_point(rx, ry, t, tt, origin, vx):
    qx, qy, qz = rx * tt - t[3], ry * tt - t[7], tt - t[11]
    Xw = (t[0] * qx + t[4] * qy) + t[8] * qz
    Yw = (t[1] * qx + t[5] * qy) + t[9] * qz
    Zw = (t[2] * qx + t[6] * qy) + t[10] * qz
    return (Xw - origin[0]) / vx, (Yw - origin[1]) / vx, (Zw - origin[2]) / vx


def raycast(vol, K, T, Hd, Wd, origin, voxel, t_min, t_max, step):
    """vol [Dz,Dy,Dx,2] in its dtype -> dict: depth, std [Hd,Wd], normal [Hd,Wd,3] in that dtype (NaN: nothing), hit [Hd,Wd] int (the
    step index k of the sample that closed the hit pair, -1: none), fmin [Hd,Wd] float64 (the smallest |F| among the valid samples up
    to and including the hit pair, or the whole ray without a hit; inf without a valid sample)."""
    dt = vol.dtype.type
    fx, fy, cx, cy = (dt(np.float32(v)) for v in K)
    t = [dt(np.float32(v)) for v in np.asarray(T).ravel()[:12]]
    org = [dt(np.float32(v)) for v in origin]
    vx, t0, t1, st = (dt(np.float32(v)) for v in (voxel, t_min, t_max, step))
    kmax = int(np.floor(np.float32((np.float32(t_max) - np.float32(t_min)) / np.float32(step))))      # the host's float32 count, both dtypes
    rx = np.broadcast_to(((np.arange(Wd).astype(dt) - cx) / fx)[None, :], (Hd, Wd))
    ry = np.broadcast_to(((np.arange(Hd).astype(dt) - cy) / fy)[:, None], (Hd, Wd))
    depth = np.full((Hd, Wd), np.nan, dt)
    hit = np.full((Hd, Wd), -1, np.int64)
    fmin = np.full((Hd, Wd), np.inf)
    alive = np.ones((Hd, Wd), bool)
    prev = np.zeros((Hd, Wd), bool)
    F_prev = np.zeros((Hd, Wd), dt)
    for k in range(kmax + 1):
        tt = t0 + dt(k) * st
        ok, F, _ = _sample(vol, *_ray_point(rx, ry, t, tt, org, vx))
        ok &= alive
        fmin = np.where(ok, np.minimum(fmin, np.abs(F.astype(np.float64))), fmin)
        pair = ok & prev
        with np.errstate(invalid="ignore", divide="ignore"):
            front = pair & (F_prev > 0) & (F <= 0)
            back = pair & (F_prev < 0) & (F > 0)
            t_prev = t0 + dt(k - 1) * st
            depth = np.where(front, t_prev + st * (F_prev / (F_prev - F)), depth)
        hit[front] = k
        alive &= ~(front | back)
        prev = ok & alive
        F_prev = np.where(ok, F, F_prev)
        if not alive.any():
            break
    assert depth.dtype == vol.dtype
    g = _ray_point(rx, ry, t, depth, org, vx)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok, _, Wt = _sample(vol, *g)
        std = np.where(ok, dt(1) / np.sqrt(Wt), dt(np.nan))
        good = hit >= 0
        dif = []
        for a in range(3):
            lo_g = [g[b] - dt(1) if b == a else g[b] for b in range(3)]
            hi_g = [g[b] + dt(1) if b == a else g[b] for b in range(3)]
            ok0, f0, _ = _sample(vol, *lo_g)
            ok1, f1, _ = _sample(vol, *hi_g)
            good = good & ok0 & ok1
            dif.append(f1 - f0)
        ln = np.sqrt((dif[0] * dif[0] + dif[1] * dif[1]) + dif[2] * dif[2])
        good = good & (ln > 0) & np.isfinite(ln)
        wx, wy, wz = dif[0] / ln, dif[1] / ln, dif[2] / ln
        n = np.stack([(t[0] * wx + t[1] * wy) + t[2] * wz, (t[4] * wx + t[5] * wy) + t[6] * wz, (t[8] * wx + t[9] * wy) + t[10] * wz], -1)
    n = np.where(good[..., None], n, dt(np.nan)).astype(dt)
    return dict(depth=depth, std=std.astype(dt), normal=n, hit=hit, fmin=fmin, kmax=kmax)


def hit_step_of(depth, t_min, step):
    """The hit step the kernel's depth implies: depth lies in (t_{k-1}, t_k) -- strictly, outside the F_BAND exclusion -- so
    k = floor((depth - t_min) / step) + 1; -1 for NaN."""
    d = depth.astype(np.float64)
    with np.errstate(invalid="ignore"):
        k = np.floor((d - float(np.float32(t_min))) / float(np.float32(step))) + 1
    return np.where(np.isnan(d), -1, k).astype(np.int64)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------

K_GRID = ((40.0, 41.5, 31.3, 23.7), (38.5, 39.25, 32.1, 24.4), (42.0, 41.0, 30.6, 22.9))       # per image, for the 48 x 64 grid
K_HALF = ((20.0, 20.75, 15.4, 11.6), (19.25, 19.6, 15.8, 11.9), (21.0, 20.5, 15.1, 11.2))      # other intrinsics, for the 24 x 32 target
# three frames, each a pose per image: a few degrees about two axes, centimetres of translation (camera-from-world)
POSES = (
    (R._rot(0.03, -0.04, 0.0, (0.02, -0.01, 0.0)), R._rot(-0.02, 0.05, 0.0, (-0.03, 0.02, 0.01)), R._rot(0.04, 0.03, 0.0, (0.01, 0.03, -0.02))),
    (R._rot(-0.05, 0.02, 0.0, (-0.04, 0.03, 0.02)), R._rot(0.03, -0.03, 0.0, (0.05, -0.02, 0.0)), R._rot(-0.03, -0.05, 0.0, (-0.02, -0.04, 0.01))),
    (R._rot(0.02, 0.06, 0.0, (0.06, 0.01, -0.01)), R._rot(0.05, 0.01, 0.0, (0.0, 0.04, 0.02)), R._rot(-0.04, 0.04, 0.0, (0.03, -0.03, 0.0))),
)
POSE_VIEW = (R._rot(-0.03, 0.07, 0.0, (0.08, -0.05, 0.03)), R._rot(0.06, -0.02, 0.0, (-0.06, 0.04, -0.02)),
             R._rot(0.01, -0.06, 0.0, (0.04, 0.06, 0.01)))       # a fourth view, for the raycasts
GRID = (48, 64)

# name: prediction size (seen on the 48 x 64 grid), with a std plane of the same size or none, the weight cap, the volume's origin
TSDF_CASES = {
    "blend_24x32": dict(h=24, w=32, std=True, w_max=None, origin=ORIGIN),
    "direct_48x64": dict(h=48, w=64, std=True, w_max=None, origin=ORIGIN),
    "no_std": dict(h=24, w=32, std=False, w_max=None, origin=ORIGIN),
    "w_max_binds": dict(h=24, w=32, std=True, w_max=900.0, origin=ORIGIN),
    "outside_the_view": dict(h=24, w=32, std=True, w_max=None, origin=(-0.7437, -0.6113, -3.0219)),
}
B = 3
# name: the integrate case whose final state is cast, target size, intrinsics, pose, (t_min, t_max), step
RAYCAST_CASES = {
    "blend_to_37x53": dict(case="blend_24x32", Hd=37, Wd=53, K=R.K_SMALL, T=POSE_VIEW, t_range=(0.3, 3.0), step=0.075),
    "blend_to_24x32": dict(case="blend_24x32", Hd=24, Wd=32, K=K_HALF, T=POSES[1], t_range=(0.5, 2.9), step=0.075),
    "direct_to_37x53": dict(case="direct_48x64", Hd=37, Wd=53, K=R.K_SMALL, T=POSE_VIEW, t_range=(0.3, 3.0), step=0.06),
    "no_std_to_24x32": dict(case="no_std", Hd=24, Wd=32, K=K_HALF, T=POSE_VIEW, t_range=(0.5, 2.9), step=0.075),
}


def w_max_of(c):
    return F32_MAX if c["w_max"] is None else c["w_max"]


@functools.lru_cache(maxsize=None)
def frames(name):
    """Per frame (pred [B,h,w] f32, std [B,h,w] f32 or None, T [B,12] f32) -- read-only.  The prediction is the analytic scene at the
    grid positions the align-corners blend puts the prediction's pixels at, times a little noise; image 2 of frame 0 carries a NaN / Inf
    patch, its std a NaN patch and a few values below the floor."""
    c = TSDF_CASES[name]
    h, w = c["h"], c["w"]
    H, W = GRID
    xs, ys = np.arange(w) * ((W - 1) / max(w - 1, 1)), np.arange(h) * ((H - 1) / max(h - 1, 1))
    rng = np.random.default_rng(5000 + h + 7 * len(name))
    out = []
    for f, poses in enumerate(POSES):
        pred = np.stack([scene_depth(K_GRID[b], poses[b], xs, ys) for b in range(B)])
        pred = (pred * np.exp(rng.normal(0.0, 0.003, pred.shape))).astype(np.float32)
        std = (0.03 + 0.04 * rng.random((B, h, w))).astype(np.float32) if c["std"] else None
        if f == 0:
            pred[2, h // 3:h // 3 + h // 8, w // 2:w // 2 + w // 8] = np.nan                 # in the middle of the volume's footprint
            pred[2, 9:11, 20:23] = np.inf
            pred[2, 14:17, 8:10] = -np.inf
            if std is not None:
                std[2, 6:9, 12:16] = np.nan                                           # takes the floor
                std[1, 0, :3] = 0.0                                                   # below the floor
        T = np.array(poses, np.float32)
        for a in (pred, std, T):
            if a is not None:
                a.setflags(write=False)
        out.append((pred, std, T))
    return tuple(out)


def grids(name, f, b, dt):
    """(d, s) of image b of frame f on the grid, in dt."""
    c = TSDF_CASES[name]
    pred, std, _ = frames(name)[f]
    interp = int((c["h"], c["w"]) != GRID)
    d = P.depth(pred[b], GRID[0], GRID[1], interp, dt=dt)
    s = None if std is None else P.plane_to_grid(std[b], GRID[0], GRID[1], dt)
    return d, s


@functools.lru_cache(maxsize=None)
def states(name):
    """The float32 restatement's volumes [B,Dz,Dy,Dx,2] before frame 0, 1, 2 and after the last -- read-only; states(name)[f] is the
    common state every comparison of frame f starts from."""
    c = TSDF_CASES[name]
    vols = [np.stack([empty_volume(DIMS) for _ in range(B)])]
    for f in range(len(POSES)):
        cur = vols[-1]
        new = []
        for b in range(B):
            d, s = grids(name, f, b, np.float32)
            new.append(integrate(cur[b], d, s, K_GRID[b], frames(name)[f][2][b], DIMS, c["origin"], VOXEL, TRUNC, w_max=w_max_of(c))["vol"])
        vols.append(np.stack(new))
    for v in vols:
        v.setflags(write=False)
    return tuple(vols)


@functools.lru_cache(maxsize=None)
def step_reference(name, f, b, dt=np.float32):
    """The dict of `integrate` for image b of frame f in dt, started from the common float32 state -- read-only, shared."""
    c = TSDF_CASES[name]
    d, s = grids(name, f, b, dt)
    return integrate(states(name)[f][b].astype(dt), d, s, K_GRID[b], frames(name)[f][2][b], DIMS, c["origin"], VOXEL, TRUNC,
                     w_max=w_max_of(c))


def guard_measured():
    """GUARD: 4 x the worst |u32 - u64|, |v32 - v64| in pixels over every voxel of every case and frame that both restatements put in
    front of the camera and whose projection lies within a pixel of the grid."""
    global GUARD_MEASURED
    if GUARD_MEASURED is None:
        worst = 0.0
        H, W = GRID
        for name in TSDF_CASES:
            for f in range(len(POSES)):
                for b in range(B):
                    a, d = step_reference(name, f, b), step_reference(name, f, b, np.float64)
                    sel = a["front"] & d["front"] & (d["u"] > -2) & (d["u"] < W + 1) & (d["v"] > -2) & (d["v"] < H + 1)
                    if sel.any():
                        worst = max(worst, float(np.abs(a["u"][sel] - d["u"][sel]).max()), float(np.abs(a["v"][sel] - d["v"][sel]).max()))
        GUARD_MEASURED = 4.0 * worst
    return GUARD_MEASURED


@functools.lru_cache(maxsize=None)
def step_excluded(name, f, b):
    """[Dz,Dy,Dx] bool: the voxels of the step left out of the exact comparisons (float64 projections)."""
    r = step_reference(name, f, b, np.float64)
    g = guard_measured()
    tr = float(np.float32(TRUNC))
    with np.errstate(invalid="ignore"):
        near_u = np.abs(r["u"] + 0.5 - np.rint(r["u"] + 0.5)) < g
        near_v = np.abs(r["v"] + 0.5 - np.rint(r["v"] + 0.5)) < g
        band = r["seen"] & (np.abs(r["sdf"] + tr) <= SDF_BAND * tr)
    return (r["front"] & (near_u | near_v)) | band


@functools.lru_cache(maxsize=None)
def raycast_reference(name, b, dt=np.float32):
    """The dict of `raycast` for image b of the case in dt, on the float32 final state of its integrate case -- read-only."""
    c = RAYCAST_CASES[name]
    vol = states(c["case"])[-1][b].astype(dt)
    return raycast(vol, c["K"][b], c["T"][b], c["Hd"], c["Wd"], TSDF_CASES[c["case"]]["origin"], VOXEL, c["t_range"][0], c["t_range"][1],
                   c["step"])


def raycast_excluded(name, b):
    """[Hd,Wd] bool: rays with a valid sample of |F| < F_BAND up to the hit, in the float64 reference."""
    return raycast_reference(name, b, np.float64)["fmin"] < F_BAND


def normal_angle_measured():
    """The worst angle between the float32 and the float64 restatement's normals over every raycast case, where both have one."""
    global NORMAL_ANGLE_MEASURED
    if NORMAL_ANGLE_MEASURED is None:
        worst = 0.0
        for name in RAYCAST_CASES:
            for b in range(B):
                n32, n64 = raycast_reference(name, b)["normal"], raycast_reference(name, b, np.float64)["normal"]
                both = ~np.isnan(n32).any(-1) & ~np.isnan(n64).any(-1)
                if both.any():
                    worst = max(worst, float(P.angle(n32[both], n64[both]).max()))
        NORMAL_ANGLE_MEASURED = worst
    return NORMAL_ANGLE_MEASURED


# ---- comparisons -------------------------------------------------------------------------------------------------------------------------

close = R.close


def close_abs(got, want, atol, what="", keep=None):
    """|got - want| <= atol over `keep`; NaN at exactly the same places.  Returns the worst distance."""
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape, got.dtype)
    k = np.ones(got.shape, bool) if keep is None else keep
    g, w = got[k].astype(np.float64), want[k].astype(np.float64)
    assert np.array_equal(np.isnan(g), np.isnan(w)), what
    fin = ~np.isnan(w)
    worst = float(np.abs(g[fin] - w[fin]).max()) if fin.any() else 0.0
    print(f"{what}: worst |got - want| = {worst:.3e} (bound {atol:.1e}) over {int(fin.sum())} values")
    assert worst <= atol, (what, worst)
    return worst
