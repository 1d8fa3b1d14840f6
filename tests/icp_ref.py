"""numpy restatement of the definition of `cfp_icp_step` (include/cfpnet_hip.h) -- TEST INFRASTRUCTURE.

Written for two dtypes: float32 with the header's order of operations (numpy rounds every float32 operation once, like the library built
without fused multiply-adds) -- what the GPU's sums are compared with -- and float64, which decides the discrete result: which model
pixel every source pixel is paired with.  The pairing can differ between the float32 kernel and the float64 reference only next to a
boundary: a projection within `GUARD` pixels of a half-integer (four times the worst distance between the float32 and the float64
projections over these very inputs, as in reproject_ref.py), a Z' within Z_BAND relative of z_near, a squared distance within DIST_BAND
relative of dist_max^2, a cosine within COS_BAND of cos_min.  Those source pixels are excluded from the exact comparison -- at most
MAX_EXCLUDED of the stride grid per case and image, asserted on the CPU (test_icp_abi.py).

The solve, exp, compose, Gram-Schmidt and the world pose are float64 like the kernel's finalize.  The scene is analytic and constrains
all six degrees of freedom: three planes and a sphere, ray-cast in float64 from any camera-from-world pose, with the analytic normals.
Also the inputs the GPU tests use, so that the CPU tests can examine the same tensors."""
import functools

import numpy as np

import pointcloud_ref as P
import reproject_ref as R

RTOL = P.RTOL            # 2e-5, tests/test_metrics.py
LO, HI = P.LO, P.HI
Z_NEAR, STD_FLOOR, DIST_MAX, COS_MIN = 1e-3, 1e-3, 0.25, 0.5
MIN_PAIRS, MIN_PIVOT = 100, 1e-6
Z_BAND, DIST_BAND, COS_BAND = 1e-4, 1e-4, 1e-5
MAX_EXCLUDED = R.MAX_EXCLUDED
GUARD_MEASURED = None    # pixels; set by guard_measured()
NT = 30                  # 21 of A (upper triangle by rows), 6 of g, sum w r r, sum w, pairs
ID12 = np.array(R.IDENTITY, np.float32)


# ---- the scene ---------------------------------------------------------------------------------------------------------------------------

PLANES = (                                            # n . (Pw - p) = 0
    (np.array([0.2, 0.0, -1.0]) / np.linalg.norm([0.2, 0.0, -1.0]), np.array([0.0, 0.0, 3.0])),      # back wall
    (np.array([0.0, -1.0, 0.0]), np.array([0.0, 1.0, 0.0])),                                         # floor
    (np.array([1.0, 0.0, 0.0]), np.array([-1.5, 0.0, 0.0])),                                         # side wall
)
SPHERE_C, SPHERE_R = np.array([0.3, 0.2, 2.0]), 0.4
SURFACES = ("back wall", "floor", "side wall", "sphere")


def mat(T):
    M = np.asarray(T, np.float64).reshape(3, 4)
    return M[:, :3], M[:, 3]


def scene(K, T, H, W, xs=None, ys=None):
    """The scene seen by the camera K at the camera-from-world pose T, float64: (depth [H,W], normals [H,W,3] in the camera frame, facing
    the camera, surface [H,W] int index into SURFACES).  The nearest hit along r = ((x - cx) / fx, (y - cy) / fy, 1): the parameter is the
    depth.  xs, ys: other grid coordinates than 0 .. W - 1, 0 .. H - 1."""
    fx, fy, cx, cy = (float(np.float32(v)) for v in K)
    Rm, t = mat(T)
    xs = np.arange(W, dtype=np.float64) if xs is None else xs
    ys = np.arange(H, dtype=np.float64) if ys is None else ys
    rays = np.stack(np.broadcast_arrays(((xs - cx) / fx)[None, :], ((ys - cy) / fy)[:, None], 1.0), -1)
    dw = rays @ Rm                                    # R^T r per pixel
    c0 = -Rm.T @ t                                    # the camera centre in the world
    ts, ns = [], []
    for n, p in PLANES:
        den = dw @ n
        with np.errstate(divide="ignore", invalid="ignore"):
            tt = (n @ (p - c0)) / den
        ts.append(np.where(tt > 0, tt, np.inf))
        ns.append(np.where((den > 0)[..., None], -n, n) * np.ones(dw.shape))
    oc = c0 - SPHERE_C
    a, b, c = (dw * dw).sum(-1), 2.0 * (dw @ oc), oc @ oc - SPHERE_R ** 2
    disc = b * b - 4 * a * c
    with np.errstate(invalid="ignore"):
        sph = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
    sph = np.where(sph > 0, sph, np.inf)
    ts.append(sph)
    ns.append(((c0 + np.where(np.isfinite(sph), sph, 0.0)[..., None] * dw) - SPHERE_C) / SPHERE_R)
    ts, ns = np.stack(ts), np.stack(ns)
    which = ts.argmin(0)
    depth = np.take_along_axis(ts, which[None], 0)[0]
    nw = np.take_along_axis(ns, which[None, ..., None], 0)[0]
    return depth, nw @ Rm.T, which


def rot(ax, ay, az, t):
    return np.array(R._rot(ax, ay, az, t), np.float64)


def relative(T_cur, T_ref):
    """[R|t] (float64, 12) that takes a point of the camera T_cur into the camera T_ref (both camera-from-world)."""
    Rc, tc = mat(T_cur)
    Rr, tr = mat(T_ref)
    Rm = Rr @ Rc.T
    return np.concatenate([Rm, (tr - Rm @ tc)[:, None]], 1).ravel()


def world(T, T_ref):
    """The header's T_world: R_cur = R^T R_ref, t_cur = R^T (t_ref - t), float64 from the float32 numbers -> float32 [12]."""
    Rm, t = mat(np.asarray(T, np.float32))
    Rr, tr = mat(np.asarray(T_ref, np.float32))
    return np.concatenate([Rm.T @ Rr, (Rm.T @ (tr - t))[:, None]], 1).ravel().astype(np.float32)


def pose_error(T, T_true):
    """(rotation error in degrees, translation error in metres) of T against T_true."""
    Ra, ta = mat(T)
    Rb, tb = mat(T_true)
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    s = np.linalg.norm(Ra.T @ Rb - Rb.T @ Ra) / (2.0 * np.sqrt(2.0))
    return float(np.degrees(np.arctan2(s, c))), float(np.linalg.norm(ta - tb))


# ---- pairs, terms, sums ------------------------------------------------------------------------------------------------------------------

def _normal_ok(n):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.isfinite(n).all(-1) & ((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2] > n.dtype.type(0.25))


def pairs(d, s, nsrc, K, md, mn, ms, Km, T, stride=1, z_near=Z_NEAR, dist_max=DIST_MAX, cos_min=COS_MIN, std_floor=STD_FLOOR, index=None):
    """d [H,W] (P.depth), s [H,W] or None (P.plane_to_grid), nsrc [H,W,3] or None on the source grid, md [Hm,Wm], mn [Hm,Wm,3], ms
    [Hm,Wm] or None the model map, all in ONE dtype; K, Km, T the float32 numbers -> dict in that dtype, everything [H,W]: index (int,
    -1: no pair), u, v, Zp, dd, cos (NaN without src normals), w, r, J [H,W,6].  With `index` the pairing is taken from it (the
    GPU's own) and no gate is applied."""
    dt = d.dtype.type
    H, W = d.shape
    Hm, Wm = md.shape
    fx, fy, cx, cy = (dt(np.float32(v)) for v in K)
    fxm, fym, cxm, cym = (dt(np.float32(v)) for v in Km)
    t = [dt(np.float32(v)) for v in np.asarray(T).ravel()[:12]]
    zn, sf0, cm = dt(np.float32(z_near)), dt(np.float32(std_floor)), dt(np.float32(cos_min))
    d2 = dt(np.float32(dist_max)) * dt(np.float32(dist_max))
    on = np.zeros((H, W), bool)
    on[::stride, ::stride] = True
    rx, ry = P._rays(K, H, W, dt)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ok = on & np.isfinite(d) & (d > 0)
        X, Y, Z = rx[None, :] * d, ry[:, None] * d, d
        Xp = (t[0] * X + t[1] * Y) + t[2] * Z + t[3]
        Yp = (t[4] * X + t[5] * Y) + t[6] * Z + t[7]
        Zp = (t[8] * X + t[9] * Y) + t[10] * Z + t[11]
        ok &= np.isfinite(Zp) & (Zp >= zn)
        u, v = fxm * (Xp / Zp) + cxm, fym * (Yp / Zp) + cym
        if index is None:
            col, row = np.floor(u + dt(0.5)), np.floor(v + dt(0.5))
            ok &= (col >= 0) & (col < Wm) & (row >= 0) & (row < Hm)
            col, row = np.where(ok, col, dt(0)), np.where(ok, row, dt(0))
            mi = row.astype(np.int64) * Wm + col.astype(np.int64)
        else:
            ok = index >= 0
            mi = np.where(ok, index, 0).astype(np.int64)
            col, row = (mi % Wm).astype(dt), (mi // Wm).astype(dt)
        dm, n = md.ravel()[mi], mn.reshape(-1, 3)[mi]
        nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
        Qx, Qy = (col - cxm) / fxm * dm, (row - cym) / fym * dm
        Dx, Dy, Dz = Xp - Qx, Yp - Qy, Zp - dm
        dd = (Dx * Dx + Dy * Dy) + Dz * Dz
        cos = np.full((H, W), np.nan, dt)
        if nsrc is not None:
            sx, sy, sz = nsrc[..., 0], nsrc[..., 1], nsrc[..., 2]
            qx, qy, qz = (t[0] * sx + t[1] * sy) + t[2] * sz, (t[4] * sx + t[5] * sy) + t[6] * sz, (t[8] * sx + t[9] * sy) + t[10] * sz
            cos = (qx * nx + qy * ny) + qz * nz
        w = np.ones((H, W), dt)
        if s is not None or ms is not None:
            sf = np.full((H, W), sf0, dt) if s is None else np.where(s > sf0, s, sf0)
            sm = np.zeros((H, W), dt) if ms is None else np.where(np.isfinite(ms.ravel()[mi]), ms.ravel()[mi], dt(0))
            w = dt(1) / (sf * sf + sm * sm)
        if index is None:
            ok &= np.isfinite(dm) & (dm > 0) & _normal_ok(n) & (dd <= d2)
            if nsrc is not None:
                ok &= _normal_ok(nsrc) & (cos >= cm)
            ok &= (w > 0) & np.isfinite(w)
        r = (nx * Dx + ny * Dy) + nz * Dz
        J = np.stack([Yp * nz - Zp * ny, Zp * nx - Xp * nz, Xp * ny - Yp * nx, nx, ny, nz], -1)
    assert r.dtype == d.dtype and J.dtype == d.dtype and w.dtype == d.dtype and u.dtype == d.dtype
    return dict(index=np.where(ok, mi, -1), on=on, u=u, v=v, Zp=Zp, dd=dd, cos=cos, w=w, r=r, J=J)


def sums(pr):
    """The 30 sums of the pairs of `pairs` -> (sums [30] float64, scale [30] float64 = the sums of the ABSOLUTE values of the terms).  The
    products are made in the dict's dtype in the header's order, the accumulation is float64."""
    ok = pr["index"] >= 0
    w, r, J = pr["w"][ok], pr["r"][ok], pr["J"][ok]
    terms = []
    for a in range(6):
        wj = w * J[:, a]
        terms += [wj * J[:, c] for c in range(a, 6)]
    terms += [(w * J[:, a]) * r for a in range(6)]
    terms += [(w * r) * r, w, np.ones_like(w)]
    assert len(terms) == NT and all(t.dtype == w.dtype for t in terms)
    t64 = np.stack(terms).astype(np.float64) if w.size else np.zeros((NT, 0))
    return t64.sum(1), np.abs(t64).sum(1)


# ---- the step ----------------------------------------------------------------------------------------------------------------------------

def unpack(s):
    A = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for c in range(a, 6):
            A[a, c] = A[c, a] = s[k]
            k += 1
    return A, np.asarray(s[21:27], np.float64)


def solve(s, min_pairs=MIN_PAIRS, min_pivot=MIN_PIVOT):
    """A xi = -g by LDL^T, float64 -> xi [6], or None when the step is refused: pairs < min_pairs or a pivot not above
    min_pivot * (largest diagonal entry of A)."""
    A, g = unpack(s)
    if s[29] < min_pairs:
        return None
    thresh = float(np.float32(min_pivot)) * A.diagonal().max()
    L, D = np.eye(6), np.zeros(6)
    for j in range(6):
        D[j] = A[j, j] - (L[j, :j] ** 2 * D[:j]).sum()
        if not (D[j] > thresh and D[j] > 0):
            return None
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j] * D[:j]).sum()) / D[j]
    z = np.linalg.solve(L, -g)
    xi = np.linalg.solve(L.T, z / D)
    return xi if np.isfinite(xi).all() else None


def exp_se3(xi):
    """exp of xi = (omega, v): (Re [3,3], te [3]), Rodrigues and V v, the first-order coefficients when theta^2 < 1e-12."""
    om, v = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th2 = float(om @ om)
    a, b, c = 1.0, 0.5, 1.0 / 6.0
    if not th2 < 1e-12:
        th = np.sqrt(th2)
        a, b, c = np.sin(th) / th, (1.0 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
    Kx = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    return np.eye(3) + a * Kx + b * Kx @ Kx, (np.eye(3) + b * Kx + c * Kx @ Kx) @ v


def step(s, T, min_pairs=MIN_PAIRS, min_pivot=MIN_PIVOT):
    """One finalize: sums [30] and the float32 pose T [12] -> (T' float32 [12], accepted, xi or None).  T' = exp(xi) o T, rows
    re-orthonormalised by Gram-Schmidt, rounded to float32; a refused step returns T itself."""
    T = np.asarray(T, np.float32)
    xi = solve(s, min_pairs, min_pivot)
    if xi is None:
        return T, False, None
    Re, te = exp_se3(xi)
    Rm, t = mat(T)
    M, tn = Re @ Rm, Re @ t + te
    r0 = M[0] / np.linalg.norm(M[0])
    r1 = M[1] - (r0 @ M[1]) * r0
    r1 /= np.linalg.norm(r1)
    Rn = np.stack([r0, r1, np.cross(r0, r1)])
    return np.concatenate([Rn, tn[:, None]], 1).ravel().astype(np.float32), True, xi


def stats_of(s, xi):
    """The row of `stats` for the sums and the step taken (None: refused), float64."""
    rms = np.sqrt(s[27] / s[28]) if s[29] > 0 else np.nan
    om, v = (0.0, 0.0) if xi is None else (np.linalg.norm(xi[:3]), np.linalg.norm(xi[3:]))
    return np.array([s[29], s[28], rms, om, v, 0.0 if xi is None else 1.0])


def run(d, s, nsrc, K, md, mn, ms, Km, T0=None, iters=10, min_pairs=MIN_PAIRS, min_pivot=MIN_PIVOT, **kw):
    """`iters` iterations from T0 (identity by default) in the dtype of the maps -> (T float32 [12], stats [iters,6], sums of the last)."""
    T = ID12.copy() if T0 is None else np.asarray(T0, np.float32)
    st = []
    for _ in range(iters):
        sm, _ = sums(pairs(d, s, nsrc, K, md, mn, ms, Km, T, **kw))
        T, _, xi = step(sm, T, min_pairs, min_pivot)
        st.append(stats_of(sm, xi))
    return T, np.array(st), sm


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------

B = 3
GRID = (48, 64)
K_GRID = ((60.0, 60.0, 31.5, 23.5), (61.5, 58.75, 31.125, 23.875), (58.25, 61.0, 32.0, 23.25))      # per image, for the 48 x 64 grid
K_MODEL_37x53 = ((49.0, 50.0, 26.25, 18.125), (50.5, 48.75, 25.75, 18.375), (48.25, 49.5, 26.5, 17.75))      # another camera, 37 x 53
K_HALF = tuple((0.5 * a, 0.5 * b, 0.5 * c - 0.25, 0.5 * d - 0.25) for a, b, c, d in K_GRID)          # f = 30, for the 24 x 32 runs
T_REF = rot(0.03, -0.05, 0.02, (0.05, -0.02, 0.1))    # camera-from-world of the model camera
# the true current-to-model motions: about 2.2 deg / 5.4 cm, 4.1 deg / 8.8 cm, 6.4 deg / 16 cm; image b moves a few percent differently
# (undamped Gauss-Newton from the identity does not converge from every direction of that size: these are directions from which the
# float64 restatement does, at every image and stride -- test_icp_abi.py asserts it)
MOTIONS = (((0.02, -0.03, 0.015), (0.03, -0.02, 0.04)), ((0.04, -0.05, 0.03), (0.05, 0.04, 0.06)), ((0.06, -0.08, -0.05), (0.1, 0.08, 0.1)))
_VARY = ((1.0, 1.0), (0.93, 1.05), (1.06, 0.95))


def motion(m, b=0, part=1.0):
    """The float64 [R|t] current-to-model of motion m for image b; `part` scales angles and translation (a start pose on the way)."""
    ang, t = MOTIONS[m]
    fa, ft = _VARY[b]
    return rot(*(part * fa * a for a in ang), tuple(part * ft * v for v in t))


def current_pose(T_rel, T_ref=T_REF):
    """Camera-from-world (float64) of the camera whose points T_rel takes into the camera T_ref."""
    Rm, t = mat(T_rel)
    Rr, tr = mat(T_ref)
    return np.concatenate([Rm.T @ Rr, (Rm.T @ (tr - t))[:, None]], 1).ravel()


# name: prediction size (seen on the 48 x 64 grid), stride, src normals, both std inputs, the model grid and camera, the motion
ICP_CASES = {
    "stride1_plain": dict(h=48, w=64, stride=1, normals=False, std=False, Hm=48, Wm=64, Km=K_GRID, m=0),
    "stride2_std": dict(h=48, w=64, stride=2, normals=False, std=True, Hm=48, Wm=64, Km=K_GRID, m=1),
    "stride3_normals": dict(h=48, w=64, stride=3, normals=True, std=False, Hm=48, Wm=64, Km=K_GRID, m=1),
    "stride1_normals_std": dict(h=48, w=64, stride=1, normals=True, std=True, Hm=48, Wm=64, Km=K_GRID, m=2),
    "model_37x53": dict(h=48, w=64, stride=1, normals=False, std=True, Hm=37, Wm=53, Km=K_MODEL_37x53, m=0),
    "blend_24x32": dict(h=24, w=32, stride=1, normals=False, std=True, Hm=48, Wm=64, Km=K_GRID, m=1),
}
CASE_COS_MIN = 0.98                                    # tight enough to drop the pairs across the sphere's rim
START_PART = 0.5                                       # the pose the single steps start from: half of the true motion


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict of read-only float32 arrays of the case: pred [B,h,w], std [B,h,w] or None, md [B,Hm,Wm], mn [B,Hm,Wm,3], ms [B,Hm,Wm] or
    None, nsrc [B,H,W,3] or None (the float32 restatement of cfp_depth_unproject's normals), K, Km [B,4], T [B,12] (the start pose),
    T_true [B,12] float64.  Image 2 carries a NaN / Inf patch in its depth and a NaN patch in its std; image 1's model map a NaN block."""
    c = ICP_CASES[name]
    h, w = c["h"], c["w"]
    H, W = GRID
    xs, ys = np.arange(w) * ((W - 1) / max(w - 1, 1)), np.arange(h) * ((H - 1) / max(h - 1, 1))
    rng = np.random.default_rng(7100 + 13 * len(name) + c["stride"])
    T_true = np.stack([motion(c["m"], b) for b in range(B)])
    pred = np.stack([scene(K_GRID[b], current_pose(T_true[b]), h, w, xs, ys)[0] for b in range(B)]).astype(np.float32)
    model = [scene(c["Km"][b], T_REF, c["Hm"], c["Wm"]) for b in range(B)]
    md = np.stack([m[0] for m in model]).astype(np.float32)
    mn = np.stack([m[1] for m in model]).astype(np.float32)
    std = (0.02 + 0.02 * rng.random((B, h, w))).astype(np.float32) if c["std"] else None
    ms = (0.01 + 0.004 * md + 0.002 * rng.random(md.shape)).astype(np.float32) if c["std"] else None
    pred[2, h // 3:h // 3 + h // 8, w // 2:w // 2 + w // 8] = np.nan
    pred[2, 5:7, 3:6] = np.inf
    pred[2, 14:16, 8:10] = -np.inf
    if std is not None:
        std[2, 6:9, 12:16] = np.nan                                                   # takes the floor
        std[0, 2, 20:23] = np.inf                                                     # observes nothing
        ms[1, 3:5, 30:34] = np.nan                                                    # counts as 0
    md[1, 20:26, 10:18] = np.nan
    mn[1, 20:26, 10:18] = np.nan
    mn[0, 30:33, 40:44] = 0.0                                                         # unproject's "no normal"
    nsrc = None
    if c["normals"]:
        nsrc = np.stack([P.normals(P.depth(pred[b], H, W, int((h, w) != GRID)), K_GRID[b]) for b in range(B)])
    T = np.stack([motion(c["m"], b, START_PART) for b in range(B)]).astype(np.float32)
    out = dict(pred=pred, std=std, md=md, mn=mn, ms=ms, nsrc=nsrc, K=np.array(K_GRID, np.float32), Km=np.array(c["Km"], np.float32), T=T,
               T_true=T_true)
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


def case_kw(name):
    c = ICP_CASES[name]
    return dict(stride=c["stride"], cos_min=CASE_COS_MIN if c["normals"] else COS_MIN)


def case_maps(name, b, dt):
    """The arguments of `pairs` up to Km for image b of the case in dt."""
    c, x = ICP_CASES[name], inputs(name)
    H, W = GRID
    interp = int((c["h"], c["w"]) != GRID)
    d = P.depth(x["pred"][b], H, W, interp, dt=dt)
    s = None if x["std"] is None else P.plane_to_grid(x["std"][b], H, W, dt)
    f = lambda a: None if a is None else a[b].astype(dt)
    return d, s, f(x["nsrc"]), x["K"][b], f(x["md"]), f(x["mn"]), f(x["ms"]), x["Km"][b]


@functools.lru_cache(maxsize=None)
def case_pairs(name, b, dt=np.float32):
    """`pairs` of image b of the case at its start pose in dt -- read-only, shared."""
    return pairs(*case_maps(name, b, dt), inputs(name)["T"][b], **case_kw(name))


def guard_measured():
    """GUARD: 4 x the worst |u32 - u64|, |v32 - v64| in pixels over the source pixels of every case that both restatements put in front
    of the model camera and whose projection lies within a pixel of the model grid."""
    global GUARD_MEASURED
    if GUARD_MEASURED is None:
        worst = 0.0
        for name, c in ICP_CASES.items():
            for b in range(B):
                a, d = case_pairs(name, b), case_pairs(name, b, np.float64)
                with np.errstate(invalid="ignore"):
                    sel = np.isfinite(a["u"]) & np.isfinite(d["u"]) & (d["Zp"] >= Z_NEAR) & (a["Zp"] >= Z_NEAR) & (d["u"] > -2) & \
                        (d["u"] < c["Wm"] + 1) & (d["v"] > -2) & (d["v"] < c["Hm"] + 1)
                worst = max(worst, float(np.abs(a["u"][sel] - d["u"][sel]).max()), float(np.abs(a["v"][sel] - d["v"][sel]).max()))
        GUARD_MEASURED = 4.0 * worst
    return GUARD_MEASURED


@functools.lru_cache(maxsize=None)
def case_excluded(name, b):
    """[H,W] bool: the source pixels of the stride grid left out of the exact comparison of the pairing (float64 quantities)."""
    r = case_pairs(name, b, np.float64)
    g = guard_measured()
    zn, d2 = float(np.float32(Z_NEAR)), float(np.float32(DIST_MAX)) ** 2
    cm = float(np.float32(case_kw(name)["cos_min"]))
    with np.errstate(invalid="ignore"):
        near = (np.abs(r["u"] + 0.5 - np.rint(r["u"] + 0.5)) < g) | (np.abs(r["v"] + 0.5 - np.rint(r["v"] + 0.5)) < g)
        near |= np.abs(r["Zp"] - zn) <= Z_BAND * zn
        near |= np.abs(r["dd"] - d2) <= DIST_BAND * d2
        near |= np.abs(r["cos"] - cm) <= COS_BAND
    return near & r["on"]


def step_gap(name):
    """The float32-vs-float64 gap of the restatement over the images of a case: (worst |sum32 - sum64| / scale over the 30 sums, worst
    |T'32 - T'64| per entry of one step from the start pose), both on the float64 pairing."""
    gs = gt = 0.0
    for b in range(B):
        idx = case_pairs(name, b, np.float64)["index"]
        T = inputs(name)["T"][b]
        res = []
        for dt in (np.float32, np.float64):
            s, scale = sums(pairs(*case_maps(name, b, dt), T, index=idx, **case_kw(name)))
            res.append((s, scale, step(s, T)[0]))
        gs = max(gs, float((np.abs(res[0][0] - res[1][0]) / np.maximum(res[1][1], 1e-300)).max()))
        gt = max(gt, float(np.abs(res[0][2].astype(np.float64) - res[1][2]).max()))
    return gs, gt


# ---- convergence -------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def converge_inputs(m, half=False):
    """The frames of the convergence runs of motion m: dict like `inputs` without std and normals; `half`: 24 x 32 frames and model maps
    with f = 30."""
    Ks = K_HALF if half else K_GRID
    H, W = (24, 32) if half else GRID
    T_true = np.stack([motion(m, b) for b in range(B)])
    pred = np.stack([scene(Ks[b], current_pose(T_true[b]), H, W)[0] for b in range(B)]).astype(np.float32)
    model = [scene(Ks[b], T_REF, H, W) for b in range(B)]
    out = dict(pred=pred, md=np.stack([x[0] for x in model]).astype(np.float32), mn=np.stack([x[1] for x in model]).astype(np.float32),
               K=np.array(Ks, np.float32), T_true=T_true)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def converge_reference(m, stride, iters, half=False):
    """The float64 restatement from the identity: per image (T float32 [12], stats, (rotation error deg, translation error m))."""
    x = converge_inputs(m, half)
    H, W = x["pred"].shape[1:]
    out = []
    for b in range(B):
        d = P.depth(x["pred"][b], H, W, 0, dt=np.float64)
        T, st, _ = run(d, None, None, x["K"][b], x["md"][b].astype(np.float64), x["mn"][b].astype(np.float64), None, x["K"][b],
                       iters=iters, stride=stride)
        out.append((T, st, pose_error(T, x["T_true"][b])))
    return out


# ---- the Tracker's sequence ----------------------------------------------------------------------------------------------------------------

TRACK_DIMS, TRACK_ORIGIN, TRACK_VOXEL, TRACK_TRUNC = (46, 46, 44), (-1.62, -0.78, 1.42), 0.05, 0.25      # holds the room's visible corner
TRACK_HI, TRACK_ITERS, TRACK_FRAMES = 5.0, 10, 4
_TRACK_ANGLES = ((0.0, 0.0, 0.0), (0.02, -0.025, 0.01), (0.035, -0.05, 0.02), (0.05, -0.07, 0.035))      # frame after frame about 2 deg
_TRACK_SHIFTS = ((0.0, 0.0, 0.0), (0.03, -0.01, 0.03), (0.05, -0.03, 0.06), (0.08, -0.04, 0.08))         # and 4 cm further


def track_pose(f, b):
    """Camera-from-world (float64) of frame f of image b: looking down and to the left, at the room's corner."""
    (ax, ay, az), (tx, ty, tz), (fa, ft) = _TRACK_ANGLES[f], _TRACK_SHIFTS[f], _VARY[b]
    return rot(0.2 + fa * ax, 0.25 + fa * ay, 0.02 + fa * az, (0.05 + ft * tx, -0.02 + ft * ty, 0.1 + ft * tz))


@functools.lru_cache(maxsize=None)
def track_frames():
    """Per frame (pred [B,48,64] f32, std [B,48,64] f32, T_true [B,12] f32) -- read-only."""
    H, W = GRID
    rng = np.random.default_rng(7300)
    out = []
    for f in range(TRACK_FRAMES):
        T = np.stack([track_pose(f, b) for b in range(B)])
        pred = np.stack([scene(K_GRID[b], T[b], H, W)[0] for b in range(B)]).astype(np.float32)
        std = (0.015 + 0.01 * rng.random((B, H, W))).astype(np.float32)
        T = T.astype(np.float32)
        for a in (pred, std, T):
            a.setflags(write=False)
        out.append((pred, std, T))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def track_reference():
    """The chain `Tracker` runs, on the CPU in float64 (tsdf_ref + this file): frame 0 integrated at its true pose, then per frame
    raycast at the last pose, `TRACK_ITERS` iterations from the identity against that raycast with both std maps, the world pose, the
    frame integrated at it -> dict: poses [frames,B,12] f32, errors [frames,B,2] (deg, m) against the truth, first (depth, normal,
    surface) of image 0's first raycast."""
    import tsdf_ref as S
    H, W = GRID
    fr = track_frames()
    poses, errs, first = [fr[0][2].copy()], [np.zeros((B, 2))], None
    vols = []
    for b in range(B):
        d, s = P.depth(fr[0][0][b], H, W, 0, hi=TRACK_HI, dt=np.float64), fr[0][1][b].astype(np.float64)
        vols.append(S.integrate(S.empty_volume(TRACK_DIMS, np.float64), d, s, K_GRID[b], fr[0][2][b], TRACK_DIMS, TRACK_ORIGIN, TRACK_VOXEL,
                                TRACK_TRUNC)["vol"])
    for f in range(1, TRACK_FRAMES):
        new, err = [], []
        for b in range(B):
            last = poses[-1][b]
            r = S.raycast(vols[b], K_GRID[b], last, H, W, TRACK_ORIGIN, TRACK_VOXEL, Z_NEAR, TRACK_HI, 0.5 * TRACK_TRUNC)
            if first is None:
                first = (r["depth"], r["normal"], scene(K_GRID[b], last, H, W)[2])
            d, s = P.depth(fr[f][0][b], H, W, 0, hi=TRACK_HI, dt=np.float64), fr[f][1][b].astype(np.float64)
            T, _, _ = run(d, s, None, K_GRID[b], r["depth"], r["normal"], r["std"], K_GRID[b], iters=TRACK_ITERS)
            cur = world(T, last)
            new.append(cur)
            err.append(pose_error(cur, track_pose(f, b)))
            vols[b] = S.integrate(vols[b], d, s, K_GRID[b], cur, TRACK_DIMS, TRACK_ORIGIN, TRACK_VOXEL, TRACK_TRUNC)["vol"]
        poses.append(np.stack(new))
        errs.append(np.array(err))
    return dict(poses=np.stack(poses), errors=np.stack(errs), first=first)
