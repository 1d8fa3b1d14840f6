"""numpy restatement of the definitions of `cfp_depth_unproject` and `cfp_points_compact` (include/cfpnet_hip.h) -- TEST INFRASTRUCTURE.

Written twice: in float32 with the header's order of operations (numpy rounds every float32 operation once, like the library built
without fused multiply-adds), and in float64 with the normal as the plain cross product of point differences.  The float32 form is what
the GPU results are compared with; the float64 form measures how far float32 arithmetic alone moves a normal (`normal_angle_measured`,
which sets the GPU tests' angular tolerance) and decides which pixels a compaction keeps (`keep_mask`), with thresholds that no pixel
comes near (`guard_band`).  Also the inputs the GPU tests use, so that the CPU tests can examine the same tensors."""
import functools

import numpy as np

from cfpnet_amd import synthetic

RTOL = 2e-5              # tests/test_metrics.py
LO, HI = 1e-3, 10.0
GUARD = 1e-4             # no reference value within this relative distance of a threshold
ZJUL5 = (611.2, 609.6, 323.4, 244.9)
NORMAL_ANGLE_MEASURED = None          # radians; set by normal_angle_measured()


# ---- depth: met_pred in mode 0 / met_plane (csrc/metrics_pred.h) -------------------------------------------------------------------------

def _taps(n_src, n_dst, dt):
    """Align-corners source index and weight along one dimension: (i0, i1, l, h) in dtype dt."""
    s = dt(n_src - 1) / dt(n_dst - 1) if n_dst > 1 else dt(0)
    f = (s * np.arange(n_dst).astype(dt)).astype(dt)
    i0 = np.minimum(f.astype(np.int64), n_src - 1)
    i1 = i0 if n_src == n_dst else np.minimum(i0 + 1, n_src - 1)
    l = (f - i0.astype(dt)).astype(dt)
    return i0, i1, l, (dt(1) - l).astype(dt)


def _blend(p, H, W, dt):
    y0, y1, ly, hy = _taps(p.shape[0], H, dt)
    x0, x1, lx, hx = _taps(p.shape[1], W, dt)
    ly, hy, lx, hx = ly[:, None], hy[:, None], lx[None, :], hx[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        return hy * (hx * p[np.ix_(y0, x0)] + lx * p[np.ix_(y0, x1)]) + ly * (hx * p[np.ix_(y1, x0)] + lx * p[np.ix_(y1, x1)])


def depth(pred, H, W, interpolate, lo=LO, hi=HI, dt=np.float32):
    """pred [Hp,Wp] f32 -> d [H,W] in dt: clip to [f32(lo), f32(hi)] (NaN passes), then the blend."""
    p = np.clip(pred.astype(np.float32), np.float32(lo), np.float32(hi)).astype(dt)
    if not interpolate:
        assert p.shape == (H, W)
        return p
    out = _blend(p, H, W, dt)
    assert out.dtype == dt
    return out


def plane_to_grid(u, H, W, dt=np.float32):
    """met_plane: read directly at equal sizes, the same blend without a clip otherwise."""
    u = u.astype(np.float32).astype(dt)
    return u if u.shape == (H, W) else _blend(u, H, W, dt)


# ---- points and normals ------------------------------------------------------------------------------------------------------------------

def _rays(K, H, W, dt):
    fx, fy, cx, cy = (dt(np.float32(v)) for v in K)
    rx = ((np.arange(W).astype(dt) - cx) / fx).astype(dt)
    ry = ((np.arange(H).astype(dt) - cy) / fy).astype(dt)
    return rx, ry


def points(d, K):
    """P = (rx * d, ry * d, d) in d's dtype, [H,W,3]."""
    dt = d.dtype.type
    rx, ry = _rays(K, *d.shape, dt)
    with np.errstate(invalid="ignore"):
        return np.stack([rx[None, :] * d, ry[:, None] * d, d], -1)


def _neighbours(n):
    i = np.arange(n)
    return np.maximum(i - 1, 0), np.minimum(i + 1, n - 1)


def tangents_closed(d, K):
    """(T_x, T_y) [H,W,3] in d's dtype by the header's cancellation-free form."""
    dt = d.dtype.type
    H, W = d.shape
    fx, fy, cx, cy = (dt(np.float32(v)) for v in K)
    rx, ry = _rays(K, H, W, dt)
    x0, x1 = _neighbours(W)
    y0, y1 = _neighbours(H)
    with np.errstate(invalid="ignore"):
        d0, d1, e0, e1 = d[:, x0], d[:, x1], d[y0, :], d[y1, :]
        kx, ky = (x1 - x0).astype(dt), (y1 - y0).astype(dt)
        xm, ym = dt(0.5) * (x0 + x1).astype(dt), dt(0.5) * (y0 + y1).astype(dt)
        dd, ds, ed, es = d1 - d0, d1 + d0, e1 - e0, e1 + e0
        tx = np.stack([dd * ((xm - cx) / fx)[None, :] + ds * (dt(0.5) * kx / fx)[None, :], dd * ry[:, None], dd], -1)
        ty = np.stack([ed * rx[None, :], ed * ((ym - cy) / fy)[:, None] + es * (dt(0.5) * ky / fy)[:, None], ed], -1)
    assert tx.dtype == d.dtype and ty.dtype == d.dtype
    return tx, ty


def tangents_diff(d, K):
    """(T_x, T_y) as differences of the points of the clamped neighbours."""
    P = points(d, K)
    x0, x1 = _neighbours(d.shape[1])
    y0, y1 = _neighbours(d.shape[0])
    with np.errstate(invalid="ignore"):
        return P[:, x1] - P[:, x0], P[y1, :] - P[y0, :]


def _finite5(d):
    x0, x1 = _neighbours(d.shape[1])
    y0, y1 = _neighbours(d.shape[0])
    f = np.isfinite(d)
    return f & f[:, x0] & f[:, x1] & f[y0, :] & f[y1, :]


def _normalize(tx, ty, ok5):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        nx = ty[..., 1] * tx[..., 2] - ty[..., 2] * tx[..., 1]
        ny = ty[..., 2] * tx[..., 0] - ty[..., 0] * tx[..., 2]
        nz = ty[..., 0] * tx[..., 1] - ty[..., 1] * tx[..., 0]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        ok = ok5 & (ln > 0) & np.isfinite(ln)
        n = np.stack([nx / ln, ny / ln, nz / ln], -1)
    n[~ok] = 0
    return n


def normals(d, K):
    """float32 d: the header's form in its order.  float64 d: the cross product of the point differences."""
    tx, ty = tangents_closed(d, K) if d.dtype == np.float32 else tangents_diff(d, K)
    n = _normalize(tx, ty, _finite5(d))
    assert n.dtype == d.dtype
    return n


def angle(a, b):
    """Angle in radians between the rows of a and b (float64, atan2 form: exact near 0)."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1))


# ---- compaction ----------------------------------------------------------------------------------------------------------------------------

def keep_mask(z, stride, near, far, u=None, unc_range=None):
    """[H,W] bool from Z [H,W] and the uncertainty u [H,W] on the same grid (or None); thresholds as the float32 the kernel receives."""
    H, W = z.shape
    grid = np.zeros((H, W), bool)
    grid[::stride, ::stride] = True
    with np.errstate(invalid="ignore"):
        keep = grid & np.isfinite(z) & (z > np.float32(near)) & (z < np.float32(far))
        if u is not None:
            keep &= (u >= np.float32(unc_range[0])) & (u <= np.float32(unc_range[1]))
    return keep


def guard_band(values, thresholds):
    """Smallest |v - t| / |t| over the finite values and the finite thresholds."""
    v = np.asarray(values, np.float64).ravel()
    v = v[np.isfinite(v)]
    worst = np.inf
    for t in thresholds:
        t = float(np.float32(t))
        if np.isfinite(t) and v.size:
            gap = float(np.abs(v - t).min())
            worst = min(worst, gap / abs(t) if t != 0 else (np.inf if gap > 0 else 0.0))
    return worst


# ---- the inputs of tests/test_pointcloud_gpu.py ------------------------------------------------------------------------------------------

K_BATCH = ((611.2, 609.6, 323.4, 244.9), (35.5, 36.25, 26.0, 18.0), (48.0, 47.0, 20.5, 22.75))
PLANE_N, PLANE_C = (0.3, -0.2, -float(np.sqrt(0.87))), -2.0       # unit normal facing the camera; n . P = c

# name: pred size, output size, interpolate, intrinsics per image
UNPROJECT_CASES = {
    "odd_19x27_to_37x53": dict(h=19, w=27, H=37, W=53, interp=1, K=((40.0, 41.5, 25.3, 17.9),)),
    "same_24x40_interp": dict(h=24, w=40, H=24, W=40, interp=1, K=((30.0, 31.0, 19.5, 11.5),)),
    "same_24x40_direct": dict(h=24, w=40, H=24, W=40, interp=0, K=((30.0, 31.0, 19.5, 11.5),)),
    "row_1x33": dict(h=1, w=17, H=1, W=33, interp=1, K=((25.0, 25.0, 16.0, 0.0),)),
    "column_33x1": dict(h=17, w=1, H=33, W=1, interp=1, K=((25.0, 25.0, 0.0, 16.0),)),
    "full_240x320_to_480x640": dict(h=240, w=320, H=480, W=640, interp=1, K=(ZJUL5,)),
    "batch3_nonfinite": dict(h=19, w=27, H=37, W=53, interp=1, K=K_BATCH),
    "plane_48x72": dict(h=48, w=72, H=48, W=72, interp=0, K=((60.0, 58.0, 35.5, 23.5),)),
}


def plane_depth(H, W, K):
    """Depth of the plane PLANE_N . P = PLANE_C along every pixel's ray, float64."""
    rx, ry = _rays(K, H, W, np.float64)
    return PLANE_C / (PLANE_N[0] * rx[None, :] + PLANE_N[1] * ry[:, None] + PLANE_N[2])


@functools.lru_cache(maxsize=None)
def unproject_inputs(name):
    """(pred [B,h,w] f32, K [B,4] f32) -- treat as read-only."""
    c = UNPROJECT_CASES[name]
    h, w, H, W = c["h"], c["w"], c["H"], c["W"]
    if name == "batch3_nonfinite":
        pred = np.stack([synthetic.make_eval_pair(H, W, h, w, 50 + b, 0.1, 0.15)[1] for b in range(3)])
        assert (pred < LO).any() and (pred > HI).any()
        pred[2, 2:5, 3:6] = np.nan
        pred[2, 9:11, 20:23] = np.inf
        pred[2, 14:17, 8:10] = -np.inf
        pred[2, 18, 26] = np.nan                      # a corner
    elif name.startswith(("row", "column")):
        pred = synthetic.make_depth(h, w, seed=61 if h == 1 else 62)[None]
    elif name == "plane_48x72":
        pred = plane_depth(H, W, c["K"][0]).astype(np.float32)[None]
        assert pred.min() > LO and pred.max() < HI
    else:
        pred = synthetic.make_eval_pair(H, W, h, w, {19: 41, 24: 42, 240: 43}[h], 0.1, 0.15)[1][None]
    K = np.array(c["K"], np.float32)
    assert K.shape == (pred.shape[0], 4)
    pred = np.ascontiguousarray(pred, np.float32)
    pred.setflags(write=False)
    K.setflags(write=False)
    return pred, K


@functools.lru_cache(maxsize=None)
def unproject_reference(name, dt=np.float32):
    """(points [B,H,W,3], normals [B,H,W,3]) in dt -- read-only, shared by the tests."""
    c = UNPROJECT_CASES[name]
    pred, K = unproject_inputs(name)
    ds = [depth(pred[b], c["H"], c["W"], c["interp"], dt=dt) for b in range(pred.shape[0])]
    P = np.stack([points(d, K[b]) for b, d in enumerate(ds)])
    N = np.stack([normals(d, K[b]) for b, d in enumerate(ds)])
    P.setflags(write=False)
    N.setflags(write=False)
    return P, N


@functools.lru_cache(maxsize=None)
def case_angle(name):
    """Worst angle between the float32 and the float64 restatement on one case, over the pixels where both normals are non-zero."""
    n32, n64 = unproject_reference(name)[1], unproject_reference(name, np.float64)[1]
    nz = (n32 != 0).any(-1)
    assert np.array_equal(nz, (n64 != 0).any(-1)), name
    return float(angle(n32[nz], n64[nz]).max()) if nz.any() else 0.0


# The plane case samples an exact plane in float64 and rounds the depths to float32: each sample is off by at most 2^-24 d along its ray
# (|r| <= 1.25 here), so a tangent -- the difference of two points 2 d / fx apart or more -- turns by at most
# 2 * 1.25 * 2^-24 d_max / (2 d_min / fx) and the normal by at most the sum over both tangents; with d_max / d_min < 2 on this plane that is
# below 5 * 2^-24 * fx.  Doubled for the foreshortening of the tilted tangents.
PLANE_ANGLE_BOUND = 10 * 2.0 ** -24 * 60.0


def normal_angle_measured():
    """The worst angle between the float32 and the float64 restatement over every input of the GPU tests, wherever both normals are
    non-zero (they are zero at the same pixels).  Stored as NORMAL_ANGLE_MEASURED; the GPU tolerance is four times this."""
    global NORMAL_ANGLE_MEASURED
    if NORMAL_ANGLE_MEASURED is None:
        NORMAL_ANGLE_MEASURED = max(case_angle(name) for name in UNPROJECT_CASES)
    return NORMAL_ANGLE_MEASURED


# Compaction: the dense map of an unproject case (batched by repeating / re-seeding), a stride, a depth range and optionally an interval
# of a half-resolution uncertainty plane.  The thresholds sit where the float64 reference has no value within GUARD (asserted on the
# CPU in test_pointcloud_abi.py), so kernel and reference cannot disagree about a pixel and nothing is excluded from a comparison.
COMPACT_CASES = {
    "small_s1": dict(shape="small", stride=1, near=0.8125, far=2.4375, unc=None),
    "small_s2": dict(shape="small", stride=2, near=0.8125, far=2.4375, unc=None),
    "small_s3_unc": dict(shape="small", stride=3, near=0.03125, far=7.5, unc=(0.0, 0.15)),
    "small_s1_unc": dict(shape="small", stride=1, near=0.8125, far=2.4375, unc=(0.1, 0.5)),
    "full_s1": dict(shape="full", stride=1, near=0.03125, far=7.5, unc=None),
    "full_s2_unc": dict(shape="full", stride=2, near=0.03125, far=7.5, unc=(0.0, 0.15)),
    "full_s3_unc": dict(shape="full", stride=3, near=0.03125, far=7.5, unc=(0.1, 0.5)),
    "full_none_kept": dict(shape="full", stride=1, near=20.0, far=30.0, unc=None),
    "small_all_kept": dict(shape="small", stride=1, near=0.0, far=float("inf"), unc=None),
}
COMPACT_SHAPES = {"small": dict(h=19, w=27, H=37, W=53, K=((40.0, 41.5, 25.3, 17.9), (35.5, 36.25, 26.0, 18.0)), seeds=(41, 44),
                                 unc_seeds=(304, 311)),
                  "full": dict(h=240, w=320, H=480, W=640, K=(ZJUL5, ZJUL5), seeds=(43, 45), unc_seeds=(343, 345))}
UNC_LEVELS = (0.05, 0.30)                             # the uncertainty plane: blobs of the second level on a floor of the first


@functools.lru_cache(maxsize=None)
def compact_inputs(shape):
    """(pred [2,h,w] f32, K [2,4] f32, unc [2,3,h,w] f32: plane 0 blobs of two levels from make_depth's holes, planes 1 / 2 other data)."""
    s = COMPACT_SHAPES[shape]
    h, w, H, W = s["h"], s["w"], s["H"], s["W"]
    pred = np.stack([synthetic.make_eval_pair(H, W, h, w, seed, 0.1, 0.15)[1] for seed in s["seeds"]])
    if shape == "small":
        pred[1, 4:6, 5:8] = np.nan                    # NaN points never pass the range test
    unc = np.empty((2, 3, h, w), np.float32)
    for b, seed in enumerate(s["unc_seeds"]):
        holes = synthetic.make_depth(h, w, seed=seed, holes=0.3) == 0
        unc[b, 0] = np.where(holes, np.float32(UNC_LEVELS[1]), np.float32(UNC_LEVELS[0]))
        unc[b, 1] = synthetic.make_depth(h, w, seed=seed + 1)
        unc[b, 2] = 0.5
    if shape == "small":
        unc[1, 0, 10, 10:13] = np.nan                 # a NaN uncertainty fails the interval
    K = np.array(s["K"], np.float32)
    for a in (pred, K, unc):
        a.setflags(write=False)
    return pred, K, unc


@functools.lru_cache(maxsize=None)
def compact_reference(name):
    """-> (keep [2,H,W] bool from the float64 reference, guard: the smallest relative distance of a reference value to a threshold)."""
    c = COMPACT_CASES[name]
    s = COMPACT_SHAPES[c["shape"]]
    pred, K, unc = compact_inputs(c["shape"])
    H, W = s["H"], s["W"]
    keep, guard = [], np.inf
    for b in range(2):
        z = depth(pred[b], H, W, 1, dt=np.float64)
        on_grid = np.zeros((H, W), bool)
        on_grid[::c["stride"], ::c["stride"]] = True
        guard = min(guard, guard_band(z[on_grid], (c["near"], c["far"])))
        u = None
        if c["unc"] is not None:
            u = plane_to_grid(unc[b, 0], H, W, np.float64)
            guard = min(guard, guard_band(u[on_grid], c["unc"]))
        keep.append(keep_mask(z, c["stride"], c["near"], c["far"], u, c["unc"]))
    keep = np.stack(keep)
    keep.setflags(write=False)
    return keep, guard


# --points_max_std of the command-line test (metres).  The deterministic key-addressed weights are untrained: their bin distribution is
# wide, with a standard deviation of 0.5 .. 3.5 m and a median of 2.54 m on the two synthetic samples, so this keeps about half the pixels.
CLI_MAX_STD = 2.5


# ---- comparisons -------------------------------------------------------------------------------------------------------------------------

def close_points(got, want, what=""):
    """The project's bound |got - want| <= RTOL * max(|want|, 1e-3) per coordinate against the float32 restatement; NaN at exactly the
    same places.  Returns the worst ratio to the bound."""
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape, got.dtype)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    g, w = got[~nan].astype(np.float64), want[~nan].astype(np.float64)
    ratio = np.abs(g - w) / (RTOL * np.maximum(np.abs(w), 1e-3))
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{what}: points worst |got - want| / bound = {worst:.3e} over {g.size} coordinates, {int(nan.sum())} NaN")
    assert worst <= 1.0, (what, worst)
    return worst


def close_normals(got, want, tol, what=""):
    """Zero normals at exactly the same pixels; elsewhere unit length and within `tol` radians of the float32 restatement."""
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape, got.dtype)
    zero = (want == 0).all(-1)
    assert not np.isnan(got).any(), what
    assert np.array_equal((got == 0).all(-1), zero), what
    g, w = got[~zero], want[~zero]
    worst = float(angle(g, w).max()) if g.size else 0.0
    length = float(np.abs(np.linalg.norm(g.astype(np.float64), axis=-1) - 1.0).max()) if g.size else 0.0
    print(f"{what}: normals worst angle = {worst:.3e} rad (tolerance {tol:.3e}), worst | |n| - 1 | = {length:.3e}, {int(zero.sum())} zero")
    assert worst <= tol and length <= 4 * 2.0 ** -23, (what, worst, tol, length)
    return worst
