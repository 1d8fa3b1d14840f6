"""numpy restatement of the definition of `cfp_luma` and `cfp_icp_rgb_step` (include/cfpnet_hip.h) -- TEST INFRASTRUCTURE.

Extends `icp_ref.py`: the geometric half IS `icp_ref.pairs` / `icp_ref.sums`; this file adds the photometric pair, its 30 sums and the
step on the sum of the two systems, for the same two dtypes (float32 in the header's order of operations -- what the GPU's sums are
compared with; float64 -- which decides the discrete result: which pixels form a photometric pair).  The photometric pairing can differ
between float32 and float64 only where `icp_ref`'s can, where u or v lies within GUARD of an integer (the cell of the blend changes; this
includes the two border limits x0 = 0 and x0 + 1 = Wm - 1), or where |rI| lies within PHOTO_BAND relative of photo_max: those pixels
join the excluded set.

The texture is an albedo painted on the analytic scene of `icp_ref`: a smooth function of the WORLD point, two sinusoids around 0.5,
rendered in float64 for any camera.  Also the inputs the GPU tests use."""
import functools

import numpy as np

import icp_ref as I
import pointcloud_ref as P

PHOTO_STD, PHOTO_MAX = 0.04, 0.25
PHOTO_WEIGHT = 1.0 / (PHOTO_STD * PHOTO_STD)
PHOTO_BAND = 1e-4
NT = 60
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TINT = (1.0, 0.9, 0.8)                                # the colour of the painted scene: albedo times this, per channel


# ---- cfp_luma --------------------------------------------------------------------------------------------------------------------------------

def luma(rgb, layout, mean=MEAN, std=STD):
    """float32 in the header's order.  layout 0: [B,3,H,W] normalised; 1: [B,H,W,3] in 0..1 -> [B,H,W] f32."""
    rgb = rgb.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        if layout == 0:
            c = [rgb[:, k] * np.float32(std[k]) + np.float32(mean[k]) for k in range(3)]
        else:
            c = [rgb[..., k] for k in range(3)]
        y = (np.float32(0.299) * c[0] + np.float32(0.587) * c[1]) + np.float32(0.114) * c[2]
    assert y.dtype == np.float32
    return np.where(np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2]), y, np.float32(np.nan))


def luma64(c):
    """The luminance of a colour [...,3] in 0..1, float64."""
    return 0.299 * c[..., 0] + 0.587 * c[..., 1] + 0.114 * c[..., 2]


# ---- the texture -----------------------------------------------------------------------------------------------------------------------------

WAVES = ((0.15, np.array([2.3, 1.1, 1.6]), 0.3), (0.10, np.array([-1.2, 2.4, 0.9]), 1.1))      # amplitude, wave vector (rad / m), phase


def albedo(Pw, waves=WAVES):
    """Pw [...,3] world points -> albedo in [0.25, 0.75], float64."""
    return 0.5 + sum(a * np.sin(Pw @ k + ph) for a, k, ph in waves)


def world_points(K, T, H, W, xs=None, ys=None):
    """The world points the camera K at the camera-from-world pose T sees on its grid, float64 [H,W,3] (NaN where a ray hits nothing),
    and the surface index."""
    d, _, which = I.scene(K, T, H, W, xs, ys)
    fx, fy, cx, cy = (float(np.float32(v)) for v in K)
    xs = np.arange(W, dtype=np.float64) if xs is None else xs
    ys = np.arange(H, dtype=np.float64) if ys is None else ys
    Rm, t = I.mat(T)
    d = np.where(np.isfinite(d), d, np.nan)
    Pc = np.stack(np.broadcast_arrays(((xs - cx) / fx)[None, :] * d, ((ys - cy) / fy)[:, None] * d, d), -1)
    return (Pc - t) @ Rm, which                       # R^T (Pc - t)


def render(K, T, H, W):
    """The painted scene's albedo seen by the camera, float64 [H,W]."""
    return albedo(world_points(K, T, H, W)[0])


def min_period(K, T, H, W):
    """The shortest period in pixels of either sinusoid over the pixels whose right and lower neighbours lie on the same surface."""
    Pw, which = world_points(K, T, H, W)
    same = (which[:-1, :-1] == which[:-1, 1:]) & (which[:-1, :-1] == which[1:, :-1])
    worst = np.inf
    for _, k, _ in WAVES:
        ph = Pw @ k
        g = np.hypot(ph[:-1, 1:] - ph[:-1, :-1], ph[1:, :-1] - ph[:-1, :-1])[same]
        worst = min(worst, float(2 * np.pi / np.nanmax(g)))
    return worst


def to_rgb(alb):
    """An albedo plane [...,H,W] -> the normalised planar image [...,3,H,W] float32 the model reads: c = albedo * TINT."""
    c = np.stack([alb * t for t in TINT], -3)
    return ((c - np.array(MEAN)[:, None, None]) / np.array(STD)[:, None, None]).astype(np.float32)


def tint_luma(alb):
    """The luminance of the painted colour: what both lumas of a case hold."""
    return alb * (0.299 * TINT[0] + 0.587 * TINT[1] + 0.114 * TINT[2])


# ---- the photometric pair ----------------------------------------------------------------------------------------------------------------------

def bilinear(ml, u, v):
    """The header's interpolant of ml [Hm,Wm] at (u, v) in ml's dtype -> (ok, Im, gx, gy, x0, y0): ok = the cell lies in the map and its
    four taps are finite."""
    dt = ml.dtype.type
    Hm, Wm = ml.shape
    with np.errstate(invalid="ignore", over="ignore"):
        x0, y0 = np.floor(u), np.floor(v)
        ax, ay = u - x0, v - y0
        ok = (x0 >= 0) & (x0 + dt(1) <= Wm - 1) & (y0 >= 0) & (y0 + dt(1) <= Hm - 1)
        xi, yi = np.where(ok, x0, 0).astype(np.int64), np.where(ok, y0, 0).astype(np.int64)
        one = ok.astype(np.int64)
        I00, I10, I01, I11 = ml[yi, xi], ml[yi, xi + one], ml[yi + one, xi], ml[yi + one, xi + one]
        ok = ok & np.isfinite(I00) & np.isfinite(I10) & np.isfinite(I01) & np.isfinite(I11)
        top = I00 + ax * (I10 - I00)
        bot = I01 + ax * (I11 - I01)
        Im = top + ay * (bot - top)
        gx = (I10 - I00) + ay * ((I11 - I01) - (I10 - I00))
        gy = bot - top
    return ok, Im, gx, gy, x0, y0


def moved(d, K, T):
    """X', Y', Z' of `icp_ref.pairs` in d's dtype (the same operations: the same bits)."""
    dt = d.dtype.type
    H, W = d.shape
    t = [dt(np.float32(v)) for v in np.asarray(T).ravel()[:12]]
    rx, ry = P._rays(K, H, W, dt)
    with np.errstate(invalid="ignore", over="ignore"):
        X, Y, Z = rx[None, :] * d, ry[:, None] * d, d
        return ((t[0] * X + t[1] * Y) + t[2] * Z + t[3], (t[4] * X + t[5] * Y) + t[6] * Z + t[7], (t[8] * X + t[9] * Y) + t[10] * Z + t[11])


def pairs(d, s, nsrc, K, md, mn, ms, Km, T, sl, ml, photo_max=PHOTO_MAX, index=None, photo=None, **kw):
    """`icp_ref.pairs` and the photometric pairs on top: sl [H,W] the frame's luminance, ml [Hm,Wm] the model's, in the dtype of the
    maps -> the dict of `icp_ref.pairs` plus photo [H,W] bool, rI [H,W], JI [H,W,6], Xp, Yp, x0, y0.  With `index` / `photo` the
    pairings are taken from them (the GPU's own) and no gate is applied."""
    dt = d.dtype.type
    pr = I.pairs(d, s, nsrc, K, md, mn, ms, Km, T, index=index, **kw)
    fxm, fym = dt(np.float32(Km[0])), dt(np.float32(Km[1]))
    Xp, Yp, Zp = moved(d, K, T)
    assert np.array_equal(Zp, pr["Zp"], equal_nan=True)
    ok, Im, gx, gy, x0, y0 = bilinear(ml, pr["u"], pr["v"])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        rI = Im - sl
        ok = ok & (pr["index"] >= 0) & np.isfinite(sl) & (np.abs(rI) <= dt(np.float32(photo_max)))
        gfx, gfy = gx * fxm, gy * fym
        a0, a1 = gfx / Zp, gfy / Zp
        a2 = -((gfx * (Xp / Zp) + gfy * (Yp / Zp)) / Zp)
        JI = np.stack([Yp * a2 - Zp * a1, Zp * a0 - Xp * a2, Xp * a1 - Yp * a0, a0, a1, a2], -1)
    assert rI.dtype == d.dtype and JI.dtype == d.dtype
    pr.update(photo=ok if photo is None else photo, rI=rI, JI=JI, Xp=Xp, Yp=Yp, x0=x0, y0=y0)
    return pr


def sums(pr, weight=PHOTO_WEIGHT):
    """The 60 sums -> (sums [60], scale [60]): `icp_ref.sums` of the geometric pairs, then of the photometric ones with the weight
    float32(weight) for every pair."""
    dt = pr["rI"].dtype.type
    g, gs = I.sums(pr)
    ph, phs = I.sums(dict(index=np.where(pr["photo"], 0, -1), w=np.full(pr["rI"].shape, dt(np.float32(weight)), pr["rI"].dtype),
                          r=pr["rI"], J=pr["JI"]))
    return np.concatenate([g, ph]), np.concatenate([gs, phs])


def combined(s):
    """The 30 numbers `icp_ref.step` takes: A and g of the two halves added, the geometric sum w r r, sum w and count."""
    c = np.array(s[:30], np.float64)
    c[:27] += s[30:57]
    return c


def step(s, T, min_pairs=I.MIN_PAIRS, min_pivot=I.MIN_PIVOT):
    """One finalize on the 60 sums: `icp_ref.step` on the combined system; min_pairs meets the geometric count."""
    return I.step(combined(s), T, min_pairs, min_pivot)


def stats_of(s, xi):
    rms = np.sqrt(s[57] / s[58]) if s[59] > 0 else np.nan
    return np.concatenate([I.stats_of(s[:30], xi), [s[59], rms]])


def run(d, s, nsrc, K, md, mn, ms, Km, sl, ml, T0=None, iters=10, weight=PHOTO_WEIGHT, min_pairs=I.MIN_PAIRS, min_pivot=I.MIN_PIVOT, **kw):
    """`iters` iterations from T0 (identity by default) -> (T float32 [12], stats [iters,8], sums of the last)."""
    T = I.ID12.copy() if T0 is None else np.asarray(T0, np.float32)
    st = []
    for _ in range(iters):
        sm, _ = sums(pairs(d, s, nsrc, K, md, mn, ms, Km, T, sl, ml, **kw), weight)
        T, _, xi = step(sm, T, min_pairs, min_pivot)
        st.append(stats_of(sm, xi))
    return T, np.array(st), sm


# ---- the cases: icp_ref's, painted -----------------------------------------------------------------------------------------------------------

CASES = ("stride1_plain", "stride2_std", "stride1_normals_std", "model_37x53", "blend_24x32")


@functools.lru_cache(maxsize=None)
def lumas(name):
    """(sl [B,48,64] f32, ml [B,Hm,Wm] f32) of the case, read-only: the painted scene seen by the frame's camera at its true pose and by
    the model camera.  Image 0's model picture carries a NaN block (no colour in the map there), image 1's frame a NaN and an Inf."""
    c, x = I.ICP_CASES[name], I.inputs(name)
    H, W = I.GRID
    sl = np.stack([tint_luma(render(I.K_GRID[b], I.current_pose(x["T_true"][b]), H, W)) for b in range(I.B)]).astype(np.float32)
    ml = np.stack([tint_luma(render(c["Km"][b], I.T_REF, c["Hm"], c["Wm"])) for b in range(I.B)]).astype(np.float32)
    ml[0, 8:13, 20:27] = np.nan
    sl[1, 30:33, 5:9] = np.nan
    sl[1, 40, 50] = np.inf
    sl.setflags(write=False)
    ml.setflags(write=False)
    return sl, ml


def case_maps(name, b, dt):
    """The arguments of `pairs` up to ml, without T, for image b of the case in dt."""
    sl, ml = lumas(name)
    return I.case_maps(name, b, dt), (sl[b].astype(dt), ml[b].astype(dt))


@functools.lru_cache(maxsize=None)
def case_pairs(name, b, dt=np.float32):
    geo, lum = case_maps(name, b, dt)
    return pairs(*geo, I.inputs(name)["T"][b], *lum, **I.case_kw(name))


@functools.lru_cache(maxsize=None)
def case_excluded(name, b):
    """[H,W] bool: `icp_ref.case_excluded` and the pixels whose photometric pair float32 may decide differently (float64 quantities)."""
    r = case_pairs(name, b, np.float64)
    g = I.guard_measured()
    Hm, Wm = I.ICP_CASES[name]["Hm"], I.ICP_CASES[name]["Wm"]
    with np.errstate(invalid="ignore"):
        near = (np.abs(r["u"] - np.rint(r["u"])) < g) | (np.abs(r["v"] - np.rint(r["v"])) < g)      # the cell changes, the border limits among them
        near |= (np.abs(r["u"]) < g) | (np.abs(r["u"] - (Wm - 1)) < g) | (np.abs(r["v"]) < g) | (np.abs(r["v"] - (Hm - 1)) < g)
        near |= np.abs(np.abs(r["rI"]) - PHOTO_MAX) <= PHOTO_BAND * PHOTO_MAX
    return (near & r["on"]) | I.case_excluded(name, b)


def step_gap(name):
    """The float32-vs-float64 gap of the restatement over the images of a case, both on the float64 pairings: (worst |sum32 - sum64| /
    scale over the geometric 30, the same over the photometric 30, worst |T'32 - T'64| per entry of one step from the start pose)."""
    gg = gp = gt = 0.0
    for b in range(I.B):
        ref = case_pairs(name, b, np.float64)
        T = I.inputs(name)["T"][b]
        res = []
        for dt in (np.float32, np.float64):
            geo, lum = case_maps(name, b, dt)
            s, scale = sums(pairs(*geo, T, *lum, index=ref["index"], photo=ref["photo"], **I.case_kw(name)))
            res.append((s, scale, step(s, T)[0]))
        rel = np.abs(res[0][0] - res[1][0]) / np.maximum(res[1][1], 1e-300)
        gg, gp = max(gg, float(rel[:30].max())), max(gp, float(rel[30:].max()))
        gt = max(gt, float(np.abs(res[0][2].astype(np.float64) - res[1][2]).max()))
    return gg, gp, gt


# ---- the wall: one fronto-parallel textured plane at 2 m ------------------------------------------------------------------------------------

WALL_Z = 2.0
WALL_WAVES = ((0.15, np.array([3.1, 1.3, 0.0]), 0.4), (0.10, np.array([-1.1, 2.7, 0.0]), 1.3))       # periods of 1.9 m and 2.2 m: 56 and 65 pixels
WALL_ANGLE = np.radians(1.0)
WALL_SHIFTS = ((0.01, -0.02, 0.03), (-0.02, 0.01, 0.02), (0.03, 0.02, -0.01))                         # 1 to 3 cm per axis, per image
WALL_ITERS = 12
# The depth's std, frame and model: the ToF regime photo_std is stated for.  With unit geometric weights (no std maps) the photometric
# weight 625 outvotes geometry 625 : 1 on the wall's tilt, which geometry sees exactly and the image only through the bilinear picture,
# and the float64 restatement ends 1 mm / 0.03 degrees away along the valley between a shift and a pan.
FRAME_STD, MODEL_STD = 0.02, 0.01


def wall_motion(b):
    """The true current-to-model [R|t] (float64, 12) of image b: 1 degree about each axis, the signs varied, and WALL_SHIFTS[b]."""
    sg = ((1, 1, 1), (1, -1, 1), (-1, 1, -1))[b]
    return I.rot(*(s * WALL_ANGLE for s in sg), WALL_SHIFTS[b])


@functools.lru_cache(maxsize=None)
def wall_inputs():
    """dict of read-only arrays: pred [B,48,64] f32 (the wall seen by the moved camera), md, mn the model maps (depth 2, normal
    (0, 0, -1)), std, ms the constant std planes of the frame and the model, sl, ml the luminance planes, K [B,4], T_true [B,12] float64."""
    H, W = I.GRID
    pred, sl, ml, Tt = [], [], [], []
    for b in range(I.B):
        fx, fy, cx, cy = I.K_GRID[b]
        T = wall_motion(b)
        Rm, t = I.mat(T)
        rays = np.stack(np.broadcast_arrays(((np.arange(W) - cx) / fx)[None, :], ((np.arange(H) - cy) / fy)[:, None], 1.0), -1)
        d = (WALL_Z - t[2]) / (rays @ Rm[2])                                          # (R (d ray) + t).z = WALL_Z
        pred.append(d)
        sl.append(albedo((rays * d[..., None]) @ Rm.T + t, WALL_WAVES))               # the texture lives in the model camera's frame
        ml.append(albedo(rays * WALL_Z, WALL_WAVES))
        Tt.append(T)
    n = np.zeros((I.B, H, W, 3), np.float32)
    n[..., 2] = -1.0
    out = dict(pred=np.stack(pred).astype(np.float32), md=np.full((I.B, H, W), WALL_Z, np.float32), mn=n,
               std=np.full((I.B, H, W), FRAME_STD, np.float32), ms=np.full((I.B, H, W), MODEL_STD, np.float32), sl=np.stack(sl).astype(np.float32),
               ml=np.stack(ml).astype(np.float32), K=np.array(I.K_GRID, np.float32), T_true=np.stack(Tt))
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def wall_reference(image=True):
    """The float64 restatement on the wall from the identity, WALL_ITERS iterations: per image (T, stats, (deg, m)).  Without the image
    it is `icp_ref.run`."""
    x = wall_inputs()
    H, W = I.GRID
    out = []
    for b in range(I.B):
        d = P.depth(x["pred"][b], H, W, 0, dt=np.float64)
        md, mn, s, ms = (x[k][b].astype(np.float64) for k in ("md", "mn", "std", "ms"))
        if image:
            T, st, _ = run(d, s, None, x["K"][b], md, mn, ms, x["K"][b], x["sl"][b].astype(np.float64), x["ml"][b].astype(np.float64),
                           iters=WALL_ITERS)
        else:
            T, st, _ = I.run(d, s, None, x["K"][b], md, mn, ms, x["K"][b], iters=WALL_ITERS)
        out.append((T, st, I.pose_error(T, x["T_true"][b])))
    return out


# ---- convergence on the painted scene ---------------------------------------------------------------------------------------------------------

CONVERGE_MOTION, CONVERGE_ITERS = 0, 12


@functools.lru_cache(maxsize=None)
def converge_lumas():
    """(sl, ml) [B,48,64] f32 of `icp_ref.converge_inputs(CONVERGE_MOTION)`."""
    x = I.converge_inputs(CONVERGE_MOTION)
    H, W = I.GRID
    sl = np.stack([tint_luma(render(I.K_GRID[b], I.current_pose(x["T_true"][b]), H, W)) for b in range(I.B)]).astype(np.float32)
    ml = np.stack([tint_luma(render(I.K_GRID[b], I.T_REF, H, W)) for b in range(I.B)]).astype(np.float32)
    sl.setflags(write=False)
    ml.setflags(write=False)
    return sl, ml


@functools.lru_cache(maxsize=None)
def converge_reference(stride):
    """The float64 restatement with the image from the identity, the depth weighted by the constant stds FRAME_STD and MODEL_STD: per
    image (T, stats, (deg, m))."""
    x = I.converge_inputs(CONVERGE_MOTION)
    sl, ml = converge_lumas()
    H, W = I.GRID
    out = []
    for b in range(I.B):
        d = P.depth(x["pred"][b], H, W, 0, dt=np.float64)
        T, st, _ = run(d, np.full((H, W), np.float64(np.float32(FRAME_STD))), None, x["K"][b], x["md"][b].astype(np.float64),
                       x["mn"][b].astype(np.float64), np.full((H, W), np.float64(np.float32(MODEL_STD))), x["K"][b],
                       sl[b].astype(np.float64), ml[b].astype(np.float64), iters=CONVERGE_ITERS, stride=stride)
        out.append((T, st, I.pose_error(T, x["T_true"][b])))
    return out


# ---- the Tracker's frames, painted -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def track_images():
    """Per frame of `icp_ref.track_frames` the normalised image [B,3,48,64] f32 of the painted scene -- read-only."""
    H, W = I.GRID
    out = []
    for f in range(I.TRACK_FRAMES):
        img = to_rgb(np.stack([render(I.K_GRID[b], I.track_pose(f, b), H, W) for b in range(I.B)]))
        img.setflags(write=False)
        out.append(img)
    return tuple(out)
