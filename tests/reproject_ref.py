"""numpy restatement of the definitions of `cfp_depth_reproject` and `cfp_depth_fuse` (include/cfpnet_hip.h) -- TEST INFRASTRUCTURE.

Written for two dtypes: float32 with the header's order of operations (numpy rounds every float32 operation once, like the library built
without fused multiply-adds) -- what the GPU's depths, planes and fused values are compared with -- and float64, which decides the
discrete results (which source wins a target pixel, which row of the fusion table a pixel takes).  A discrete result can differ between
the float32 kernel and the float64 reference only where a value lies next to a boundary; `GUARD` (four times the worst distance between
the float32 and the float64 projections over these very inputs, measured in test_reproject_abi.py) and the relative bands below say how
near, and the target pixels such a source can reach are excluded from the exact comparisons -- at most 1 % of a case's pixels, asserted on
the CPU.  Also the inputs the GPU tests use, so that the CPU tests can examine the same tensors."""
import functools

import numpy as np

import pointcloud_ref as P
from cfpnet_amd import synthetic

RTOL = P.RTOL            # 2e-5, tests/test_metrics.py
LO, HI = P.LO, P.HI
Z_NEAR = 1e-3
Z_TIE = 1e-5             # two sources competing for a pixel within this relative distance in Z': the winner is not compared
GATE_BAND = 1e-4         # a pixel within this relative distance of the fusion gate: its row of the table is not compared
MAX_EXCLUDED = 0.01      # share of a case's target pixels the exact comparisons may leave out
GUARD_MEASURED = None    # pixels; set by guard_measured()


# ---- reproject -----------------------------------------------------------------------------------------------------------------------------

def project(d, K, T, Kd, z_near=Z_NEAR):
    """d [H,W] in its dtype -> (ok [H,W] bool, Z' [H,W], u [H,W], v [H,W]) in that dtype, the header's order of operations."""
    dt = d.dtype.type
    H, W = d.shape
    fx, fy, cx, cy = (dt(np.float32(v)) for v in K)
    t = [dt(np.float32(v)) for v in np.asarray(T).ravel()[:12]]
    gx, gy, hx, hy = (dt(np.float32(v)) for v in Kd)
    x = np.arange(W).astype(dt)[None, :]
    y = np.arange(H).astype(dt)[:, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        X = (x - cx) / fx * d
        Y = (y - cy) / fy * d
        Z = d
        Xp = (t[0] * X + t[1] * Y) + t[2] * Z + t[3]
        Yp = (t[4] * X + t[5] * Y) + t[6] * Z + t[7]
        Zp = (t[8] * X + t[9] * Y) + t[10] * Z + t[11]
        ok = np.isfinite(d) & (d > 0) & np.isfinite(Zp) & (Zp >= dt(np.float32(z_near)))
        u = gx * (Xp / Zp) + hx
        v = gy * (Yp / Zp) + hy
    assert Zp.dtype == d.dtype and u.dtype == d.dtype
    return ok, Zp, u, v


def _targets(u, v, splat):
    """The (column, row) float arrays a source hits: one pair for splat 1, four for splat 2."""
    dt = u.dtype.type
    with np.errstate(invalid="ignore"):
        if splat == 1:
            return [(np.floor(u + dt(0.5)), np.floor(v + dt(0.5)))]
        u0, v0 = np.floor(u), np.floor(v)
        return [(u0, v0), (u0 + dt(1), v0), (u0, v0 + dt(1)), (u0 + dt(1), v0 + dt(1))]


def _hits(ok, Zp, u, v, Hd, Wd, splat):
    """-> (target pixel index, Z', source index) of every hit inside the Hd x Wd grid, one row per hit."""
    src = np.arange(ok.size).reshape(ok.shape)
    tg, zz, ss = [], [], []
    for col, row in _targets(u, v, splat):
        with np.errstate(invalid="ignore"):
            inside = ok & (col >= 0) & (col < Wd) & (row >= 0) & (row < Hd)          # on the float values; NaN fails
        tg.append(row[inside].astype(np.int64) * Wd + col[inside].astype(np.int64))
        zz.append(Zp[inside])
        ss.append(src[inside])
    return np.concatenate(tg), np.concatenate(zz), np.concatenate(ss)


def zbuffer(ok, Zp, u, v, Hd, Wd, splat):
    """-> (depth [Hd,Wd] in Zp's dtype, NaN where nothing lands; index [Hd,Wd] int32, -1 there; tie [Hd,Wd] bool: the runner-up of the
    pixel is within Z_TIE relative of the winner).  The nearest wins, a tie in depth goes to the lowest source index."""
    tg, zz, ss = _hits(ok, Zp, u, v, Hd, Wd, splat)
    order = np.lexsort((ss, zz, tg))
    tg, zz, ss = tg[order], zz[order], ss[order]
    first = np.ones(tg.size, bool)
    first[1:] = tg[1:] != tg[:-1]
    depth = np.full(Hd * Wd, np.nan, Zp.dtype)
    index = np.full(Hd * Wd, -1, np.int32)
    depth[tg[first]] = zz[first]
    index[tg[first]] = ss[first]
    tie = np.zeros(Hd * Wd, bool)
    second = ~first
    second[1:] &= first[:-1]                                                          # the runner-up follows the winner
    if second.any():
        w = zz[np.flatnonzero(second) - 1].astype(np.float64)
        r = zz[second].astype(np.float64)
        tie[tg[second]] = (r - w) <= Z_TIE * w
    return depth.reshape(Hd, Wd), index.reshape(Hd, Wd), tie.reshape(Hd, Wd)


def ambiguous_targets(ok, Zp, u, v, Hd, Wd, splat, guard, z_near=Z_NEAR):
    """[Hd,Wd] bool: the target pixels whose hit by some source depends on a rounding that float32 and float64 may make differently --
    u or v within `guard` pixels of a rounding boundary (for splat 1 the half-integers, both neighbours can be hit; for splat 2 the
    integers, the columns n - 1 and n + 1 are hit or not) -- plus everything a source whose Z' lies within Z_TIE relative of z_near can
    reach.  Float64 inputs."""
    out = np.zeros((Hd, Wd), bool)
    shift = 0.5 if splat == 1 else 0.0
    with np.errstate(invalid="ignore"):
        nu, nv = np.rint(u + shift), np.rint(v + shift)                               # the nearest boundary, as an integer
        au, av = ok & (np.abs(u + shift - nu) < guard), ok & (np.abs(v + shift - nv) < guard)
        near = ok & (np.abs(Zp - z_near) <= Z_TIE * z_near)
        cols = [np.floor(u + shift) + k for k in range(splat)]
        rows = [np.floor(v + shift) + k for k in range(splat)]

    def mark(sel, cs, rs):
        for c in cs:
            for r in rs:
                with np.errstate(invalid="ignore"):
                    inside = sel & (c >= 0) & (c < Wd) & (r >= 0) & (r < Hd)
                out[r[inside].astype(np.int64), c[inside].astype(np.int64)] = True

    side = [nu - 1, nu] if splat == 1 else [nu - 1, nu + 1]
    mark(au, side, rows)
    side_v = [nv - 1, nv] if splat == 1 else [nv - 1, nv + 1]
    mark(av, cols, side_v)
    mark(au & av, side, side_v)
    mark(near, cols, rows)
    return out


# name: source prediction size, source grid, interpolate, target grid, images, splat, source / target intrinsics and pose per image
_ID = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)


def _rot(ax, ay, az, t):
    """[R|t] row-major, R = Rz Ry Rx (radians), as 12 float32-representable numbers."""
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ \
        np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return tuple(float(np.float32(v)) for v in np.concatenate([R, np.array(t, np.float64)[:, None]], 1).ravel())


K_SMALL = ((40.0, 41.5, 25.3, 17.9), (35.5, 36.25, 26.0, 18.0), (48.0, 47.0, 20.5, 22.75))      # per image, for the 37 x 53 grid

# Every pose keeps Z' away from 0 for the depths of these inputs (t_z >= 0, no rotation that turns a visible ray sideways): a point whose Z'
# cancels to nearly nothing projects with a large float32 error, which would only inflate GUARD for every other case.
REPROJECT_CASES = {
    "odd_19x27_to_37x53": dict(h=19, w=27, H=37, W=53, interp=1, Hd=37, Wd=53, splat=1, K=K_SMALL, Kd=K_SMALL,
                               T=(_rot(0.01, -0.02, 0.005, (0.03, -0.02, 0.05)), _rot(-0.015, 0.01, 0.0, (-0.04, 0.01, 0.03)),
                                  _rot(0.0, 0.02, -0.01, (0.02, 0.03, 0.02)))),
    "odd_splat2": dict(h=19, w=27, H=37, W=53, interp=1, Hd=37, Wd=53, splat=2, K=K_SMALL, Kd=K_SMALL,
                       T=(_rot(0.01, -0.02, 0.005, (0.03, -0.02, 0.05)), _rot(-0.015, 0.01, 0.0, (-0.04, 0.01, 0.0)),
                          _rot(0.0, 0.02, -0.01, (0.02, 0.03, 0.02)))),
    "same_24x40_direct": dict(h=24, w=40, H=24, W=40, interp=0, Hd=24, Wd=40, splat=1, K=((30.0, 31.0, 19.5, 11.5),),
                              Kd=((30.0, 31.0, 19.5, 11.5),), T=(_rot(0.02, 0.015, -0.01, (-0.05, 0.02, 0.04)),)),
    "register_37x53_to_29x61": dict(h=19, w=27, H=37, W=53, interp=1, Hd=29, Wd=61, splat=2, K=((40.0, 41.5, 25.3, 17.9),),
                                    Kd=((44.0, 30.5, 30.2, 14.1),), T=(_rot(0.0, 0.01, 0.0, (0.06, -0.01, 0.0)),)),
    "leaves_the_frame": dict(h=24, w=40, H=24, W=40, interp=0, Hd=24, Wd=40, splat=1, K=((30.0, 31.0, 19.5, 11.5),),
                             Kd=((30.0, 31.0, 19.5, 11.5),), T=(_rot(0.0, -0.9, 0.0, (0.3, 0.0, 0.0)),)),
    "two_planes_occlusion": dict(h=32, w=48, H=32, W=48, interp=0, Hd=32, Wd=48, splat=1, K=((40.0, 40.0, 23.5, 15.5),),
                                 Kd=((40.0, 40.0, 23.5, 15.5),), T=(_ID[:3] + (0.305,) + _ID[4:],)),
    "full_240x320_to_480x640": dict(h=240, w=320, H=480, W=640, interp=1, Hd=480, Wd=640, splat=1, K=(P.ZJUL5,), Kd=(P.ZJUL5,),
                                    T=(_rot(0.004, -0.006, 0.003, (0.004, -0.002, 0.003)),)),
}
PLANES_NEAR, PLANES_FAR = 1.0, 2.0                    # the occlusion case: the near plane covers columns 16 .. 31 of the source
IDENTITY = _ID


@functools.lru_cache(maxsize=None)
def reproject_inputs(name):
    """(pred [B,h,w] f32, K [B,4], T [B,12], Kd [B,4], plane [B,h,w] f32: a std map that travels with the depth) -- read-only."""
    c = REPROJECT_CASES[name]
    h, w, H, W = c["h"], c["w"], c["H"], c["W"]
    B = len(c["K"])
    if name == "two_planes_occlusion":
        pred = np.full((1, h, w), PLANES_FAR, np.float32)
        pred[:, :, 16:32] = PLANES_NEAR
    elif h == 240:
        # No clipped outliers here, and a small translation: the float32 source coordinate of the protocol's blend is off by up to an ulp
        # of 319, which moves a depth by 3e-5 of the local contrast; next to a pixel clipped to 10 m that shifts u by milli-pixels under
        # a translation, and GUARD -- one constant for all cases -- would exclude far more than 1 % of the pixels.
        rng = np.random.default_rng(73)
        pred = (synthetic.make_depth(h, w, seed=73) * np.exp(rng.normal(0.0, 0.02, (h, w))))[None].astype(np.float32)
    else:
        seed = {19: 71, 24: 72}[h]
        pred = np.stack([synthetic.make_eval_pair(H, W, h, w, seed + 10 * b, 0.0, 0.02)[1] for b in range(B)])
        if B == 3:                                    # the batched cases carry a NaN / Inf patch in one image
            pred[2, 2:5, 3:6] = np.nan
            pred[2, 9:11, 20:23] = np.inf
            pred[2, 14:17, 8:10] = -np.inf
    rng = np.random.default_rng(900 + h)
    plane = (0.02 + 0.1 * rng.random((B, h, w))).astype(np.float32)
    out = (np.ascontiguousarray(pred, np.float32), np.array(c["K"], np.float32), np.array(c["T"], np.float32), np.array(c["Kd"], np.float32),
           plane)
    assert out[1].shape == (B, 4) and out[2].shape == (B, 12) and out[3].shape == (B, 4)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def projections(name, dt=np.float32):
    """Per image (ok, Z', u, v) of the case in dt -- read-only, shared."""
    c = REPROJECT_CASES[name]
    pred, K, T, Kd, _ = reproject_inputs(name)
    return [project(P.depth(pred[b], c["H"], c["W"], c["interp"], dt=dt), K[b], T[b], Kd[b]) for b in range(pred.shape[0])]


@functools.lru_cache(maxsize=None)
def reproject_reference(name, dt=np.float32, splat=None):
    """(depth [B,Hd,Wd] in dt, index [B,Hd,Wd] i32, plane [B,Hd,Wd] in dt, tie [B,Hd,Wd] bool) -- read-only, shared by the tests."""
    c = REPROJECT_CASES[name]
    splat = splat or c["splat"]
    plane = reproject_inputs(name)[4]
    ds, ix, pl, ti = [], [], [], []
    for b, (ok, Zp, u, v) in enumerate(projections(name, dt)):
        d, i, t = zbuffer(ok, Zp, u, v, c["Hd"], c["Wd"], splat)
        grid = P.plane_to_grid(plane[b], c["H"], c["W"], dt).ravel()
        ds.append(d); ix.append(i); ti.append(t)
        pl.append(np.where(i >= 0, grid[np.maximum(i, 0)], dt(np.nan)).astype(dt))
    out = (np.stack(ds), np.stack(ix), np.stack(pl), np.stack(ti))
    for a in out:
        a.setflags(write=False)
    return out


def guard_measured():
    """GUARD: 4 x the worst |u32 - u64| and |v32 - v64| in pixels over every source of every case that both restatements project and
    whose projection lies within a pixel of the target grid (a point far outside cannot reach a pixel whichever way it is rounded)."""
    global GUARD_MEASURED
    if GUARD_MEASURED is None:
        worst = 0.0
        for name, c in REPROJECT_CASES.items():
            for (ok32, _, u32, v32), (ok64, _, u64, v64) in zip(projections(name), projections(name, np.float64)):
                sel = ok32 & ok64 & (u64 > -2) & (u64 < c["Wd"] + 1) & (v64 > -2) & (v64 < c["Hd"] + 1)
                if sel.any():
                    worst = max(worst, float(np.abs(u32[sel] - u64[sel]).max()), float(np.abs(v32[sel] - v64[sel]).max()))
        GUARD_MEASURED = 4.0 * worst
    return GUARD_MEASURED


@functools.lru_cache(maxsize=None)
def reproject_excluded(name, splat=None):
    """[B,Hd,Wd] bool: the target pixels left out of the exact comparisons of the case (float64 projections, GUARD, Z' ties)."""
    c = REPROJECT_CASES[name]
    splat = splat or c["splat"]
    tie = reproject_reference(name, np.float64, splat)[3]
    amb = np.stack([ambiguous_targets(ok, Zp, u, v, c["Hd"], c["Wd"], splat, guard_measured())
                    for ok, Zp, u, v in projections(name, np.float64)])
    out = tie | amb
    out.setflags(write=False)
    return out


# ---- fuse ----------------------------------------------------------------------------------------------------------------------------------

ROWS = ("current_only", "filled", "neither", "rejected", "fused")      # the rows of the header's table, in its order


def fuse(c, s, p, vp0, process_var, gate_k, gate_abs, std_floor):
    """c, s, p, vp0 [H,W] in one dtype (current depth, current std, prior depth, prior variance on the same grid) -> dict with
    depth, var [H,W], row [H,W] int (index into ROWS), gate_margin [H,W] float64 (|  |p - c| - gate | / gate where both are present, inf
    elsewhere), terms (|p - c|, (p - c)^2 in the dtype, at the pixels where both are present)."""
    dt = c.dtype.type
    pv, gk, ga, sf = (dt(np.float32(v)) for v in (process_var, gate_k, gate_abs, std_floor))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        sd = np.where(s > sf, s, sf)
        vc = sd * sd
        present = np.isfinite(p) & np.isfinite(vp0)
        cf = np.isfinite(c)
        vp = vp0 + pv
        diff = p - c
        ad = np.abs(diff)
        tot = vc + vp
        gate = gk * np.sqrt(tot) + ga
        both = present & cf
        rej = both & (ad > gate)
        fus = both & ~rej
        w = vc / tot
        depth = np.where(cf, c, dt(np.nan))
        var = np.where(cf, vc, dt(np.inf))
        depth = np.where(present & ~cf, p, depth)
        var = np.where(present & ~cf, vp, var)
        depth = np.where(fus, c + w * diff, depth)
        var = np.where(fus, (vc * vp) / tot, var)
        margin = np.where(both, np.abs(ad.astype(np.float64) - gate) / np.maximum(gate.astype(np.float64), 1e-30), np.inf)
    row = np.select([rej, fus, present & ~cf, ~present & cf], [3, 4, 1, 0], 2)
    assert depth.dtype == c.dtype and var.dtype == c.dtype
    return dict(depth=depth, var=var, row=row, gate_margin=margin, abs=ad[both], sq=(diff * diff)[both], present=present)


def counts_of(row, present, keep=None):
    """(prior present, fused, rejected, filled) over the pixels of `keep` (all by default)."""
    k = np.ones(row.shape, bool) if keep is None else keep
    return [int((present & k).sum()), int(((row == 4) & k).sum()), int(((row == 3) & k).sum()), int(((row == 1) & k).sum())]


FUSE_NUMBERS = dict(process_sigma=0.02, gate_k=3.0, gate_abs=0.05, std_floor=1e-3)
# name: the reproject case whose warped depth / plane is the prior (the plane squared is its variance), and the size of the current frame
FUSE_CASES = {
    "odd_half_res": dict(prior="odd_splat2", h=19, w=27),
    "same_size": dict(prior="same_24x40_direct", h=24, w=40),
    "full": dict(prior="full_240x320_to_480x640", h=240, w=320),
}


@functools.lru_cache(maxsize=None)
def fuse_inputs(name):
    """(cur [B,h,w] f32, cur_std [B,h,w] f32, prior_depth [B,H,W] f32, prior_var [B,H,W] f32) -- read-only.  The prior is the float32
    reference of a reproject case (so it has holes where nothing landed); the current frame is the prior's own source prediction,
    slightly rescaled so that most pixels fuse, with a band moved beyond the gate (rejected) and a NaN patch (filled, or neither where
    the prior has a hole too)."""
    c = FUSE_CASES[name]
    rc = REPROJECT_CASES[c["prior"]]
    h, w = c["h"], c["w"]
    depth, _, plane, _ = reproject_reference(c["prior"])
    pred = reproject_inputs(c["prior"])[0]
    B = pred.shape[0]
    rng = np.random.default_rng(4000 + h)
    cur = (np.nan_to_num(pred, nan=1.5, posinf=HI, neginf=LO) * (1.0 + rng.normal(0.0, 0.004, pred.shape))).astype(np.float32)
    cur[:, h // 3:h // 3 + max(h // 8, 2), :] += np.float32(0.8)                      # a band where the scene changed
    cur[:, -max(h // 5, 3):, :max(w // 4, 3)] = np.nan                                # the model has nothing here
    std = (0.02 + 0.05 * rng.random((B, h, w))).astype(np.float32)
    std[:, 0, :3] = 0.0                                                               # below the floor
    if B > 1:
        std[1, 1, :2] = np.nan                                                        # a NaN std takes the floor
    prior_depth = depth.copy()
    prior_var = (plane * plane).astype(np.float32)
    assert rc["Hd"] == rc["H"] and rc["Wd"] == rc["W"]
    out = (cur, std, prior_depth, prior_var)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fuse_reference(name, dt=np.float32):
    """Per image the dict of `fuse` in dt -- read-only."""
    c = FUSE_CASES[name]
    rc = REPROJECT_CASES[c["prior"]]
    cur, std, pd, pvar = fuse_inputs(name)
    H, W = rc["H"], rc["W"]
    interp = int((c["h"], c["w"]) != (H, W))
    n = FUSE_NUMBERS
    res = []
    for b in range(cur.shape[0]):
        cg = P.depth(cur[b], H, W, interp, dt=dt)
        sg = P.plane_to_grid(std[b], H, W, dt)
        res.append(fuse(cg, sg, pd[b].astype(dt), pvar[b].astype(dt), np.float32(n["process_sigma"] * n["process_sigma"]), n["gate_k"],
                        n["gate_abs"], n["std_floor"]))
    return res


def fuse_excluded(name):
    """Per image [H,W] bool: within GATE_BAND relative of the gate in the float64 reference."""
    return [r["gate_margin"] <= GATE_BAND for r in fuse_reference(name, np.float64)]


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------------

def close(got, want, what="", keep=None):
    """The project's bound |got - want| <= RTOL * max(|want|, 1e-3) against the float32 restatement over `keep` (all by default); NaN and
    infinities at exactly the same places.  Returns the worst ratio to the bound."""
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape, got.dtype)
    k = np.ones(got.shape, bool) if keep is None else keep
    g, w = got[k], want[k]
    assert np.array_equal(np.isnan(g), np.isnan(w)), what
    inf = np.isinf(w)
    assert np.array_equal(g[inf], w[inf]) and np.array_equal(np.isinf(g), inf), what
    fin = np.isfinite(w)
    g, w = g[fin].astype(np.float64), w[fin].astype(np.float64)
    ratio = np.abs(g - w) / (RTOL * np.maximum(np.abs(w), 1e-3))
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{what}: worst |got - want| / bound = {worst:.3e} over {g.size} values, {int(np.isnan(want[k]).sum())} NaN")
    assert worst <= 1.0, (what, worst)
    return worst
