"""numpy restatement of the definitions of `cfp_tsdf_integrate_rgb`, `cfp_tsdf_shade` and `cfp_tsdf_surface_rgb` (include/cfpnet_hip.h) --
TEST INFRASTRUCTURE, on top of tsdf_ref.py and tsdf_surface_ref.py: their cases, frames, poses and states, no new volumes.

Written for two dtypes like those: float32 in the header's order of operations, what the GPU's colours are compared with, and float64,
which decides which voxels a step colours.  The geometry of a step is tsdf_ref.integrate itself, so everything said there about the
excluded set holds; colour adds one boundary, sdf = +trunc, and the voxels whose float64 sdf lies within SDF_BAND relative of it join the
excluded set (`step_excluded`).

The image is an analytic texture of the world point, rendered per frame at the scene's float64 hit point of every pixel of the 48 x 64
grid: on the wall a sum of sines of Xw and Yw, on the sphere one of Xw and Zw, each channel with its own frequencies.  Both functions are
defined in all of space and are Lipschitz there with the constant LIPSCHITZ[k] (amplitude times the length of the frequency vector),
which is what the end-to-end bound of test_tsdf_color_abi.py rests on.  The image is then normalised with MEAN / CSTD, neither trivial, so
that c = x * cstd + mean is exercised; frame 0 / image 2 carries a NaN patch in channel 1.  A second image kind (`pix_image`) holds
(pix + 1) / (H W) in channel 0: on an empty volume the colour a voxel takes is the pixel it read."""
import functools

import numpy as np

import tsdf_ref as S
import tsdf_surface_ref as S2

RTOL = S.RTOL
SDF_BAND = S.SDF_BAND
MAX_EXCLUDED = S.MAX_EXCLUDED
MEAN = (0.41, 0.52, 0.36)
CSTD = (0.27, 0.19, 0.31)
NAN_PATCH = (2, 1, slice(18, 26), slice(28, 40))      # image, channel, rows, columns of frame 0: in the middle of the volume's footprint

# c_k = 0.5 + AMP * (sin(f0 * a + p0) + sin(f1 * b + p1)) with (a, b) = (Xw, Yw) on the wall and (Xw, Zw) on the sphere, in 0.1 .. 0.9
AMP = 0.2
WALL_TEX = (((1.3, 0.2), (1.7, 1.1)), ((0.9, 2.0), (1.4, 0.3)), ((1.6, 4.0), (0.8, 2.5)))          # per channel ((f0, p0), (f1, p1)), rad / m
SPHERE_TEX = (((1.5, 1.0), (1.1, 3.0)), ((1.2, 0.5), (1.8, 2.2)), ((0.7, 5.0), (1.6, 0.9)))
LIPSCHITZ = tuple(AMP * max(float(np.hypot(w[0][0], w[1][0])), float(np.hypot(s[0][0], s[1][0]))) for w, s in zip(WALL_TEX, SPHERE_TEX))
WALL, SPHERE, NOTHING = 0, 1, -1


def texture(P, label):
    """The colour [..., 3] (float64) of the surface `label` (WALL / SPHERE, broadcast) at the world points P [..., 3]: smooth functions of
    the whole space, so a point need not lie on the surface."""
    P = np.asarray(P, np.float64)
    out = np.empty(P.shape[:-1] + (3,))
    for k in range(3):
        (wf0, wp0), (wf1, wp1) = WALL_TEX[k]
        (sf0, sp0), (sf1, sp1) = SPHERE_TEX[k]
        wall = 0.5 + AMP * (np.sin(wf0 * P[..., 0] + wp0) + np.sin(wf1 * P[..., 1] + wp1))
        sph = 0.5 + AMP * (np.sin(sf0 * P[..., 0] + sp0) + np.sin(sf1 * P[..., 2] + sp1))
        out[..., k] = np.where(np.asarray(label) == SPHERE, sph, wall)
    return out


def label_of(P):
    """WALL or SPHERE: the surface of tsdf_ref's scene a world point is nearer to."""
    P = np.asarray(P, np.float64)
    wall = np.abs(P @ S.WALL_N - S.WALL_C)
    sph = np.abs(np.linalg.norm(P - S.SPHERE_C, axis=-1) - S.SPHERE_R)
    return np.where(sph < wall, SPHERE, WALL)


def nearest_scene_point(P):
    """The nearest point of the scene's nearer surface, float64."""
    P = np.asarray(P, np.float64)
    on_wall = P - (P @ S.WALL_N - S.WALL_C)[..., None] * S.WALL_N
    v = P - S.SPHERE_C
    on_sph = S.SPHERE_C + S.SPHERE_R * v / np.linalg.norm(v, axis=-1, keepdims=True)
    return np.where((label_of(P) == SPHERE)[..., None], on_sph, on_wall)


@functools.lru_cache(maxsize=None)
def render(f, b):
    """(colour [3,H,W] float64 in 0..1, label [H,W]) of image b of frame f: the texture at the float64 hit point of every grid pixel."""
    H, W = S.GRID
    K, T = S.K_GRID[b], S.POSES[f][b]
    d = S.scene_depth(K, T, np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    fx, fy, cx, cy = (float(np.float32(v)) for v in K)
    M = np.asarray(T, np.float64).reshape(3, 4)
    rays = np.stack(np.broadcast_arrays(((np.arange(W) - cx) / fx)[None, :], ((np.arange(H) - cy) / fy)[:, None], 1.0), -1)
    Pw = (rays * d[..., None] - M[:, 3]) @ M[:, :3]                                    # R^T (r d - t)
    assert np.isfinite(Pw).all() and S2.scene_distance(Pw).max() < 1e-9
    lab = label_of(Pw)
    c = np.moveaxis(texture(Pw, lab), -1, 0)
    assert c.min() >= 0.1 - 1e-12 and c.max() <= 0.9 + 1e-12
    for a in (c, lab):
        a.setflags(write=False)
    return c, lab


@functools.lru_cache(maxsize=None)
def images():
    """Per frame the normalised image [B,3,H,W] f32 -- read-only; the same for every case, they share the grid, cameras and poses."""
    m, s = (np.array(v, np.float32).astype(np.float64)[:, None, None] for v in (MEAN, CSTD))
    out = []
    for f in range(len(S.POSES)):
        img = np.stack([((render(f, b)[0] - m) / s) for b in range(S.B)]).astype(np.float32)
        if f == 0:
            b, k, rows, cols = NAN_PATCH
            img[b, k, rows, cols] = np.nan
        img.setflags(write=False)
        out.append(img)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pix_image():
    """[B,3,H,W] f32: channel 0 is (pix + 1) / (H W), the others constants -- for mean 0, std 1 and an EMPTY volume only."""
    H, W = S.GRID
    img = np.empty((S.B, 3, H, W), np.float32)
    img[:, 0] = ((np.arange(H * W, dtype=np.float64) + 1.0) / (H * W)).astype(np.float32).reshape(H, W)
    img[:, 1], img[:, 2] = 0.25, 0.75
    img.setflags(write=False)
    return img


def pix_of(c0):
    """The pixel a colour of `pix_image` names."""
    H, W = S.GRID
    return np.rint(np.asarray(c0, np.float64) * (H * W)).astype(np.int64) - 1


# ---- integrate ---------------------------------------------------------------------------------------------------------------------------

def empty_color(dims, dt=np.float32):
    Dx, Dy, Dz = dims
    return np.zeros((Dz, Dy, Dx, 4), dt)


def integrate_rgb(vol, col, d, s, img, mean, cstd, K, T, dims, origin, voxel, trunc, std_floor=S.STD_FLOOR, w_max=S.F32_MAX):
    """tsdf_ref.integrate, then the colour step: col [Dz,Dy,Dx,4] and img [3,H,W] in vol's dtype -> the dict of tsdf_ref.integrate plus
    col (new) and coloured [Dz,Dy,Dx] bool."""
    dt = vol.dtype.type
    assert col.dtype == vol.dtype and img.dtype == vol.dtype
    r = S.integrate(vol, d, s, K, T, dims, origin, voxel, trunc, std_floor=std_floor, w_max=w_max)
    pix = np.where(r["pix"] >= 0, r["pix"], 0)
    tr, sf0, wm = (dt(np.float32(x)) for x in (trunc, std_floor, w_max))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if s is None:
            w = np.ones(pix.shape, dt)
        else:
            sv = s.ravel()[pix]
            sf = np.where(sv > sf0, sv, sf0)
            w = dt(1) / (sf * sf)
        band = r["updated"] & ~(r["sdf"] > tr)
        c = [img[k].ravel()[pix] * dt(np.float32(cstd[k])) + dt(np.float32(mean[k])) for k in range(3)]
        coloured = band & np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2])
        Wc = col[..., 3]
        tot = Wc + w
        new = [(col[..., k] * Wc + c[k] * w) / tot for k in range(3)] + [np.minimum(tot, wm)]
    out = col.copy()
    for k in range(4):
        out[..., k] = np.where(coloured, new[k], col[..., k])
    assert out.dtype == vol.dtype
    r.update(col=out, coloured=coloured, band=band)
    return r


def counts_of(r, keep=None):
    k = np.ones(r["seen"].shape, bool) if keep is None else keep
    return S.counts_of(r, keep) + [int((r["coloured"] & k).sum())]


def _step(name, f, b, col, dt):
    c = S.TSDF_CASES[name]
    d, s = S.grids(name, f, b, dt)
    return integrate_rgb(S.states(name)[f][b].astype(dt), col.astype(dt), d, s, images()[f][b].astype(dt), MEAN, CSTD, S.K_GRID[b],
                         S.frames(name)[f][2][b], S.DIMS, c["origin"], S.VOXEL, S.TRUNC, w_max=S.w_max_of(c))


@functools.lru_cache(maxsize=None)
def color_states(name):
    """The float32 restatement's colour volumes [B,Dz,Dy,Dx,4] before frame 0, 1, 2 and after the last, next to tsdf_ref.states(name) --
    read-only."""
    cols = [np.stack([empty_color(S.DIMS) for _ in range(S.B)])]
    for f in range(len(S.POSES)):
        cols.append(np.stack([_step(name, f, b, cols[-1][b], np.float32)["col"] for b in range(S.B)]))
    for v in cols:
        v.setflags(write=False)
    return tuple(cols)


@functools.lru_cache(maxsize=None)
def step_reference(name, f, b, dt=np.float32):
    """The dict of `integrate_rgb` for image b of frame f in dt, started from the common float32 states -- read-only, shared."""
    return _step(name, f, b, color_states(name)[f][b], dt)


@functools.lru_cache(maxsize=None)
def step_excluded(name, f, b):
    """[Dz,Dy,Dx] bool: tsdf_ref.step_excluded plus the voxels whose float64 sdf lies within SDF_BAND relative of +trunc."""
    r = S.step_reference(name, f, b, np.float64)
    tr = float(np.float32(S.TRUNC))
    with np.errstate(invalid="ignore"):
        band = r["seen"] & (np.abs(r["sdf"] - tr) <= SDF_BAND * tr)
    return S.step_excluded(name, f, b) | band


@functools.lru_cache(maxsize=None)
def final_color64(name):
    """[B,Dz,Dy,Dx,4] float64: the colour chain carried in float64 over the three frames (the geometry of every step starts from the common
    float32 state, like everything in tsdf_ref.py) -- what the end-to-end check looks at."""
    col = np.stack([empty_color(S.DIMS, np.float64) for _ in range(S.B)])
    for f in range(len(S.POSES)):
        col = np.stack([_step(name, f, b, col[b], np.float64)["col"] for b in range(S.B)])
    col.setflags(write=False)
    return col


# ---- shade -------------------------------------------------------------------------------------------------------------------------------

def shade(col, K, T, depth, origin, voxel):
    """col [Dz,Dy,Dx,4] in its dtype, depth [Hd,Wd] -> rgb [Hd,Wd,3] in that dtype, NaN where the map has no colour."""
    dt = col.dtype.type
    Dz, Dy, Dx = col.shape[:3]
    Hd, Wd = depth.shape
    fx, fy, cx, cy = (dt(np.float32(v)) for v in K)
    t = [dt(np.float32(v)) for v in np.asarray(T).ravel()[:12]]
    org = [dt(np.float32(v)) for v in origin]
    vx = dt(np.float32(voxel))
    dep = depth.astype(dt)
    rx = np.broadcast_to(((np.arange(Wd).astype(dt) - cx) / fx)[None, :], (Hd, Wd))
    ry = np.broadcast_to(((np.arange(Hd).astype(dt) - cy) / fy)[:, None], (Hd, Wd))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        gx, gy, gz = S._ray_point(rx, ry, t, dep, org, vx)
        x0, y0, z0 = np.floor(gx), np.floor(gy), np.floor(gz)
        ok = np.isfinite(dep) & (x0 >= 0) & (x0 <= Dx - 2) & (y0 >= 0) & (y0 <= Dy - 2) & (z0 >= 0) & (z0 <= Dz - 2)
        i, j, k = (np.where(ok, a, 0).astype(np.int64) for a in (x0, y0, z0))
        a, b, c = gx - x0, gy - y0, gz - z0
        wx, wy, wz = (dt(1) - a, a), (dt(1) - b, b), (dt(1) - c, c)
        den = np.zeros((Hd, Wd), dt)
        num = [np.zeros((Hd, Wd), dt) for _ in range(3)]
        anyc = np.zeros((Hd, Wd), bool)
        for dk in (0, 1):
            for dj in (0, 1):
                for di in (0, 1):                     # x fastest
                    v = col[np.minimum(k + dk, Dz - 1), np.minimum(j + dj, Dy - 1), np.minimum(i + di, Dx - 1)]
                    tw = (wx[di] * wy[dj]) * wz[dk]
                    has = ok & (v[..., 3] > 0)
                    anyc |= has
                    den = np.where(has, den + tw, den)
                    for ch in range(3):
                        num[ch] = np.where(has, num[ch] + tw * v[..., ch], num[ch])
        out = np.stack([np.where(anyc, num[ch] / den, dt(np.nan)) for ch in range(3)], -1)
    assert out.dtype == col.dtype
    return out


# ---- surface colours ---------------------------------------------------------------------------------------------------------------------

def surface_rgb(vol, col, index):
    """vol [Dz,Dy,Dx,2], col [Dz,Dy,Dx,4] in one dtype, index [N] int (edge indices e) -> dict: colors [N,3] in that dtype (NaN rows:
    none), ends [N] int: how many ends of the edge have a colour (-1: e names no edge of the lattice)."""
    dt = vol.dtype.type
    Dz, Dy, Dx = vol.shape[:3]
    nvox = Dx * Dy * Dz
    e = np.asarray(index, np.int64)
    good = (e >= 0) & (e < 3 * nvox)
    es = np.where(good, e, 0)
    n, a = es // 3, es % 3
    k, r = n // (Dx * Dy), n % (Dx * Dy)
    j, i = r // Dx, r % Dx
    good &= np.where(a == 0, i + 1 < Dx, np.where(a == 1, j + 1 < Dy, k + 1 < Dz))
    q = np.where(good, n + np.where(a == 0, 1, np.where(a == 1, Dx, Dx * Dy)), 0)
    n = np.where(good, n, 0)
    F, C = vol.reshape(-1, 2)[:, 0], col.reshape(-1, 4)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        fp, fq = F[n], F[q]
        t = fp / (fp - fq)
        h = dt(1) - t
        cp, cq = C[n], C[q]
        hp, hq = good & (cp[:, 3] > 0), good & (cq[:, 3] > 0)
        both = h[:, None] * cp[:, :3] + t[:, None] * cq[:, :3]
        out = np.where((hp & hq)[:, None], both, np.where(hp[:, None], cp[:, :3], np.where(hq[:, None], cq[:, :3], dt(np.nan))))
    out = out.astype(dt)
    return dict(colors=out, ends=np.where(good, hp.astype(np.int64) + hq.astype(np.int64), -1))


@functools.lru_cache(maxsize=None)
def surface_reference(name, b, w_min=0.0, max_jump=np.inf, dt=np.float32):
    """The dict of `surface_rgb` for the rows of tsdf_surface_ref.reference(name, b, ...) on the float32 final states, in dt."""
    idx = S2.reference(name, b, w_min, max_jump)["index"]                              # float32 decides the rows, as on the GPU
    return surface_rgb(S.states(name)[-1][b].astype(dt), color_states(name)[-1][b].astype(dt), idx)


close = S.close
