"""numpy restatement of the definition of `cfp_tsdf_surface` (include/cfpnet_hip.h) -- TEST INFRASTRUCTURE.

Written for two dtypes: float32 with the header's order of operations (numpy rounds every float32 operation once, like the library built
without fused multiply-adds) and float64.  Unlike the integrate and raycast restatements (tsdf_ref.py) nothing is excluded anywhere: which
edges are kept, and in which order, is decided by comparisons of float32 values already in memory and by one correctly rounded float32
subtraction, so the GPU's counts and index lists are compared exactly with the float32 restatement.

Inputs: (a) the final states of three integrate cases of tsdf_ref.py (B = 3, 31 x 25 x 29) and (b) dense random volumes at the shapes that
put a crossing at the last lane of a wave, at a row end that is no wave end, in a wave that spans several rows, in the first and the last
chunk of 256 voxels, and in more chunks than the scan workgroup has threads."""
import functools

import numpy as np

import pointcloud_ref as P
import tsdf_ref as S

STATE_CASES = ("direct_48x64", "blend_24x32", "no_std")
JUMP = 2.0 * S.VOXEL / S.TRUNC                        # |F(p) - F(q)| of neighbours across a clean surface is voxel / trunc per axis unit
RANDOM_DIMS = ((1, 1, 1), (2, 1, 1), (1, 1, 2), (64, 1, 1), (65, 3, 2), (130, 5, 3), (67, 33, 31))
RANDOM_B = 2
RANDOM_ORIGIN, RANDOM_VOXEL = (-0.3317, 0.2141, 0.9073), 0.0213
W_MIN_BINDS = 450.0
ANGLE_TOL = 2e-5                                      # radians: the project's relative bound (tsdf_ref.RTOL) applied to a unit vector

close = S.close


def _shift(A, a, fill):
    """result[idx] = A[idx + e_a] (axis a = 0 / 1 / 2 = x / y / z of a [Dz,Dy,Dx] array), `fill` where idx + e_a leaves the grid."""
    ax = 2 - a
    out = np.full_like(A, fill)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    src[ax], dst[ax] = slice(1, None), slice(None, -1)
    out[tuple(dst)] = A[tuple(src)]
    return out


def _shift_back(A, a, fill):
    """result[idx] = A[idx - e_a]."""
    ax = 2 - a
    out = np.full_like(A, fill)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    src[ax], dst[ax] = slice(None, -1), slice(1, None)
    out[tuple(dst)] = A[tuple(src)]
    return out


def surface(vol, origin, voxel, w_min=0.0, max_jump=np.inf):
    """vol [Dz,Dy,Dx,2] in its dtype -> dict in candidate order: index [N] int64 (e = 3 * n + a), points [N,3], normals [N,3] (NaN rows:
    none), std [N] in that dtype, axis [N], t [N]."""
    dt = vol.dtype.type
    Dz, Dy, Dx = vol.shape[:3]
    F, Wt = vol[..., 0], vol[..., 1]
    org = [dt(np.float32(v)) for v in origin]
    vx, wm, mj = dt(np.float32(voxel)), dt(np.float32(w_min)), dt(np.float32(max_jump))
    inside = np.ones((Dz, Dy, Dx), bool)
    n = np.arange(Dz * Dy * Dx, dtype=np.int64).reshape(Dz, Dy, Dx)
    kk, jj, ii = np.meshgrid(np.arange(Dz), np.arange(Dy), np.arange(Dx), indexing="ij")
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # the central differences and their validity at every voxel
        G, V = [], []
        for c in range(3):
            hi_in, lo_in = _shift(inside, c, False), _shift_back(inside, c, False)
            f1, f0 = _shift(F, c, dt(0)), _shift_back(F, c, dt(0))
            w1, w0 = _shift(Wt, c, dt(0)), _shift_back(Wt, c, dt(0))
            G.append(f1 - f0)
            V.append(hi_in & lo_in & (w1 > 0) & (w0 > 0))
        valid = V[0] & V[1] & V[2]
        es, rows = [], []
        for a in range(3):
            Fq, Wq, q_in = _shift(F, a, dt(1)), _shift(Wt, a, dt(0)), _shift(inside, a, False)
            keep = q_in & (Wt > 0) & (Wq > 0) & (Wt >= wm) & (Wq >= wm) & (((F < 0) & (Fq >= 0)) | ((F >= 0) & (Fq < 0))) & \
                (np.abs(F - Fq) <= mj)
            sel = np.flatnonzero(keep.ravel())
            fp, fq, wp, wq = F.ravel()[sel], Fq.ravel()[sel], Wt.ravel()[sel], Wq.ravel()[sel]
            t = fp / (fp - fq)
            idx = [ii.ravel()[sel].astype(dt), jj.ravel()[sel].astype(dt), kk.ravel()[sel].astype(dt)]
            idx[a] = idx[a] + t
            pts = np.stack([org[c] + vx * idx[c] for c in range(3)], -1)
            h = dt(1) - t
            std = dt(1) / np.sqrt(h * wp + t * wq)
            g = [h * G[c].ravel()[sel] + t * _shift(G[c], a, dt(0)).ravel()[sel] for c in range(3)]
            ln = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            ok = valid.ravel()[sel] & _shift(valid, a, False).ravel()[sel] & (ln > 0) & np.isfinite(ln)
            nrm = np.where(ok[:, None], np.stack([g[0] / ln, g[1] / ln, g[2] / ln], -1), dt(np.nan))
            es.append(3 * n.ravel()[sel] + a)
            rows.append((pts, nrm, std, np.full(sel.size, a), t))
        e = np.concatenate(es)
        order = np.argsort(e, kind="stable")
        cat = [np.concatenate([r[c] for r in rows])[order] for c in range(5)]
    out = dict(index=e[order], points=cat[0].astype(dt), normals=cat[1].astype(dt), std=cat[2].astype(dt), axis=cat[3], t=cat[4])
    assert cat[0].dtype == np.dtype(dt) and cat[1].dtype == np.dtype(dt) and cat[2].dtype == np.dtype(dt)
    return out


# ---- the inputs --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def random_volume(dims):
    """[RANDOM_B,Dz,Dy,Dx,2] f32, read-only: F uniform in [-1, 1], 15 % of the voxels with Wt = 0 and the rest uniform in [0.5, 900], 2 %
    each of F set to 0.0, -0.0 and NaN; the three smallest shapes carry a hand-set crossing instead."""
    Dx, Dy, Dz = dims
    rng = np.random.default_rng(9100 + Dx + 7 * Dy + 31 * Dz)
    shape = (RANDOM_B, Dz, Dy, Dx)
    F = rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    Wt = np.where(rng.random(shape) < 0.15, 0.0, rng.uniform(0.5, 900.0, shape)).astype(np.float32)
    u = rng.random(shape)
    F[u < 0.02] = 0.0
    F[(u >= 0.02) & (u < 0.04)] = -0.0
    F[(u >= 0.04) & (u < 0.06)] = np.nan
    if Dx * Dy * Dz <= 2:
        F[...] = np.float32(0.5)
        Wt[...] = np.float32(2.0)
        F[0].flat[-1] = -0.25                          # image 0: a crossing on the only edge there is (none in 1 x 1 x 1)
        F[1].flat[0], F[1].flat[-1] = -0.0, -0.75      # image 1: -0.0 is non-negative, so this crosses too
        Wt[1].flat[-1] = 3.0
    vol = np.stack([F, Wt], -1)
    vol.setflags(write=False)
    return vol


def inputs():
    """name -> (vol [B,Dz,Dy,Dx,2] f32, origin, voxel) for every input of (a) and (b)."""
    out = {name: (S.states(name)[-1], S.TSDF_CASES[name]["origin"], S.VOXEL) for name in STATE_CASES}
    for dims in RANDOM_DIMS:
        out["random_%dx%dx%d" % dims] = (random_volume(dims), RANDOM_ORIGIN, RANDOM_VOXEL)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, b, w_min=0.0, max_jump=np.inf, dt=np.float32):
    """The dict of `surface` for image b of the input in dt -- read-only, shared."""
    vol, origin, voxel = inputs()[name]
    r = surface(vol[b].astype(dt), origin, voxel, w_min, max_jump)
    for v in r.values():
        v.setflags(write=False)
    return r


def scene_distance(pts):
    """Distance (float64, metres) of world points to the analytic wall-and-sphere scene of tsdf_ref.py."""
    p = np.asarray(pts, np.float64)
    wall = np.abs(p @ S.WALL_N - S.WALL_C)
    sph = np.abs(np.linalg.norm(p - S.SPHERE_C, axis=-1) - S.SPHERE_R)
    return np.minimum(wall, sph)


def angle(a, b):
    return P.angle(a, b)
