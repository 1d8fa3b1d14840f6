"""numpy restatement of the sparsification definition (include/cfpnet_hip.h, cfp_unc_sparsification) -- TEST INFRASTRUCTURE.

The reference project has no such metric, so the definition is the contract and this file is its checker: float32 per-pixel terms,
float64 sums, tie groups by `np.unique`.  `test_sparsification_abi.py` checks this file against a plain stable argsort, against the
mean over random tie-breaks and against closed forms; `test_sparsification_gpu.py` checks the kernel against it."""
import numpy as np

RANKINGS = ("std", "entropy", "pmax", "oracle_rmse", "oracle_absrel")


def kept_counts(n, K):
    return [n - (k * n) // K for k in range(K)]


def terms(g, v):
    """float32 like the kernel: d = g - v, t0 = d*d, t1 = |d|/g."""
    g, v = g.astype(np.float32), v.astype(np.float32)
    with np.errstate(all="ignore"):
        d = g - v
        return d * d, np.abs(d) / g


def scores(planes, t0, t1):
    """planes [3,n] float32 (std, entropy, pmax) -> the five float32 scores, larger = removed first."""
    return [planes[0], planes[1], np.float32(1.0) - planes[2], t0, t1]


def _groups(s):
    """Tie groups of a float32 score in ascending order, -0 == +0, all NaNs one group above +inf -> (group index per pixel, group count)."""
    s = s.astype(np.float32) + np.float32(0.0)          # -0 -> +0
    nan = np.isnan(s)
    inv = np.empty(s.shape, np.int64)
    uniq, inv_f = np.unique(s[~nan], return_inverse=True)
    inv[~nan] = inv_f
    inv[nan] = uniq.size
    return inv, uniq.size + int(nan.any())


def curve(s, t0, t1, K):
    """One ranking: [2,K] float64.  The kept set of point k is the n_k smallest scores; a tie group straddling the boundary with t of
    its c members kept contributes t/c of its sums."""
    n = s.size
    inv, ng = _groups(s)
    cnt = np.bincount(inv, minlength=ng)
    cum = np.concatenate([[0], np.cumsum(cnt)])
    out = np.empty((2, K))
    for m, t in enumerate((t0, t1)):
        gs = np.bincount(inv, weights=t.astype(np.float64), minlength=ng)       # float64 sums per group
        cs = np.concatenate([[0.0], np.cumsum(gs)])
        for k, nk in enumerate(kept_counts(n, K)):
            j = int(np.searchsorted(cum, nk, side="left")) - 1                  # cum[j] < nk <= cum[j+1]
            S = cs[j] + (nk - cum[j]) / cnt[j] * gs[j]
            out[m, k] = np.sqrt(S / nk) if m == 0 else S / nk
    return out


def summarize(curves):
    """curves [5,2,K] -> (ause [3,2], aurg [3,2]); NaN when e0 == 0."""
    ause, aurg = np.full((3, 2), np.nan), np.full((3, 2), np.nan)
    if curves[3, 0, 0] == 0 or curves[4, 1, 0] == 0:
        return ause, aurg
    for u in range(3):
        for m in range(2):
            e0 = curves[3 + m, m, 0]
            ause[u, m] = np.mean(curves[u, m] - curves[3 + m, m]) / e0
            aurg[u, m] = np.mean(e0 - curves[u, m]) / e0
    return ause, aurg


def sparsify(g, v, planes, K):
    """Masked vectors: g, v [n], planes [3,n] -> dict(curves [5,2,K], ause, aurg, n_valid); all NaN for n == 0 or e0 == 0."""
    n = g.size
    curves = np.full((5, 2, K), np.nan)
    if n:
        t0, t1 = terms(g, v)
        with np.errstate(all="ignore"):
            for r, s in enumerate(scores(planes.astype(np.float32), t0, t1)):
                curves[r] = curve(s, t0, t1, K)
    ause, aurg = summarize(curves) if n else (np.full((3, 2), np.nan), np.full((3, 2), np.nan))
    if n and np.isnan(ause).all() and (curves[3, 0, 0] == 0 or curves[4, 1, 0] == 0):
        curves[:] = np.nan
    return dict(curves=curves, ause=ause, aurg=aurg, n_valid=n)


def image_equal_size(pred, unc, gt, lo, hi, K):
    """interpolate = 0, mode 0: pred [H,W] clipped to [lo, hi], unc [3,H,W] read directly, valid lo < gt < hi."""
    valid = np.logical_and(gt > lo, gt < hi)
    v = np.clip(pred.astype(np.float32), np.float32(lo), np.float32(hi))
    return sparsify(gt[valid], v[valid], unc[:, valid], K)


def curve_argsort(s, t0, t1, K):
    """The textbook form for tie-free scores: stable argsort, keep the first n_k."""
    order = np.argsort(s, kind="stable")
    c0, c1 = np.cumsum(t0[order].astype(np.float64)), np.cumsum(t1[order].astype(np.float64))
    out = np.empty((2, K))
    for k, nk in enumerate(kept_counts(s.size, K)):
        out[0, k], out[1, k] = np.sqrt(c0[nk - 1] / nk), c1[nk - 1] / nk
    return out


# ---- the interpolated protocol: align-corners bilinear with a chosen rounding of the blend ------------------------------------------

def _taps(n_in, n_out):
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    f = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(f.astype(np.int64), n_in - 1)
    i1 = i0 if n_in == n_out else np.minimum(i0 + 1, n_in - 1)
    lam = (f - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, lam


def bilinear(x, H, W, how):
    """x [h,w] float32 -> [H,W] float32, align_corners=True.  how = "ours": float32 op by op in the kernel's order
    hy*(hx*t00 + lx*t01) + ly*(hx*t10 + lx*t11); "f64": the same expression in float64, rounded once; "aten": ATen's order
    (torch.nn.functional.interpolate on the CPU)."""
    if how == "aten":
        import torch
        import torch.nn.functional as F
        return F.interpolate(torch.from_numpy(np.ascontiguousarray(x, np.float32))[None, None], (H, W), mode="bilinear",
                             align_corners=True)[0, 0].numpy()
    y0, y1, ly = _taps(x.shape[0], H)
    x0, x1, lx = _taps(x.shape[1], W)
    dt = np.float32 if how == "ours" else np.float64
    x = x.astype(dt)
    ly, lx = ly.astype(dt)[:, None], lx.astype(dt)[None, :]
    hy, hx = dt(1) - ly, dt(1) - lx
    t00, t01, t10, t11 = x[y0][:, x0], x[y0][:, x1], x[y1][:, x0], x[y1][:, x1]
    with np.errstate(all="ignore"):
        return (hy * (hx * t00 + lx * t01) + ly * (hx * t10 + lx * t11)).astype(np.float32)


def protocol_v(pred, H, W, lo, hi, mode, how):
    """pred [hp,wp] -> the prediction on the H x W grid under the protocol of `mode` (0: clip then bilinear; 1: bilinear, clamp, nan -> lo)."""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    p = pred.astype(np.float32)
    with np.errstate(all="ignore"):
        if mode == 0:
            return bilinear(np.clip(p, lo32, hi32), H, W, how)
        v = bilinear(p, H, W, how)
        v = np.where(v < lo32, lo32, np.where(v > hi32, hi32, v))
        return np.where(np.isnan(v), lo32, v).astype(np.float32)


def image_interpolated(pred, unc, gt, lo, hi, K, mode, how):
    """pred [hp,wp], unc [3,hp,wp] -> gt's grid with the protocol of `mode`; the planes are interpolated without a clip."""
    H, W = gt.shape
    v = protocol_v(pred, H, W, lo, hi, mode, how)
    with np.errstate(all="ignore"):
        planes = np.stack([bilinear(unc[i], H, W, how) for i in range(3)])
    valid = np.logical_and(gt > lo, gt < hi)
    return sparsify(gt[valid], v[valid], planes[:, valid], K)
