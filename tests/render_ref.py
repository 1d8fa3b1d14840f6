"""numpy restatement of the definitions of `cfp_render_depth`, `cfp_render_zones` and `cfp_render_rgb` (include/cfpnet_hip.h) -- TEST
INFRASTRUCTURE.

Float32 with the header's order of operations (numpy rounds every float32 operation once, like the library built without fused
multiply-adds); the depth is `pointcloud_ref.depth`, the restatement of met_pred in mode 0.  Two tiers of inputs:

  exact      inputs on which every intermediate is exact in float32 (depths k / 64 m with vmin = 0, vmax = 8: t = k / 2 and
             v * 1000 = k * 15.625; zone samples that are multiples of 2^-6; the 256 byte values through the normalisation and back),
             plus NaN, +-inf and out-of-range entries.  Byte equality on every pixel.
  realistic  `synthetic.make_eval_pair` data through the bilinear blend.  The kernel's d may differ from the restatement's by the
             project's bound for this very value, |dd| <= RTOL * max(|d|, 1e-3) (tests/test_metrics.py; `pointcloud_ref.close_points`).
             Every pixel is checked: its colour (or its 16-bit count) must be one the definition yields for some d' in that interval --
             `accepted` computes the interval of table indices (counts), which is a single one wherever the interval of d' crosses no
             boundary.  `crossing_share` reports the share of pixels where it does; tests/test_render_abi.py caps it.

Also the inputs the GPU tests use, so that the CPU tests examine the same tensors."""
import functools

import numpy as np

import pointcloud_ref as P
from cfpnet_amd import synthetic
from cfpnet_amd.geometry import centered_zone_rects

RTOL = P.RTOL
LO, HI = P.LO, P.HI
DEPTH, GT, ABS_ERR, REL_ERR = range(4)
WHITE = np.array([255, 255, 255], np.uint8)
F = np.float32


# ---- the lookup ----------------------------------------------------------------------------------------------------------------------------

def lut_index(v, vmin, vmax):
    """Table index of the float32 values v: 0..255, or -1 for NaN (the "bad" colour)."""
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = ((v - F(vmin)) / (F(vmax) - F(vmin))) * F(256)
        assert t.dtype == F
        idx = np.where(t < 0, 0, np.where(t >= 256, 255, np.where(np.isnan(t), 0, t))).astype(np.int64)
    return np.where(np.isnan(t), -1, idx)


def index_colour(idx, lut):
    """[...,3] uint8 from indices (-1 -> black)."""
    c = lut[np.maximum(idx, 0)]
    c[idx < 0] = 0
    return c


def lookup(v, vmin, vmax, lut):
    return index_colour(lut_index(v, vmin, vmax), lut)


def u16_count(v, scale):
    """(uint16) of v * scale: NaN or <= 0 -> 0, >= 65535 -> 65535, else rint (ties to even)."""
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.asarray(v, F) * F(scale)
        assert m.dtype == F
        r = np.where(m >= 65535, F(65535), np.rint(m))
        r = np.where(m > 0, r, F(0))                   # NaN and <= 0
    return r.astype(np.uint16)


# ---- cfp_render_depth ----------------------------------------------------------------------------------------------------------------------

def value(what, d, gt):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if what == DEPTH:
            return d
        if what == GT:
            return gt
        e = np.abs(d - gt)
        return e if what == ABS_ERR else e / gt


def painted(what, gt, lo, hi, shape):
    if what == DEPTH:
        return np.ones(shape, bool)
    with np.errstate(invalid="ignore"):
        return (gt > F(lo)) & (gt < F(hi))


def render_depth(pred, gt, H, W, interp, what, vmin, vmax, lut, lo=LO, hi=HI):
    """One image: pred [h,w] f32 or None, gt [H,W] f32 or None -> uint8 [H,W,3]."""
    d = None if what == GT else P.depth(pred, H, W, interp, lo, hi)
    ok = painted(what, gt, lo, hi, (H, W))
    out = lookup(value(what, d, gt), vmin, vmax, lut)
    out[~ok] = WHITE
    return out


def render_u16(pred, gt, H, W, interp, what, scale, lo=LO, hi=HI):
    d = None if what == GT else P.depth(pred, H, W, interp, lo, hi)
    out = u16_count(value(what, d, gt), scale)
    out[~painted(what, gt, lo, hi, (H, W))] = 0
    return out


def _d_interval(d):
    """The float32 ends of [d - e, d + e], e = RTOL * max(|d|, 1e-3); NaN stays NaN."""
    e = RTOL * np.maximum(np.abs(d.astype(np.float64)), 1e-3)
    return (d - e).astype(F), (d + e).astype(F)


def _v_interval(what, d, gt):
    """The ends (v_lo, v_hi) of the values the definition yields for d' in the interval of d: the error kinds are |d' - gt| (/ gt),
    which reaches 0 when the interval contains gt."""
    if what == GT:
        return gt, gt
    dl, dh = _d_interval(d)
    if what == DEPTH:
        return dl, dh
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a, b = value(what, dl, gt), value(what, dh, gt)
        lo_v = np.where((dl <= gt) & (gt <= dh), F(0), np.minimum(a, b))
        return lo_v, np.maximum(a, b)


def accepted(pred, gt, H, W, interp, what, fn, lo=LO, hi=HI):
    """fn: float32 values -> integers (a table index or a 16-bit count), monotone in v.  -> (n_lo, n_hi, ok): a pixel painted per `ok`
    may show any integer in [n_lo, n_hi]; the two are equal where the interval of d' crosses no boundary."""
    d = None if what == GT else P.depth(pred, H, W, interp, lo, hi)
    v_lo, v_hi = _v_interval(what, d, gt)
    ok = painted(what, gt, lo, hi, (H, W))
    n_lo, n_hi = fn(v_lo).astype(np.int64), fn(v_hi).astype(np.int64)
    n_lo, n_hi = np.where(ok, n_lo, 0), np.where(ok, n_hi, 0)          # what an unpainted pixel's value would give is of no interest
    assert (n_lo <= n_hi).all()
    return n_lo, n_hi, ok


def check_colour(got, pred, gt, H, W, interp, what, vmin, vmax, lut, what_name=""):
    """Every pixel of got [H,W,3]: white where unpainted, else the colour of an index in its accepted interval.  -> share of painted
    pixels whose interval holds more than one index."""
    n_lo, n_hi, ok = accepted(pred, gt, H, W, interp, what, lambda v: lut_index(v, vmin, vmax))
    assert got.shape == (H, W, 3) and got.dtype == np.uint8
    assert (got[~ok] == WHITE).all(), what_name
    good = np.zeros((H, W), bool)
    gap = int((n_hi - n_lo).max()) if n_lo.size else 0
    for k in range(gap + 1):
        good |= (index_colour(np.minimum(n_lo + k, n_hi), lut) == got).all(-1)
    bad = ok & ~good
    plain = (got == render_depth(pred, gt, H, W, interp, what, vmin, vmax, lut)).all(-1)
    share = float(((n_hi != n_lo) & ok).sum() / max(ok.sum(), 1))
    print(f"{what_name}: {int((~plain).sum())} of {H * W} pixels differ from the restatement, {int(bad.sum())} outside the accepted interval; "
          f"{100 * share:.2f} % of {int(ok.sum())} painted pixels cross a boundary, largest index gap {gap}")
    assert not bad.any(), (what_name, int(bad.sum()))
    return share


def check_u16(got, pred, gt, H, W, interp, what, scale, what_name=""):
    n_lo, n_hi, ok = accepted(pred, gt, H, W, interp, what, lambda v: u16_count(v, scale))
    assert got.shape == (H, W) and got.dtype == np.uint16
    assert (got[~ok] == 0).all(), what_name
    g = got.astype(np.int64)
    bad = ok & ((g < n_lo) | (g > n_hi))
    share = float(((n_hi != n_lo) & ok).sum() / max(ok.sum(), 1))
    print(f"{what_name}: u16 {int((got != render_u16(pred, gt, H, W, interp, what, scale)).sum())} of {H * W} differ from the restatement, "
          f"{int(bad.sum())} outside the accepted interval; {100 * share:.2f} % cross a boundary, largest gap {int((n_hi - n_lo).max())}")
    assert not bad.any(), (what_name, int(bad.sum()))
    return share


def crossing_share(pred, gt, H, W, interp, what, fn):
    """(share of painted pixels whose accepted interval holds more than one integer, the largest gap)."""
    n_lo, n_hi, ok = accepted(pred, gt, H, W, interp, what, fn)
    return float(((n_hi != n_lo) & ok).sum() / max(ok.sum(), 1)), int((n_hi - n_lo).max())


# ---- cfp_render_zones ----------------------------------------------------------------------------------------------------------------------

def zone_of(rect, H, W):
    """[H,W] index of the first zone containing the pixel, compared in float32; -1: none."""
    Y, X = np.arange(H, dtype=F)[:, None], np.arange(W, dtype=F)[None, :]
    z_of = np.full((H, W), -1, np.int64)
    for z in range(rect.shape[0] - 1, -1, -1):          # backwards, so that the first zone in index order wins
        sy, sx, ey, ex = rect[z]
        z_of[(sy <= Y) & (Y < ey) & (sx <= X) & (X < ex)] = z
    return z_of


def render_zones(out, hist, rect, mask, vmin, vmax, lut, alpha):
    """One image: out uint8 [H,W,3] -> a new array with the zones drawn over it."""
    H, W = out.shape[:2]
    rect = rect.astype(F)
    z_of = zone_of(rect, H, W)
    s = hist[:, 0].astype(F)
    for k in range(1, hist.shape[1]):
        s = s + hist[:, k].astype(F)
    inner = lookup(s / F(hist.shape[1]), vmin, vmax, lut)
    inner[np.asarray(mask) == 0] = 128
    z = np.maximum(z_of, 0)
    Y, X = np.broadcast_to(np.arange(H, dtype=F)[:, None], (H, W)), np.broadcast_to(np.arange(W, dtype=F)[None, :], (H, W))
    sy, sx, ey, ex = (rect[z, i] for i in range(4))
    border = (Y < sy + F(1)) | (Y >= ey - F(1)) | (X < sx + F(1)) | (X >= ex - F(1))
    c = inner[z].astype(np.int64)
    c[border] = 0
    blended = ((c * alpha + out.astype(np.int64) * (256 - alpha) + 128) >> 8).astype(np.uint8)
    res = out.copy()
    res[z_of >= 0] = blended[z_of >= 0]
    return res


# ---- cfp_render_rgb ------------------------------------------------------------------------------------------------------------------------

MEAN, STD = synthetic.IMAGENET_MEAN, synthetic.IMAGENET_STD


def _u8(v):
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.where(v >= 1, F(255), np.rint(v * F(255)))
        return np.where(v > 0, r, F(0)).astype(np.uint8)


def denorm(rgb, mean=MEAN, std=STD):
    """rgb [3,H,W] f32 -> v [H,W,3] f32 = x * std + mean, one rounding per operation."""
    v = rgb.astype(F) * np.asarray(std, F)[:, None, None] + np.asarray(mean, F)[:, None, None]
    assert v.dtype == F
    return np.ascontiguousarray(v.transpose(1, 2, 0))


def render_rgb(rgb, mean=MEAN, std=STD):
    return _u8(denorm(rgb, mean, std))


def check_rgb(got, rgb, what_name=""):
    """Every byte of got [H,W,3] is one the definition yields for some v' within RTOL * max(|v|, 1e-3) of the restatement's v."""
    v = denorm(rgb)
    lo_v, hi_v = _d_interval(v)
    n_lo, n_hi = _u8(lo_v).astype(np.int64), _u8(hi_v).astype(np.int64)
    g = got.astype(np.int64)
    bad = (g < n_lo) | (g > n_hi)
    print(f"{what_name}: {int((got != _u8(v)).sum())} of {got.size} bytes differ from the restatement, {int(bad.sum())} outside the accepted "
          f"interval; {100 * float((n_lo != n_hi).mean()):.2f} % cross a boundary")
    assert got.dtype == np.uint8 and not bad.any(), what_name


def byte_round_trip():
    """rgb [3,16,16] f32: channel c holds (u / 255 - mean[c]) / std[c] for the 256 byte values u; and the bytes [16,16,3] to come back."""
    u = np.arange(256, dtype=F).reshape(16, 16)
    x = np.stack([((u / F(255)) - MEAN[c]) / STD[c] for c in range(3)]).astype(F)
    return x, np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, 2)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------

# name: the case of pointcloud_ref.UNPROJECT_CASES whose prediction it shares, and the seeds of the ground truth
CASES = {
    "odd_19x27_to_37x53": (41,),
    "same_24x40_direct": (42,),
    "same_24x40_interp": (42,),
    "row_1x33": (61,),
    "column_33x1": (62,),
    "batch3_nonfinite": (50, 51, 52),
    "full_240x320_to_480x640": (43,),
}
EXACT_RANGE = (0.0, 8.0)
COLOUR_RANGES = ((1e-3, 10.0), (0.0, 5.0), (0.5, 3.0))


def shape(name):
    c = P.UNPROJECT_CASES[name]
    return c["h"], c["w"], c["H"], c["W"], c["interp"]


@functools.lru_cache(maxsize=None)
def realistic_inputs(name):
    """(pred [B,h,w] f32, gt [B,H,W] f32 with holes) -- read-only."""
    h, w, H, W, _ = shape(name)
    pred = P.unproject_inputs(name)[0]
    if name.startswith(("row", "column")):
        gt = np.stack([synthetic.make_depth(H, W, seed=s, holes=0.2) for s in CASES[name]])
    else:
        gt = np.stack([synthetic.make_eval_pair(H, W, h, w, s, 0.1, 0.15)[0] for s in CASES[name]])
    gt = np.ascontiguousarray(gt, F)
    assert gt.shape == (pred.shape[0], H, W)
    gt.setflags(write=False)
    return pred, gt


@functools.lru_cache(maxsize=None)
def exact_inputs(name):
    """(pred [B,H,W], gt [B,H,W]) at the OUTPUT size of the case (rendered with interpolate = 0): depths k / 64 m, k in 32 .. 512, all
    481 of them when the image has that many pixels, the ground truth another walk through the same values; a few NaN, +-inf and
    out-of-range entries in both."""
    _, _, H, W, _ = shape(name)
    B, n = len(CASES[name]), H * W
    i = np.arange(B * n)
    pred = ((32 + (i * 7) % 481).astype(F) / F(64)).reshape(B, H, W)
    gt = ((32 + (i * 11 + 5) % 481).astype(F) / F(64)).reshape(B, H, W)
    # the special predictions sit on valid ground truth and the other way round
    for a, first, vals in ((pred.reshape(-1), 3, (np.nan, np.inf, -np.inf, 37.5, -1.0, 0.0)), (gt.reshape(-1), 4, (0.0, np.nan, 12.0, np.inf, -2.0))):
        for j, v in enumerate(vals):
            a[(first + 5 * j) % a.size] = v
    for a in (pred, gt):
        a.setflags(write=False)
    return pred, gt


def zone_inputs(Z, B=2, seed=7):
    """(hist [B,Z,16] f32 in multiples of 2^-6, mask [B,Z] bool) from `synthetic.make_inputs` with drop_hist = 0.34."""
    n = int(round(Z ** 0.5))
    add = synthetic.make_inputs(B, zone_num=n, seed=seed, drop_hist=0.34)["additional"]
    hist = (np.rint(add["hist_data"].numpy().astype(np.float64) * 64) / 64).astype(F)
    mask = add["mask"].numpy().astype(bool)
    assert hist.shape == (B, Z, 16) and mask.shape == (B, Z) and 0 < (~mask).sum() < mask.size
    return hist, mask


def zone_rects(kind, H, W, Z):
    """[Z,4] f32 for an H x W picture: `centered`, `pitched` (fractional pitch and origin) or `overhang` (beyond the top-left and the
    bottom-right corner)."""
    n = int(round(Z ** 0.5))
    px = min(H, W) // (n + 1)
    if kind == "centered":
        return centered_zone_rects(H, W, n, px)
    if kind == "pitched":
        return synthetic.pitched_zone_rects(px + 0.25, 1.75, 2.5, n)
    assert kind == "overhang"
    py, px_, oy, ox = F((H + 8) / n), F((W + 8) / n), F(-4.5), F(-3.25)
    rects = np.zeros((Z, 4), F)
    for zy in range(n):
        for zx in range(n):
            sy, sx = oy + F(zy) * py, ox + F(zx) * px_
            rects[zy * n + zx] = (sy, sx, sy + py, sx + px_)
    return rects
