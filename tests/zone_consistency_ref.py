"""numpy restatement of the definition of `cfp_tof_zone_consistency` (include/cfpnet_hip.h) -- TEST INFRASTRUCTURE.

The depth at a pixel is `pointcloud_ref.depth` (met_pred in mode 0), which existing GPU tests hold bit for bit.  The bins are float32
with the header's formula (numpy rounds every float32 operation once, like the library built without fused multiply-adds); the floor
and the run selection are integers; the moments are a sequential float64 loop in ascending bin order, the order of the kernel, so
only `sqrt` can differ.  Also the inputs the GPU tests use, so that the CPU tests can examine the same tensors.

The measured (mu, sigma) of a case are what this same sensor model returns on a `scene` that differs a little from the prediction
(scaled and shifted), so most zones compare within a bin; the masks are then overridden per case to reach every state."""
import functools

import numpy as np

import pointcloud_ref as PR

BIN_WIDTH = 0.04          # tof.BIN_WIDTH
NAMES = ("n_compared", "mae_mu", "rmse_mu", "rel_mu", "mae_sigma", "frac_1bin", "frac_window", "n_lost", "n_unmeasured", "n_measured")
COMPARED, LOST, UNMEASURED, NEITHER = range(4)
NO_RETURN = (1.5, 0.05)   # the measured values given to a zone whose mask is forced on although the scene has no return there


def n_bins(max_d):
    return int(max_d / BIN_WIDTH)                         # metrics.zone_consistency


# ---- the sensor model (csrc/tof_cluster.h) -----------------------------------------------------------------------------------------------

def bins_of(d, max_d, bins):
    """float32 values -> bin index, -1 where ignored: bin = (int)(((d - 0.f) * (float)bins) / (max_d - 0.f)), d == max_d folded."""
    d = np.asarray(d, np.float32)
    md = np.float32(max_d)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (d >= np.float32(0)) & (d <= md)
        q = ((d - np.float32(0)) * np.float32(bins)) / (md - np.float32(0))
    assert q.dtype == np.float32
    b = np.where(ok, q, 0).astype(np.int64)
    b[b == bins] = bins - 1
    return np.where(ok, b, -1)


def floor_counts(d, max_d, bins, floor):
    """The histogram of a zone's depths after the floor: bin 0 cleared, `floor` subtracted, clamped at 0."""
    b = bins_of(d, max_d, bins)
    c = np.bincount(b[b >= 0], minlength=bins).astype(np.int64)
    c[0] = 0
    return np.maximum(c - floor, 0)


def runs(c):
    """[(start, stop, sum)] of the runs of consecutive non-zero bins, ascending."""
    out, j, n = [], 0, len(c)
    while j < n:
        if c[j] > 0:
            k = j
            while k < n and c[k] > 0:
                k += 1
            out.append((j, k, int(c[j:k].sum())))
            j = k
        else:
            j += 1
    return out


def moments(c, bin_width=BIN_WIDTH):
    """counts after the floor -> (mu, sigma, n) of the strongest run (lowest start on ties), sequential float64."""
    best = (0, 0, 0)
    for r in runs(c):
        if r[2] > best[2]:
            best = r
    start, stop, n = best
    nf = np.float64(np.float32(n) + np.float32(1e-9))
    centre = lambda j: (np.float64(np.float32(np.float64(j + 1) * bin_width)) + np.float64(j) * bin_width) / 2.0
    acc = np.float64(0.0)
    for j in range(start, stop):
        acc += centre(j) * np.float64(c[j])
    mu = acc / nf
    var = np.float64(0.0)
    for j in range(start, stop):
        d = centre(j) - mu
        var += np.float64(c[j]) * (d * d)
    return float(mu), float(np.sqrt(var / nf) + 1e-9), n


def members(rect, H, W):
    """[H,W] bool: sy <= (float)y < ey && sx <= (float)x < ex in float32; a NaN coordinate gives an empty zone."""
    sy, sx, ey, ex = (np.float32(v) for v in rect)
    ys, xs = np.arange(H).astype(np.float32), np.arange(W).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return ((sy <= ys) & (ys < ey))[:, None] & ((sx <= xs) & (xs < ex))[None, :]


def zone_table(d, rect, mask, raw, max_d, floor, bin_width=BIN_WIDTH):
    """d [H,W] f32, rect [Z,4], mask [Z], raw [Z,2] f64 -> [Z,6] f64 {mu_p, sigma_p, n_signal, n_pix, n_window, state}."""
    bins = n_bins(max_d)
    out = np.zeros((len(rect), 6), np.float64)
    for z, r in enumerate(rect):
        v = d[members(r, *d.shape)]                       # row-major; the order does not matter to a histogram
        mu, sigma, n = moments(floor_counts(v, max_d, bins, floor), bin_width)
        mu_m, s3 = np.float64(raw[z, 0]), 3.0 * np.float64(raw[z, 1])
        w = s3 if s3 > bin_width else np.float64(bin_width)
        with np.errstate(invalid="ignore"):
            inside = (mu_m - w <= v.astype(np.float64)) & (v.astype(np.float64) <= mu_m + w)
        measured = bool(mask[z])
        state = (COMPARED if n > 0 else LOST) if measured else (UNMEASURED if n > 0 else NEITHER)
        out[z] = (mu, sigma, n, v.size, int(inside.sum()) if measured else 0, state)
    return out


def summarize(zone, raw, bin_width=BIN_WIDTH):
    """[Z,6] zone table + [Z,2] measured -> the ten summary values, float64 sums in ascending zone order."""
    state = zone[:, 5].astype(np.int64)
    C = state == COMPARED
    meas = state <= LOST
    n = int(C.sum())
    out = np.full(10, np.nan)
    out[0] = n
    if n:
        dmu = np.abs(zone[C, 0] - raw[C, 0])
        out[1] = dmu.sum() / n
        out[2] = np.sqrt((dmu * dmu).sum() / n)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[3] = (dmu / raw[C, 0]).sum() / n
        out[4] = np.abs(zone[C, 1] - raw[C, 1]).sum() / n
        out[5] = int((dmu <= bin_width).sum()) / n
    npix = int(zone[meas, 3].sum())
    if npix:
        out[6] = int(zone[meas, 4].sum()) / npix
    out[7], out[8], out[9] = int((state == LOST).sum()), int((state == UNMEASURED).sum()), int(meas.sum())
    return out


def dev_map(d, rect, mask, raw):
    """d - (float)mu_m of the lowest-index measured zone that contains the pixel, NaN where there is none; float32."""
    out = np.full(d.shape, np.nan, np.float32)
    todo = np.ones(d.shape, bool)
    for z, r in enumerate(rect):
        if not mask[z]:
            continue
        m = members(r, *d.shape) & todo
        with np.errstate(invalid="ignore", over="ignore"):
            out[m] = d[m] - np.float32(raw[z, 0])
        todo &= ~m
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------

def _smooth(rng, h, w, near=1.2, dy=0.6, dx=0.3, box=0.8, noise=0.01):
    """A tilted plane with a box standing `box` metres behind it and a little noise: zones that straddle the edge see two returns."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    p = near + dy * yy / h + dx * xx / w
    p[h // 3: 2 * h // 3, w // 2: 5 * w // 6] += box
    return (p + rng.normal(0.0, noise, (h, w))).astype(np.float32)


def _interp(rng):
    rect = [(2.5, 3.25, 20.75, 25.5),                    # fractional
            (10.0, 15.5, 30.5, 40.0),                     # overlaps zone 0
            (-6.5, 40.2, 12.3, 60.0),                     # partly off the image (top and right)
            (40.0, 5.0, 50.0, 20.0),                      # wholly off (H = 37)
            (np.nan, 5.0, 20.0, 20.0),                    # a NaN coordinate: empty
            (12.0, 8.0, 12.0, 30.0),                      # zero area
            (22.3, 1.0, 36.9, 22.7)]
    return dict(pred=_smooth(rng, 19, 27)[None], rect=np.array([rect], np.float32), force={(0, 3): 1, (0, 4): 1, (0, 5): 0})


def _big(rng):
    p = _smooth(rng, 64, 64, noise=0.004)
    p[56:59, 2:7] = np.array([1.22] * 7 + [np.nan] + [1.62] * 7, np.float32).reshape(3, 5)      # two runs of 7 counts: a tie
    return dict(pred=p[None], rect=np.array([[(3, 7, 53, 54), (56, 2, 59, 7)]], np.float32), force={})


def _bins1024(rng):
    yy, xx = np.mgrid[0:24, 0:32].astype(np.float64)
    p = (0.5 + 40.3 * (yy * 32 + xx) / (24 * 32 - 1) + rng.normal(0.0, 0.004, (24, 32))).astype(np.float32)      # 0.5 .. 40.8 m
    p[5, 3:9] = np.nan
    return dict(pred=p[None], rect=np.array([[(0, 0, 24, 32), (18.5, 0, 24, 32), (0, 0, 3, 32)]], np.float32), force={})


def _hi(rng):
    p = _smooth(rng, 20, 28, near=2.9, dy=0.9, dx=0.5, box=1.5)        # a good part beyond hi = max_d = 4: clipped onto 4.0, the last bin
    p[0, 0] = 4.0
    return dict(pred=p[None], rect=np.array([[(0, 0, 20, 14), (0, 14, 20, 28), (6, 12, 14, 24)]], np.float32), force={})


def _batch3(rng):
    p = np.stack([_smooth(rng, 16, 20), _smooth(rng, 16, 20, near=0.8), _smooth(rng, 16, 20, near=1.6)])
    p[0, 2, 3], p[0, 9, 11:14], p[0, 12, 5], p[0, 13, 6] = np.nan, np.nan, np.inf, -np.inf
    p[1, 4, 4:9], p[1, 10, 2] = np.nan, np.inf
    rect = np.array([[(0, 0, 16, 20), (16, 0, 32, 20), (0, 20, 16, 40), (16, 20, 32, 40)],
                     [(1.5, 2.5, 17.5, 22.5), (14, 2, 30, 18), (3, 22, 19, 38), (33, 0, 40, 10)],
                     [(0, 0, 11, 40), (11, 0, 22, 40), (22, 0, 32, 13), (22, 13, 32, 40)]], np.float32)
    p[2, :11, :] = 20.0                                   # clipped to hi = 10 > max_d: the two measured zones of image 2 are lost
    p[2, 5, 5] = -np.inf
    # image 0: one zone dropped (unmeasured); image 1: nothing measured; image 2: zones 0 and 1 measured, both lost
    force = {(0, 2): 0, (1, 0): 0, (1, 1): 0, (1, 2): 0, (1, 3): 0, (2, 0): 1, (2, 1): 1, (2, 2): 0, (2, 3): 0}
    return dict(pred=p, rect=rect, force=force)


def _flat(rng):
    return dict(pred=np.full((1, 64, 64), 2.0, np.float32), rect=np.array([[(0, 0, 64, 64)]], np.float32), force={})


CASES = {
    "interp_19x27_to_37x53": dict(make=_interp, seed=11, H=37, W=53, interp=1, max_d=4.0, floor=2, lo=1e-3, hi=10.0),
    "big_zone": dict(make=_big, seed=12, H=64, W=64, interp=0, max_d=4.0, floor=0, lo=1e-3, hi=10.0),
    "bins_1024": dict(make=_bins1024, seed=13, H=24, W=32, interp=0, max_d=40.96, floor=0, lo=1e-3, hi=50.0),
    "hi_equals_max_d": dict(make=_hi, seed=14, H=20, W=28, interp=0, max_d=4.0, floor=2, lo=1e-3, hi=4.0),
    "batch3_nonfinite": dict(make=_batch3, seed=15, H=32, W=40, interp=1, max_d=4.0, floor=2, lo=1e-3, hi=10.0),
    "flat": dict(make=_flat, seed=16, H=64, W=64, interp=0, max_d=4.0, floor=2, lo=1e-3, hi=10.0),
}


def depth(name, pred):
    c = CASES[name]
    return np.stack([PR.depth(p, c["H"], c["W"], c["interp"], c["lo"], c["hi"]) for p in pred])


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> pred [B,h,w] f32, rect [B,Z,4] f32, mask [B,Z] u8, raw [B,Z,2] f64; read-only arrays."""
    c = CASES[name]
    made = c["make"](np.random.default_rng(c["seed"]))
    pred, rect = made["pred"], made["rect"]
    d = depth(name, pred)
    with np.errstate(invalid="ignore", over="ignore"):
        scene = (d * np.float32(1.01) + np.float32(0.01)).astype(np.float32)
    B, Z = rect.shape[:2]
    mask, raw = np.zeros((B, Z), np.uint8), np.zeros((B, Z, 2), np.float64)
    for b in range(B):
        for z in range(Z):
            v = scene[b][members(rect[b, z], c["H"], c["W"])]
            mu, sigma, n = moments(floor_counts(v, c["max_d"], n_bins(c["max_d"]), c["floor"]))
            mask[b, z], raw[b, z] = n > 0, (mu, sigma)
    for (b, z), v in made["force"].items():
        if v and not mask[b, z]:
            raw[b, z] = NO_RETURN
        mask[b, z] = v
    for a in (pred, rect, mask, raw):
        a.setflags(write=False)
    return pred, rect, mask, raw


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> dict(zone [B,Z,6], summary [B,10], map [B,H,W] f32, depth [B,H,W] f32)."""
    c = CASES[name]
    pred, rect, mask, raw = inputs(name)
    d = depth(name, pred)
    zone = np.stack([zone_table(d[b], rect[b], mask[b], raw[b], c["max_d"], c["floor"]) for b in range(len(d))])
    res = dict(zone=zone, summary=np.stack([summarize(zone[b], raw[b]) for b in range(len(d))]),
               map=np.stack([dev_map(d[b], rect[b], mask[b], raw[b]) for b in range(len(d))]), depth=d)
    for a in res.values():
        a.setflags(write=False)
    return res


def zone_counts(name, b, z):
    """The histogram after the floor of zone z of image b, for tests that look at the runs."""
    c = CASES[name]
    pred, rect, _, _ = inputs(name)
    d = depth(name, pred)[b]
    return floor_counts(d[members(rect[b, z], c["H"], c["W"])], c["max_d"], n_bins(c["max_d"]), c["floor"])


# ---- the round trip: a ground-truth map against its own simulation ---------------------------------------------------------------------

ROUND_TRIP = dict(B=2, H=96, W=128, zone_num=3, zone_px=24, sy0=12, sx0=28, max_d=4.0, floor=2, lo=1e-3, hi=10.0, nsamp=16)


@functools.lru_cache(maxsize=None)
def round_trip_depth():
    """[2,96,128] f32 with zeros, NaN and values above max_distance: every zone of the 3 x 3 grid of 24 px zones keeps or loses its return."""
    rng = np.random.default_rng(21)
    g = np.stack([_smooth(rng, 96, 128, near=1.0, dy=0.5, dx=0.7, noise=0.005), _smooth(rng, 96, 128, near=2.6, dy=1.2, dx=0.9, noise=0.005)])
    g[0, 20:30, 40:70] = 0.0                              # holes
    g[0, 50, 30:60], g[1, 70:74, 90:96] = np.nan, np.nan
    g[1, 12:36, 28:52] = 7.5                              # a whole zone beyond max_distance: no return
    g[0, 60:84, 76:100][::2, ::3] = 0.0
    g.setflags(write=False)
    return g
