"""numpy float64 restatement of the definition of `cfp_tof_zone_loss` (include/cfpnet_hip.h) -- TEST INFRASTRUCTURE.

Built on `zone_consistency_ref`: its `depth`, `members`, `bins_of`, `floor_counts` and `runs` are the metric's bits, and its `CASES` are
the inputs, plus one case with 260 small zones (the backward stages the zones through LDS in chunks of 256).  Everything after the run
is float64: the weights omega_j = c'_j / cnt_j, the zone mean, the dead zone, the Huber penalty, the means over zones and images, and the
gradient with the run and the weights held constant, carried to `pred` through the transpose of the blend (a scatter here, a gather in
the kernel) times the derivative of the clip.  `loss` also returns, per element of `pred`, the sum of the absolute values of the terms
of its gradient and their number: the GPU test's bound is stated in them.

`frozen_loss` evaluates the same objective on a float64 prediction with every zone's pixel weights frozen, through a gather blend that
shares no code with the gradient's scatter: central differences of it check the analytic gradient (tests/test_zone_loss_ref.py)."""
import functools

import numpy as np

import zone_consistency_ref as ZR

BIN_WIDTH = ZR.BIN_WIDTH
COLUMNS = ("m_z", "n_z", "r_z", "rho_z", "run_start", "run_stop", "state", "coef")
M, N, R, RHO, START, STOP, STATE, COEF = range(8)
INT_COLS = (N, START, STOP, STATE)
FLOORS = (0, 2, 20)


# ---- the cases: the metric's table and one with more zones than a chunk ------------------------------------------------------------------

def _many_zones(rng):
    """13 x 20 = 260 rectangles of about 4 x 4 pixels on 32 x 40, fractional and overlapping their neighbours by a pixel."""
    rect = [(2.4 * i - 0.3, 2.0 * j - 0.6, 2.4 * i + 3.4, 2.0 * j + 3.1) for i in range(13) for j in range(20)]
    return dict(pred=ZR._smooth(rng, 16, 20, noise=0.003)[None], rect=np.array([rect], np.float32), force={(0, 7): 0, (0, 258): 0})


EXTRA = {"many_zones_260": dict(make=_many_zones, seed=31, H=32, W=40, interp=1, max_d=4.0, floor=0, lo=1e-3, hi=10.0, scale=1.03, shift=0.02)}
CASES = {**ZR.CASES, **EXTRA}
RUNS = [(name, c["floor"]) for name, c in CASES.items()] + [(name, 20) for name, c in CASES.items() if c["floor"] != 20]


def depth(name, pred):
    c = CASES[name]
    return np.stack([ZR.PR.depth(p, c["H"], c["W"], c["interp"], c["lo"], c["hi"]) for p in pred])


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> pred [B,h,w] f32, rect [B,Z,4] f32, mask [B,Z] u8, raw [B,Z,2] f64; read-only.  The metric's inputs for its cases; the extra
    case is measured by the same recipe (the sensor model on a scene that is the prediction scaled and shifted a little more)."""
    if name in ZR.CASES:
        return ZR.inputs(name)
    c = CASES[name]
    made = c["make"](np.random.default_rng(c["seed"]))
    pred, rect = made["pred"], made["rect"]
    d = depth(name, pred)
    scene = (d * np.float32(c["scale"]) + np.float32(c["shift"])).astype(np.float32)
    B, Z = rect.shape[:2]
    mask, raw = np.zeros((B, Z), np.uint8), np.zeros((B, Z, 2), np.float64)
    for b in range(B):
        for z in range(Z):
            v = scene[b][ZR.members(rect[b, z], c["H"], c["W"])]
            mu, sigma, n = ZR.moments(ZR.floor_counts(v, c["max_d"], ZR.n_bins(c["max_d"]), c["floor"]))
            mask[b, z], raw[b, z] = n > 0, (mu, sigma)
    for (b, z), v in made["force"].items():
        mask[b, z] = v
    for a in (pred, rect, mask, raw):
        a.setflags(write=False)
    return pred, rect, mask, raw


# ---- the blend (csrc/metrics_pred.h, mode 0) and its transpose ----------------------------------------------------------------------------

def taps(Hp, Wp, H, W):
    """The float32 taps of met_pred: (y0, y1, ly, hy), (x0, x1, lx, hx); the weights are float32 values, exact in float64."""
    return ZR.PR._taps(Hp, H, np.float32), ZR.PR._taps(Wp, W, np.float32)


def blend64(p, H, W, interp):
    """The blend of a clipped float64 map with the float32 tap weights, as a gather."""
    if not interp:
        return p
    (y0, y1, ly, hy), (x0, x1, lx, hx) = taps(*p.shape, H, W)
    ly, hy, lx, hx = (a.astype(np.float64) for a in (ly, hy, lx, hx))
    ly, hy, lx, hx = ly[:, None], hy[:, None], lx[None, :], hx[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        return hy * (hx * p[np.ix_(y0, x0)] + lx * p[np.ix_(y0, x1)]) + ly * (hx * p[np.ix_(y1, x0)] + lx * p[np.ix_(y1, x1)])


def blend_transpose(g, Hp, Wp, interp):
    """g [H,W] f64 on the grid -> (the gradient on the [Hp,Wp] taps, the sum of the absolute terms, their number), as a scatter."""
    if not interp:
        return g.copy(), np.abs(g), (g != 0).astype(np.int64)
    H, W = g.shape
    (y0, y1, ly, hy), (x0, x1, lx, hx) = taps(Hp, Wp, H, W)
    out, tot, cnt = np.zeros((Hp, Wp)), np.zeros((Hp, Wp)), np.zeros((Hp, Wp), np.int64)
    for yi, wy in ((y0, hy), (y1, ly)):
        for xi, wx in ((x0, hx), (x1, lx)):
            w = wy.astype(np.float64)[:, None] * wx.astype(np.float64)[None, :]
            idx = (np.broadcast_to(yi[:, None], g.shape), np.broadcast_to(xi[None, :], g.shape))
            np.add.at(out, idx, w * g)
            np.add.at(tot, idx, np.abs(w * g))
            np.add.at(cnt, idx, ((w != 0) & (g != 0)).astype(np.int64))
    return out, tot, cnt


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------

def huber(e, delta):
    return e * e / (2.0 * delta) if e <= delta else e - delta / 2.0


def zone_run(v, max_d, bins, floor, weighted=True):
    """A zone's float32 depths -> (bin of each pixel, its weight omega, a, b, n_z).  `weighted` False: the unweighted mean of the run's
    pixels (every omega 1, n_z their number), which the definition rejects."""
    bn = ZR.bins_of(v, max_d, bins)
    cnt = np.bincount(bn[bn >= 0], minlength=bins).astype(np.int64)
    cf = ZR.floor_counts(v, max_d, bins, floor)
    best = (bins, bins, 0)
    for r in ZR.runs(cf):
        if r[2] > best[2]:
            best = r
    a, b, n = best
    omega = np.zeros(bins)
    if n > 0:
        omega[a:b] = cf[a:b] / cnt[a:b] if weighted else 1.0
    w = np.where(bn >= 0, omega[np.maximum(bn, 0)], 0.0)
    if not weighted:
        n = int((w > 0).sum())
    return bn, w, a, b, n


def loss(pred, rect, mask, raw, H, W, interp, lo, hi, max_d, floor, delta=None, grad_scale=1.0, bin_width=BIN_WIDTH, weighted=True,
         exact_blend=False):
    """-> dict(zone [B,Z,8], out [1+B], grad [B,Hp,Wp], terms_abs [B,Hp,Wp], terms_n [B,Hp,Wp], frozen, e [B,Z]); float64.
    `exact_blend`: the zone means are taken over the float64 blend instead of the float32 depths (bins, runs and weights still come from
    the float32 depths): the point at which `frozen_loss_image` evaluates, for the difference quotients."""
    B, Hp, Wp = pred.shape
    Z, bins = rect.shape[1], ZR.n_bins(max_d)
    delta = bin_width if delta is None else float(delta)
    d = np.stack([ZR.PR.depth(p, H, W, interp, lo, hi) for p in pred])
    dm = d
    if exact_blend:
        dm = np.stack([blend64(np.clip(p, np.float32(lo), np.float32(hi)).astype(np.float64), H, W, interp) for p in pred])
    zone, out, e_all = np.zeros((B, Z, 8)), np.zeros(1 + B), np.zeros((B, Z))
    grad, tabs, tn = np.zeros((B, Hp, Wp)), np.zeros((B, Hp, Wp)), np.zeros((B, Hp, Wp), np.int64)
    frozen = []
    for b in range(B):
        pix, fr = [], []
        for z in range(Z):
            mem = ZR.members(rect[b, z], H, W)
            v = d[b][mem]
            _, w, a, stop, n = zone_run(v, max_d, bins, floor, weighted)
            m = float((w[w > 0] * dm[b][mem][w > 0].astype(np.float64)).sum() / n) if n > 0 else 0.0
            measured = bool(mask[b, z])
            state = (ZR.COMPARED if n > 0 else ZR.LOST) if measured else (ZR.UNMEASURED if n > 0 else ZR.NEITHER)
            zone[b, z] = (m, n, np.nan, 0.0, a, stop, state, 0.0)
            mu_m = float(raw[b, z, 0])
            if state == ZR.COMPARED and np.isfinite(mu_m):
                r = m - mu_m
                e = max(abs(r) - bin_width / 2.0, 0.0)
                zone[b, z, R], zone[b, z, RHO], e_all[b, z] = r, huber(e, delta), e
                wz = np.zeros((H, W))
                wz[mem] = w / n
                pix.append((z, wz, e, r))
                fr.append((wz, mu_m))
        nb = len(pix)
        out[1 + b] = sum(zone[b, z, RHO] for z, _, _, _ in pix) / nb if nb else 0.0
        gd, gabs = np.zeros((H, W)), np.zeros((H, W))
        for z, wz, e, r in pix:
            coef = grad_scale * min(e / delta, 1.0) * np.sign(r) / (B * nb) if e > 0 else 0.0
            zone[b, z, COEF] = coef
            gd += coef * wz
            gabs += abs(coef) * wz
        g, _, cnt = blend_transpose(gd, Hp, Wp, interp)
        _, ga, _ = blend_transpose(gabs, Hp, Wp, interp)            # zones of opposite sign on one pixel: the terms are per zone
        with np.errstate(invalid="ignore"):
            inside = (pred[b] >= np.float32(lo)) & (pred[b] <= np.float32(hi))
        grad[b], tabs[b], tn[b] = np.where(inside, g, 0.0), np.where(inside, ga, 0.0), cnt
        frozen.append(fr)
    out[0] = out[1:].sum() / B
    return dict(zone=zone, out=out, grad=grad, terms_abs=tabs, terms_n=tn, frozen=frozen, e=e_all)


def frozen_loss_image(p64, fr, B, H, W, interp, lo, hi, delta=BIN_WIDTH, bin_width=BIN_WIDTH):
    """L_b / B of one image on a float64 prediction, the pixel weights of its compared zones frozen (`loss(...)["frozen"][b]`)."""
    d = blend64(np.clip(p64, np.float64(np.float32(lo)), np.float64(np.float32(hi))), H, W, interp)
    rho = []
    for wz, mu_m in fr:
        sel = wz != 0
        r = float((wz[sel] * d[sel]).sum()) - mu_m
        rho.append(huber(max(abs(r) - bin_width / 2.0, 0.0), delta))
    return sum(rho) / len(rho) / B if rho else 0.0


def run_args(name, floor=None):
    c = CASES[name]
    pred, rect, mask, raw = inputs(name)
    return dict(pred=pred, rect=rect, mask=mask, raw=raw, H=c["H"], W=c["W"], interp=c["interp"], lo=c["lo"], hi=c["hi"], max_d=c["max_d"],
                floor=c["floor"] if floor is None else floor)


@functools.lru_cache(maxsize=None)
def reference(name, floor=None):
    """The definition on the case's inputs at `floor` (None: the case's own), delta = bin_width, grad_scale = 1."""
    return loss(**run_args(name, floor))


def self_measurement(name, floor):
    """(mask, raw) of each image's own prediction through the sensor model at `floor`: what a perfect prediction is compared with."""
    c = CASES[name]
    pred, rect, _, _ = inputs(name)
    d = depth(name, pred)
    B, Z = rect.shape[:2]
    mask, raw = np.zeros((B, Z), np.uint8), np.zeros((B, Z, 2), np.float64)
    for b in range(B):
        for z in range(Z):
            v = d[b][ZR.members(rect[b, z], c["H"], c["W"])]
            mu, sigma, n = ZR.moments(ZR.floor_counts(v, c["max_d"], ZR.n_bins(c["max_d"]), floor))
            mask[b, z], raw[b, z] = n > 0, (mu, sigma)
    return mask, raw


def n_pix(name):
    c = CASES[name]
    _, rect, _, _ = inputs(name)
    return np.array([[int(ZR.members(r, c["H"], c["W"]).sum()) for r in rb] for rb in rect])


# ---- the same objective on a torch prediction, for autograd of the oracle ----------------------------------------------------------------

def torch_loss(pred, rect, mask, raw, H, W, lo, hi, max_d, floor, delta=BIN_WIDTH, bin_width=BIN_WIDTH):
    """L on a torch prediction [B,1,h,w] (any float dtype, may require grad): the run and the weights of every zone come from `loss` on
    the float32 cast of the prediction and are held constant; clamp, align-corners blend, zone means and penalty are torch operations,
    so autograd carries the gradient of the definition."""
    import torch
    import torch.nn.functional as F
    p32 = pred.detach().to(torch.float32).cpu().numpy()[:, 0]
    B = p32.shape[0]
    fr = loss(p32, rect, mask, raw, H, W, int(p32.shape[1:] != (H, W)), lo, hi, max_d, floor, delta=delta, bin_width=bin_width)["frozen"]
    d = torch.clamp(pred, float(np.float32(lo)), float(np.float32(hi)))
    if tuple(d.shape[-2:]) != (H, W):
        d = F.interpolate(d, size=(H, W), mode="bilinear", align_corners=True)
    total = pred.new_zeros(())
    for b in range(B):
        rho = []
        for wz, mu_m in fr[b]:
            r = (torch.from_numpy(wz).to(pred.dtype) * d[b, 0]).sum() - mu_m
            e = torch.clamp(r.abs() - bin_width / 2.0, min=0.0)
            rho.append(torch.where(e <= delta, e * e / (2.0 * delta), e - delta / 2.0))
        if rho:
            total = total + torch.stack(rho).mean()
    return total / B
