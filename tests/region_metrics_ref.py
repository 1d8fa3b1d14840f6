"""numpy restatement of the definition of `cfp_eval_metrics_regions` (include/cfpnet_hip.h) -- TEST INFRASTRUCTURE.

Segment masks from `rect`, `mask` and `edges`, then the protocols and `compute_errors` of oracle/metrics_oracle.py (pinned by the
reference's goldens) on the masked vectors.  Also the inputs the GPU tests use (`CASES`), so that the CPU tests can examine the same
tensors, and a float64-sum form of `compute_errors` that bounds what the summation order can change."""
import functools

import numpy as np

from cfpnet_amd import synthetic
from cfpnet_amd.geometry import centered_zone_rects
from oracle import metrics_oracle as MO

REGIONS = ("all", "fov_in", "fov_out", "zone_valid", "zone_invalid")
KEYS = ("a1", "a2", "a3", "abs_rel", "rmse", "log_10", "rmse_log", "silog", "sq_rel")
RTOL = 2e-5              # tests/test_metrics.py
LO, HI = 1e-3, 10.0


def fov_rect(rect, H, W):
    """`my_mask` (nyu.py:182-187) without the negative-slice wrap-around: (aa, bb, cc, dd)."""
    r = np.asarray(rect, np.float32)
    aa, bb = max(0, int(np.trunc(r[0, 0]))), max(0, int(np.trunc(r[0, 1])))
    cc, dd = min(H, int(np.trunc(r[-1, 2]))), min(W, int(np.trunc(r[-1, 3])))
    return aa, bb, cc, dd


def region_masks(rect, mask, H, W):
    """[5,H,W] bool in `REGIONS` order (validity of the ground truth not applied)."""
    r = np.asarray(rect, np.float32)
    aa, bb, cc, dd = fov_rect(r, H, W)
    fov = np.zeros((H, W), bool)
    if cc > aa and dd > bb:
        fov[aa:cc, bb:dd] = True
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    zone = np.zeros((H, W), bool)
    for z in range(r.shape[0]):
        if mask[z]:
            zone |= (r[z, 0] <= yy) & (yy < r[z, 2]) & (r[z, 1] <= xx) & (xx < r[z, 3])
    return np.stack([np.ones((H, W), bool), fov, ~fov, fov & zone, fov & ~zone])


def range_masks(gt, edges):
    """[Q,H,W] bool: q = 0 all depths, q = 1 + r the pixels whose number of edges e with gt >= e (float32) is r."""
    if len(edges) == 0:
        return np.ones((1,) + gt.shape, bool)
    idx = np.zeros(gt.shape, np.int64)
    for e in edges:
        idx += gt >= np.float32(e)
    return np.stack([np.ones(gt.shape, bool)] + [idx == r for r in range(len(edges) + 1)])


def errors_f64(g, p):
    """`compute_errors` with the same float32 per-pixel terms summed in float64."""
    g, p = g.astype(np.float32), p.astype(np.float32)
    n = float(g.size)
    th = np.maximum(g / p, p / g)
    s = lambda a: float(np.sum(a, dtype=np.float64))
    le = np.log(p) - np.log(g)
    d = g - p
    out = dict(a1=s(th < 1.25) / n, a2=s(th < 1.25 ** 2) / n, a3=s(th < 1.25 ** 3) / n, abs_rel=s(np.abs(d) / g) / n,
               rmse=np.sqrt(s(d ** 2) / n), log_10=s(np.abs(np.log10(g) - np.log10(p))) / n, rmse_log=np.sqrt(s((np.log(g) - np.log(p)) ** 2) / n))
    out["silog"] = np.sqrt(s(le ** 2) / n - (s(le) / n) ** 2) * 100
    out["sq_rel"] = s((d ** 2) / g) / n
    return {k: float(v) for k, v in out.items()}


def reference(pred, gt, lo, hi, rect, mask, edges=(), mode=0, errors=MO.compute_errors):
    """One image -> (table [5,Q,9] float64 with NaN rows for empty segments, counts [5,Q] int64)."""
    H, W = gt.shape
    proto = MO.protocol_evaluate_all if mode == 0 else MO.protocol_validate
    rm, qm = region_masks(rect, mask, H, W), range_masks(gt, edges)
    table = np.full((5, qm.shape[0], 9), np.nan)
    counts = np.zeros((5, qm.shape[0]), np.int64)
    for r in range(5):
        for q in range(qm.shape[0]):
            g, p = proto(pred.copy(), np.where(rm[r] & qm[q], gt, np.float32(np.nan)), lo, hi)     # NaN is outside lo < gt < hi
            counts[r, q] = g.size
            if g.size:
                e = errors(g, p)
                table[r, q] = [e[k] for k in KEYS]
    return table, counts


# ---- the inputs of tests/test_region_metrics_gpu.py ----------------------------------------------------------------------------------

# name: H, W, pred size, zone grid n x n of px pixels, grid shift, seed, holes, noise, drop, edges
CASES = {
    "overhang_bottom_right": dict(H=75, W=101, Hp=38, Wp=51, n=3, px=24, shift=20, seed=12, holes=0.1, noise=0.15, drop=0.34, edges=(1.0, 2.0)),
    "overhang_top_left_E7": dict(H=75, W=101, Hp=75, Wp=101, n=2, px=24, shift=-30, seed=13, holes=0.1, noise=0.15, drop=0.34,
                                 edges=(0.1, 0.3, 0.5, 0.7, 1.0, 1.5, 2.2)),
    "no_edges": dict(H=96, W=128, Hp=48, Wp=64, n=3, px=24, shift=0, seed=11, holes=0.1, noise=0.15, drop=0.34, edges=()),
    "full_size": dict(H=480, W=640, Hp=240, Wp=320, n=8, px=56, shift=0, seed=700, holes=0.1, noise=0.15, drop=0.34, edges=(2.0, 4.0)),
    # rectangles that are no grid (fractional, overlapping, one outside the image): membership by the definition alone
    "irregular": dict(H=75, W=101, Hp=38, Wp=51, n=0, px=0, shift=0, seed=16, holes=0.1, noise=0.15, drop=0.0, edges=(1.5,)),
}
IRREGULAR_RECTS = np.array([[5.5, 7.25, 30.0, 40.5], [20.0, 30.0, 50.75, 60.0], [-10.0, 80.0, 12.0, 120.0], [200.0, 200.0, 210.0, 210.0],
                            [40.0, 10.0, 70.5, 95.0]], np.float32)
IRREGULAR_MASK = np.array([1, 1, 0, 1, 1], bool)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(gt [H,W], pred [Hp,Wp], rect [Z,4] f32, mask [Z] bool, edges) -- treat as read-only."""
    c = CASES[name]
    gt, pred = synthetic.make_eval_pair(c["H"], c["W"], c["Hp"], c["Wp"], c["seed"], c["holes"], c["noise"])
    if name == "irregular":
        rect, mask = IRREGULAR_RECTS.copy(), IRREGULAR_MASK.copy()
    else:
        rect = centered_zone_rects(c["H"], c["W"], c["n"], c["px"], c["shift"])
        mask = np.random.default_rng(c["seed"]).random(c["n"] * c["n"]) >= c["drop"]
    for a in (gt, pred, rect, mask):
        a.setflags(write=False)
    return gt, pred, rect, mask, tuple(c["edges"])


@functools.lru_cache(maxsize=None)
def case_reference(name, mode):
    gt, pred, rect, mask, edges = case_inputs(name)
    table, counts = reference(pred, gt, LO, HI, rect, mask, edges, mode)
    table.setflags(write=False)
    counts.setflags(write=False)
    return table, counts


@functools.lru_cache(maxsize=None)
def batch_inputs():
    """B = 3 on the 75x101 shape: different masks per image, image 1 with every zone dropped, image 2 without a valid pixel."""
    c = CASES["overhang_bottom_right"]
    pairs = [synthetic.make_eval_pair(c["H"], c["W"], c["Hp"], c["Wp"], s, c["holes"], c["noise"]) for s in (12, 14, 15)]
    gt, pred = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    gt[2] = 0.0
    rect = np.stack([centered_zone_rects(c["H"], c["W"], c["n"], c["px"], c["shift"])] * 3)
    mask = np.stack([np.random.default_rng(40 + b).random(9) >= c["drop"] for b in range(3)])
    mask[1] = False
    for a in (gt, pred, rect, mask):
        a.setflags(write=False)
    return gt, pred, rect, mask, tuple(c["edges"])


def close(got, want, counts_got, counts_want, what=""):
    """The project's metric tolerance per entry, counts exact, NaN exactly where the segment is empty.  Returns the worst ratio to the bound."""
    assert np.array_equal(np.asarray(counts_got, np.int64), counts_want), (what, counts_got, counts_want)
    empty = counts_want == 0
    assert np.isnan(got[empty]).all() and not np.isnan(got[~empty]).any(), what
    bound = RTOL * np.maximum(np.abs(want[~empty]), 1e-3)
    ratio = np.abs(got[~empty] - want[~empty]) / bound
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{what}: worst |got - want| / bound = {worst:.3e} over {int((~empty).sum())} non-empty segments")
    assert worst <= 1.0, (what, worst)
    return worst
