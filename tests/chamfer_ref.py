"""Reference statements of the bin-centre chamfer loss (include/cfpnet_hip.h, cfp_bins_chamfer) for the tests, all on the CPU:

  chamfer_ref      brute force in torch (float64 or float32), autograd for the gradient w.r.t. the centres
  interval_scheme  the kernel's scheme in numpy float64: interval by binary search, per-centre sum of d, per-interval min / max,
                   prefix-max / suffix-min scans that step over empty intervals
  tie_margins      how far the case is from the two kinds of tie (the GPU tests assert on it before they compare)
  CASES / make_case  the case table: shapes, how the targets are drawn, and seeds chosen on the CPU so that no case sits near a tie

    L_b = (1/P) sum_p min_t (c_p - t)^2 + (1/N_b) sum_t min_p (c_p - t)^2,   L = (1/B) sum_b L_b,   N_b = 0: L_b = 0
"""
import numpy as np
import torch

MIN_VAL, MAX_VAL = 1e-3, 10.0


def centers_of(edges: torch.Tensor) -> torch.Tensor:
    """float32 centres, as the model and the kernel form them: 0.5f * (e_p + e_{p+1})."""
    e = edges.float()
    return 0.5 * (e[:, :-1] + e[:, 1:])


def valid_targets(target: torch.Tensor, mask, b: int) -> torch.Tensor:
    t = target[b].reshape(-1).float()
    keep = (mask[b].reshape(-1) != 0) if mask is not None else (t >= 1e-3)
    return torch.sort(t[keep]).values          # ascending: the first of equal distances is the lower target


def _argmin_rows(a: torch.Tensor, t: torch.Tensor, chunk: int = 1 << 15):
    """For every a_i the index of the nearest t_j (first one on a tie), without the whole |a| x |t| matrix at once."""
    best = torch.full((a.numel(),), float("inf"), dtype=a.dtype)
    arg = torch.zeros(a.numel(), dtype=torch.long)
    for s in range(0, t.numel(), chunk):
        d = (a[:, None] - t[None, s:s + chunk]) ** 2
        v, i = d.min(dim=1)
        upd = v < best                         # strict: an earlier (lower) index keeps a tie
        best = torch.where(upd, v, best)
        arg = torch.where(upd, i + s, arg)
    return arg


def chamfer_of_centers(c: torch.Tensor, target: torch.Tensor, mask=None):
    """Brute force on centres c [B,P] in c's dtype, differentiable in c (the nearest neighbours are found without a graph, the
    distances to them are formed with one) -> (L, L_b [B])."""
    B, P = c.shape
    per = []
    for b in range(B):
        t = valid_targets(target, mask, b).to(c.dtype)
        if t.numel() == 0:
            per.append(c[b].sum() * 0.0)
            continue
        with torch.no_grad():
            near_t = _argmin_rows(c[b].detach(), t)          # per centre: its nearest target
            near_c = _argmin_rows(t, c[b].detach())          # per target: its nearest centre
        per.append(((c[b] - t[near_t]) ** 2).sum() / P + ((c[b][near_c] - t) ** 2).sum() / t.numel())
    per = torch.stack(per)
    return per.sum() / B, per


def chamfer_ref(edges: torch.Tensor, target: torch.Tensor, mask=None, dtype=torch.float64):
    """-> (L, L_b [B], dL/dc [B, P]) in `dtype`, by brute force (every centre against every target) and autograd."""
    c = centers_of(edges).to(dtype).clone().requires_grad_(True)
    L, per = chamfer_of_centers(c, target, mask)
    L.backward()
    return L.detach(), per.detach(), c.grad.detach()


def interval_scheme(edges, target, mask=None):
    """The kernel's scheme, float64 numpy.  edges [B,P+1], target [B,1,H,W] (numpy or torch) -> (L, L_b [B], dL/dc [B,P])."""
    edges = np.asarray(edges, dtype=np.float32)
    target = np.asarray(target, dtype=np.float32)
    B, P = edges.shape[0], edges.shape[1] - 1
    Lb, grad = np.zeros(B), np.zeros((B, P))
    for b in range(B):
        c = (np.float32(0.5) * (edges[b, :-1] + edges[b, 1:])).astype(np.float64)
        t = target[b].reshape(-1)
        keep = (np.asarray(mask[b]).reshape(-1) != 0) if mask is not None else (t >= np.float32(1e-3))
        t = t[keep].astype(np.float64)
        N = t.size
        if N == 0:
            continue
        k = np.searchsorted(c, t, side="right")                   # interval: c[k-1] <= t < c[k], k = 0..P
        lo, hi = np.clip(k - 1, 0, P - 1), np.clip(k, 0, P - 1)
        nn = np.where((k > 0) & (k < P) & (t - c[lo] > c[hi] - t), hi, lo)      # tie: the lower index
        d = t - c[nn]
        sum_d = np.zeros(P)
        np.add.at(sum_d, nn, d)
        imax, imin = np.full(P + 1, -np.inf), np.full(P + 1, np.inf)            # empty interval = the scans' identities
        np.maximum.at(imax, k, t)
        np.minimum.at(imin, k, t)
        below = np.maximum.accumulate(imax)[:P]                   # largest target < c_p: intervals 0..p
        above = np.minimum.accumulate(imin[::-1])[::-1][1:]       # smallest target >= c_p: intervals p+1..P
        dl, dh = c - below, above - c
        diff = np.where(np.isfinite(dl) & (~np.isfinite(dh) | (dl <= dh)), dl, -dh)      # c_p - near_p; tie: the lower target
        Lb[b] = (diff ** 2).sum() / P + (d ** 2).sum() / N
        grad[b] = (2.0 * diff / P - 2.0 * sum_d / N) / B
    return Lb.sum() / B, Lb, grad


def tie_margins(edges: torch.Tensor, target: torch.Tensor, mask=None):
    """(a, b): a = the least distance of a valid target from a midpoint between adjacent centres; b = the least | (c - lower) - (upper - c) |
    over the centres that have a target on both sides.  inf where there is nothing to tie."""
    c64 = centers_of(edges).double()
    a = b_ = float("inf")
    for b in range(edges.shape[0]):
        t = valid_targets(target, mask, b).double()
        if t.numel() == 0:
            continue
        c = c64[b]
        if c.numel() > 1:
            mid = 0.5 * (c[:-1] + c[1:])
            j = torch.searchsorted(t, mid).clamp(1, t.numel() - 1) if t.numel() > 1 else torch.zeros_like(mid, dtype=torch.long)
            a = min(a, float(torch.minimum((t[j] - mid).abs(), (t[(j - 1).clamp(min=0)] - mid).abs()).min()))
        j = torch.searchsorted(t, c)                     # t[j-1] < c <= t[j]
        both = (j > 0) & (j < t.numel())
        if bool(both.any()):
            jj = j[both]
            b_ = min(b_, float(((c[both] - t[jj - 1]) - (t[jj] - c[both])).abs().min()))
    return a, b_


def edges_from_widths(wn: np.ndarray, min_val: float = MIN_VAL, max_val: float = MAX_VAL) -> np.ndarray:
    """cfp_bin_centers' edges on the CPU, float32 operation by operation: e_0 = min_val, e_{k+1} = e_k + (max_val - min_val) * wn_k."""
    wn = np.asarray(wn, dtype=np.float32)
    lo, span = np.float32(min_val), np.float32(max_val) - np.float32(min_val)
    e = np.empty((wn.shape[0], wn.shape[1] + 1), dtype=np.float32)
    e[:, 0] = lo
    for k in range(wn.shape[1]):
        e[:, k + 1] = e[:, k] + span * wn[:, k]
    return e


# name -> (B, H, W, P, kind, seed).  Seeds were chosen on the CPU (tie_margins > 1e-5 on both counts for every case).
CASES = {
    "odd_tail_wave": (3, 13, 17, 5, "mask", 0),
    "p80": (2, 37, 41, 80, "mask", 1),
    "p256": (2, 37, 41, 256, "mask", 104),
    "p1": (2, 9, 11, 1, "mask", 0),
    "p1024": (2, 23, 29, 1024, "sparse", 51),
    "empty_middle_image": (3, 13, 17, 16, "empty_middle", 0),
    "all_below_c0": (2, 13, 17, 16, "below", 0),
    "all_above_clast": (2, 13, 17, 16, "above", 0),
    "all_in_one_bin": (2, 13, 17, 16, "one_bin", 0),
    "null_mask_straddles_1e-3": (2, 13, 17, 16, "null_mask", 0),
    "one_416x544_image": (1, 416, 544, 256, "big", 7),
}


def make_case(name: str, seed=None):
    """-> (wn [B,P] float32 normalised widths, target [B,1,H,W] float32, mask [B,1,H,W] bool or None), all torch CPU tensors.
    The edges are cfp_bin_centers(wn, MIN_VAL, MAX_VAL) (`edges_from_widths` on the CPU)."""
    B, H, W, P, kind, s0 = CASES[name]
    rng = np.random.default_rng(1000 * (list(CASES).index(name) + 1) + (s0 if seed is None else seed))
    w = rng.random((B, P), dtype=np.float32) + np.float32(0.1)
    wn = (w / w.sum(1, keepdims=True)).astype(np.float32)
    e = edges_from_widths(wn)
    t = (0.3 + 9.5 * rng.random((B, 1, H, W))).astype(np.float32)
    mask = rng.random((B, 1, H, W)) < 0.8
    if kind == "sparse":
        mask = rng.random((B, 1, H, W)) < 0.25
    elif kind == "empty_middle":
        mask[1] = False
    elif kind == "below":                                  # every target under the first centre (> MIN_VAL + half a first bin)
        c0 = 0.5 * (e[:, 0] + e[:, 1])
        t = (MIN_VAL + (c0[:, None, None, None] - MIN_VAL) * (0.05 + 0.9 * rng.random((B, 1, H, W)))).astype(np.float32)
    elif kind == "above":
        t = (MAX_VAL + 0.5 + 1.5 * rng.random((B, 1, H, W))).astype(np.float32)
    elif kind == "one_bin":                                # strictly inside bin 7 of each image
        lo, hi = e[:, 7, None, None, None], e[:, 8, None, None, None]
        t = (lo + (hi - lo) * (0.02 + 0.96 * rng.random((B, 1, H, W)))).astype(np.float32)
    elif kind == "null_mask":
        small = rng.choice(np.array([0.0, 5e-4, 9.9e-4, 1.01e-3, 1.5e-3], dtype=np.float32), size=(B, 1, H, W))
        t = np.where(rng.random((B, 1, H, W)) < 0.4, small, t).astype(np.float32)
        mask = None
    elif kind == "big":                                    # a few hundred distinct depths: dense continuous targets would tie somewhere
        t = (np.floor(t * 64.0) / 64.0 + 0.003).astype(np.float32)
        t[rng.random((B, 1, H, W)) < 0.1] = 0.0            # holes
        mask = t > 1e-3
    return torch.from_numpy(wn), torch.from_numpy(t), (torch.from_numpy(mask) if mask is not None else None)
