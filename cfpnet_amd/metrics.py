"""Depth-evaluation metrics on the device: host-side mirror of the reference's evaluation helpers.

Reference interface: `compute_errors(gt, pred)` (`src/utils/metrics.py:4-24`), `RunningAverageDict`
(`src/utils/utils.py:14-41`) and the protocol around them in `evaluate_all.py:38-41,80-84` / `train.py:187-199`.
The arithmetic is the HIP kernel behind `cfp_eval_metrics` (`csrc/metrics.hip`); nothing here computes on the CPU.

`sparsification` / `RunningSparsification` have no counterpart in the reference: they rate the per-pixel uncertainty planes of the
model (sparsification curves, AUSE, AURG; `cfp_unc_sparsification`, `csrc/unc_metrics.hip`), again without leaving the device.

`region_metrics` / `RunningRegionAverage` split the nine metrics by where a pixel lies relative to the ToF zones (the reference's
`my_mask`, `src/dataloader/nyu.py:182-187`, and its `--zone_area_only` / `--outside_zone_area_only` flags) and by depth range
(`cfp_eval_metrics_regions`, `csrc/region_metrics.hip`).

`normal_metrics` / `RunningNormalAverage` rate the geometry: the angle between the surface normal of the prediction and that of the
ground-truth depth, both formed as `pointcloud.unproject` forms them (`cfp_normal_metrics`, `csrc/normal_metrics.hip`).

`zone_consistency` / `RunningZoneConsistency` need no ground truth: the ToF zones are re-simulated from the prediction with the sensor
model of `tof.TofSimulator` and compared with the measured (mu, sigma) per zone (`cfp_tof_zone_consistency`, `csrc/zone_consistency.hip`).

`temporal_consistency` compares two consecutive predictions after the first is warped into the second's view (`cfpnet_amd/temporal.py`).
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import hip, tof

KEYS = ("a1", "a2", "a3", "abs_rel", "rmse", "log_10", "rmse_log", "silog", "sq_rel")   # the reference's dict order
EVALUATE_ALL, VALIDATE = 0, 1


def eval_metrics(pred: torch.Tensor, gt: torch.Tensor, lo: float, hi: float, mode: int = EVALUATE_ALL,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pred [B,1,Hp,Wp] / [B,Hp,Wp] f32 at model resolution, gt [B,1,H,W] / [B,H,W] f32 -> [B,10] f64 on the device:
    the nine metrics in `KEYS` order plus the valid-pixel count.  No host synchronisation."""
    if pred.dim() == 4:
        pred = pred[:, 0]
    if gt.dim() == 4:
        gt = gt[:, 0]
    if pred.dtype != torch.float32 or gt.dtype != torch.float32 or not pred.is_cuda or not gt.is_cuda:
        raise ValueError("pred and gt must be float32 device tensors")
    pred, gt = pred.contiguous(), gt.contiguous()
    B, Hp, Wp = pred.shape
    if gt.shape[0] != B:
        raise ValueError("batch sizes differ")
    H, W = gt.shape[1:]
    # torch's bilinear kernel is not a copy at equal sizes: it reads each pixel twice with weights (1, 0), so in VALIDATE
    # order (interpolate, then clamp) an infinite prediction becomes NaN -> min_depth; that mode always interpolates
    interp = int((Hp, Wp) != (H, W) or mode == VALIDATE)
    nbytes = hip.load().cfp_eval_metrics_ws_bytes(B)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=pred.device)
    if out is None:
        out = torch.empty(B, 10, dtype=torch.float64, device=pred.device)
    hip.call("cfp_eval_metrics", pred.data_ptr(), Hp, Wp, gt.data_ptr(), H, W, B, interp, mode, lo, hi,
             ws.data_ptr(), nbytes, out.data_ptr(), hip.current_stream())
    return out


def compute_errors(gt: torch.Tensor, pred: torch.Tensor) -> Dict[str, float]:
    """Drop-in for `compute_errors(gt, pred)` on two already-masked float32 device vectors (any shape, same size)."""
    g, p = gt.reshape(1, 1, -1), pred.reshape(1, 1, -1)
    if g.numel() != p.numel() or g.numel() == 0:
        raise ValueError("gt and pred must be non-empty and the same size")
    r = eval_metrics(p, g, float("-inf"), float("inf"), mode=EVALUATE_ALL)[0].cpu().tolist()
    return dict(zip(KEYS, r[:9]))


class RunningAverageDict:
    """`RunningAverageDict` (src/utils/utils.py:27-41) over per-image metric rows kept on the device: `update` takes the
    [B,10] tensor of `eval_metrics`, skips images without valid pixels (evaluate_all.py:83) and applies the reference's
    running-mean recurrence avg <- (v + count*avg)/(count+1) image by image when the value is read."""

    def __init__(self):
        self._rows = []

    def update(self, rows: torch.Tensor) -> None:
        self._rows.append(rows)

    def get_value(self) -> Dict[str, float]:
        if not self._rows:
            return {}
        rows = torch.cat(self._rows, 0).cpu().tolist()            # the only host synchronisation
        avg, count = [0.0] * 9, 0
        for r in rows:
            if not r[9] > 0:
                continue
            avg = [(v + count * a) / (count + 1) for v, a in zip(r[:9], avg)]
            count += 1
        return dict(zip(KEYS, avg)) if count else {}


RANKINGS = ("std", "entropy", "pmax", "oracle_rmse", "oracle_absrel")   # CFP_SPARS_* order; the first three are the planes of `unc`
SPARS_METRICS = ("rmse", "absrel")


def sparsification(pred: torch.Tensor, unc: torch.Tensor, gt: torch.Tensor, lo: float, hi: float, steps: int = 20,
                   mode: int = EVALUATE_ALL, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """Sparsification curves of the three uncertainty planes against the two oracles (`cfp_unc_sparsification`, definition in
    include/cfpnet_hip.h).  pred and gt as in `eval_metrics`, unc [B,3,Hp,Wp] f32 at the prediction's resolution ->
    {"curves": [B,5,2,K] f64 (ranking in `RANKINGS` order, metric rmse / absrel, point k removes floor(k*N/K) pixels),
     "ause": [B,3,2], "aurg": [B,3,2], "n_valid": [B]} on the device.  `out` is a dict of a previous call to write into.
    No host synchronisation."""
    if pred.dim() == 4:
        pred = pred[:, 0]
    if gt.dim() == 4:
        gt = gt[:, 0]
    if pred.dtype != torch.float32 or gt.dtype != torch.float32 or not pred.is_cuda or not gt.is_cuda:
        raise ValueError("pred and gt must be float32 device tensors")
    if unc.dtype != torch.float32 or not unc.is_cuda:
        raise ValueError("unc must be a float32 device tensor")
    pred, gt, unc = pred.contiguous(), gt.contiguous(), unc.contiguous()
    B, Hp, Wp = pred.shape
    if gt.shape[0] != B:
        raise ValueError("batch sizes differ")
    if tuple(unc.shape) != (B, 3, Hp, Wp):
        raise ValueError(f"unc must be [B,3,Hp,Wp] = {(B, 3, Hp, Wp)}, got {tuple(unc.shape)}")
    H, W = gt.shape[1:]
    K = int(steps)
    interp = int((Hp, Wp) != (H, W) or mode == VALIDATE)     # the rule of eval_metrics
    nbytes = hip.load().cfp_unc_sparsification_ws_bytes(B, H, W, K)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=pred.device)
    if out is None:
        out = {"curves": torch.empty(B, 5, 2, max(K, 0), dtype=torch.float64, device=pred.device),
               "summary": torch.empty(B, 3, 2, 2, dtype=torch.float64, device=pred.device),
               "n_valid": torch.empty(B, dtype=torch.float64, device=pred.device)}
    hip.call("cfp_unc_sparsification", pred.data_ptr(), unc.data_ptr(), Hp, Wp, gt.data_ptr(), H, W, B, interp, mode, lo, hi, K,
             ws.data_ptr(), nbytes, out["curves"].data_ptr(), out["summary"].data_ptr(), out["n_valid"].data_ptr(),
             hip.current_stream())
    out["ause"], out["aurg"] = out["summary"][..., 0], out["summary"][..., 1]
    return out


class RunningSparsification:
    """Per-image means of the sparsification curves, AUSE and AURG over a data set: `update` takes the dict of `sparsification`
    and keeps the rows on the device; `get_value` synchronises once, skips images without valid pixels or with NaN rows and returns
    {"ause_rmse_std": ..., "ause_absrel_std": ..., ..., "aurg_absrel_pmax": ..., "curves": [5][2][K] nested lists}."""

    def __init__(self):
        self._rows = []

    def update(self, res: Dict[str, torch.Tensor]) -> None:
        B = res["n_valid"].shape[0]
        self._rows.append(torch.cat([res["n_valid"].reshape(B, 1), res["summary"].reshape(B, 12), res["curves"].reshape(B, -1)], 1))

    def get_value(self) -> Dict[str, object]:
        if not self._rows:
            return {}
        rows = torch.cat(self._rows, 0).cpu()                    # the only host synchronisation
        keep = (rows[:, 0] > 0) & ~torch.isnan(rows).any(1)
        if not bool(keep.any()):
            return {}
        mean = rows[keep].mean(0).tolist()
        res: Dict[str, object] = {}
        for a, name in enumerate(("ause", "aurg")):
            for m, metric in enumerate(SPARS_METRICS):
                for u, plane in enumerate(RANKINGS[:3]):
                    res[f"{name}_{metric}_{plane}"] = mean[1 + (u * 2 + m) * 2 + a]
        K = (len(mean) - 13) // 10
        res["curves"] = [[mean[13 + (r * 2 + m) * K: 13 + (r * 2 + m + 1) * K] for m in range(2)] for r in range(5)]
        return res


REGIONS = ("all", "fov_in", "fov_out", "zone_valid", "zone_invalid")     # CFP_REGION_* order
MAX_RANGE_EDGES = 7


def range_labels(range_edges: Sequence[float] = ()) -> Tuple[str, ...]:
    """Labels of the range axis of `region_metrics`: () -> ("all",); (2, 4) -> ("all", "<2", "2-4", ">=4")."""
    e = [f"{float(v):g}" for v in range_edges]
    if not e:
        return ("all",)
    return ("all", f"<{e[0]}") + tuple(f"{a}-{b}" for a, b in zip(e[:-1], e[1:])) + (f">={e[-1]}",)


def region_metrics(pred: torch.Tensor, gt: torch.Tensor, lo: float, hi: float, rect_data: torch.Tensor, mask: torch.Tensor,
                   range_edges: Sequence[float] = (), mode: int = EVALUATE_ALL, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The metrics of `eval_metrics` per region and depth range (`cfp_eval_metrics_regions`, definition in include/cfpnet_hip.h).
    pred and gt as in `eval_metrics`; rect_data [B,Z,4] f32 (sy, sx, ey, ex) and mask [B,Z] bool / uint8 on the device, as the model
    receives them; range_edges: up to 7 finite, strictly increasing depths in metres -> [B,5,Q,10] f64 on the device, regions in
    `REGIONS` order, ranges in `range_labels(range_edges)` order (Q = 1 without edges), then the nine metrics in `KEYS` order and
    the pixel count; a segment without a valid pixel holds NaN metrics and count 0.  No host synchronisation."""
    if pred.dim() == 4:
        pred = pred[:, 0]
    if gt.dim() == 4:
        gt = gt[:, 0]
    if pred.dtype != torch.float32 or gt.dtype != torch.float32 or not pred.is_cuda or not gt.is_cuda:
        raise ValueError("pred and gt must be float32 device tensors")
    if rect_data.dtype != torch.float32 or not rect_data.is_cuda or mask.dtype not in (torch.bool, torch.uint8) or not mask.is_cuda:
        raise ValueError("rect_data must be a float32 and mask a bool / uint8 device tensor")
    if pred.dim() != 3 or gt.dim() != 3:
        raise ValueError("pred and gt must be [B,H,W] or [B,1,H,W]")
    pred, gt, rect_data, mask = pred.contiguous(), gt.contiguous(), rect_data.contiguous(), mask.contiguous()
    B, Hp, Wp = pred.shape
    if gt.shape[0] != B:
        raise ValueError("batch sizes differ")
    if rect_data.dim() != 3 or rect_data.shape[0] != B or rect_data.shape[2] != 4 or rect_data.shape[1] < 1:
        raise ValueError(f"rect_data must be [B,Z,4] with B = {B}, got {tuple(rect_data.shape)}")
    Z = rect_data.shape[1]
    if tuple(mask.shape) != (B, Z):
        raise ValueError(f"mask must be [B,Z] = {(B, Z)}, got {tuple(mask.shape)}")
    edges = [float(v) for v in range_edges]
    E = len(edges)
    if E > MAX_RANGE_EDGES:
        raise ValueError(f"at most {MAX_RANGE_EDGES} range edges, got {E}")
    Q = 1 if E == 0 else E + 2
    H, W = gt.shape[1:]
    interp = int((Hp, Wp) != (H, W) or mode == VALIDATE)     # the rule of eval_metrics
    nbytes = hip.load().cfp_eval_metrics_regions_ws_bytes(B)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=pred.device)
    if out is None:
        out = torch.empty(B, 5, Q, 10, dtype=torch.float64, device=pred.device)
    elif tuple(out.shape) != (B, 5, Q, 10) or out.dtype != torch.float64 or not out.is_cuda or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float64 device tensor {(B, 5, Q, 10)}")
    host_edges = (ctypes.c_float * max(E, 1))(*edges)      # the one host pointer of the call: copied into the kernel arguments
    hip.call("cfp_eval_metrics_regions", pred.data_ptr(), Hp, Wp, gt.data_ptr(), H, W, B, interp, mode, lo, hi, rect_data.data_ptr(),
             mask.data_ptr(), Z, host_edges, E, ws.data_ptr(), nbytes, out.data_ptr(), hip.current_stream())
    return out


class RunningRegionAverage:
    """`RunningAverageDict` per (region, range): `update` takes the [B,5,Q,10] tensor of `region_metrics` and keeps it on the device;
    `get_value` synchronises once and applies the reference's recurrence avg <- (v + count*avg)/(count+1) image by image, skipping
    -- for that segment only -- the images whose count there is 0 (evaluate_all.py:83).  It returns
    {region: {range label: {metric: mean}}} with an empty dict for a segment no image contributed to; `image_counts` then holds
    {region: {range label: number of images averaged}}."""

    def __init__(self, range_edges: Sequence[float] = ()):
        self.labels = range_labels(range_edges)
        self.image_counts: Dict[str, Dict[str, int]] = {}
        self._rows = []

    def update(self, rows: torch.Tensor) -> None:
        if rows.dim() != 4 or tuple(rows.shape[1:]) != (5, len(self.labels), 10):
            raise ValueError(f"rows must be [B,5,{len(self.labels)},10], got {tuple(rows.shape)}")
        self._rows.append(rows)

    def get_value(self) -> Dict[str, Dict[str, Dict[str, float]]]:
        if not self._rows:
            return {}
        rows = torch.cat(self._rows, 0).cpu().tolist()            # the only host synchronisation
        res: Dict[str, Dict[str, Dict[str, float]]] = {}
        self.image_counts = {}
        for ri, region in enumerate(REGIONS):
            res[region], self.image_counts[region] = {}, {}
            for qi, label in enumerate(self.labels):
                avg, count = [0.0] * 9, 0
                for img in rows:
                    r = img[ri][qi]
                    if not r[9] > 0:
                        continue
                    avg = [(v + count * a) / (count + 1) for v, a in zip(r[:9], avg)]
                    count += 1
                res[region][label] = dict(zip(KEYS, avg)) if count else {}
                self.image_counts[region][label] = count
        return res


NORMAL_METRIC_NAMES = ("mean_deg", "median_deg", "rmse_deg", "frac_11_25", "frac_22_5", "frac_30")   # CFP_NORMAL_* order; column 6 is n_valid
NORMAL_BINS = 1800                                    # bins of 0.1 degree


def normal_metrics(pred: torch.Tensor, gt: torch.Tensor, lo: float, hi: float, intrinsics=None, size=None, hist: bool = False,
                   angle_map: bool = False):
    """Surface-normal error of the prediction against the ground truth (`cfp_normal_metrics`, definition in include/cfpnet_hip.h).
    pred and gt as in `eval_metrics`, in EVALUATE_ALL order; `intrinsics`: (fx, fy, cx, cy) in pixels of the ground-truth grid -- host
    numbers, used for every image -- or a float32 [B,4] tensor, `pointcloud.ZJUL5_INTRINSICS` by default; `size` = (H, W), if given, must
    be the ground truth's -> [B,7] f64 on the device: the six metrics in `NORMAL_METRIC_NAMES` order and the valid-pixel count.  With
    `hist` and / or `angle_map` a tuple: the rows, then the histogram [B,1800] i32 (bins of 0.1 degree), then the angle per pixel
    [B,H,W] f32 in degrees (NaN where the pixel is not valid), whichever were asked for.  No host synchronisation."""
    from . import pointcloud
    if not isinstance(gt, torch.Tensor) or gt.dtype != torch.float32 or not gt.is_cuda:
        raise ValueError("gt must be a float32 device tensor")
    pred = pointcloud._pred3(pred)
    if gt.dim() == 4 and gt.shape[1] == 1:
        gt = gt[:, 0]
    if gt.dim() != 3 or min(gt.shape) < 1:
        raise ValueError(f"gt must be [B,H,W] or [B,1,H,W], got {tuple(gt.shape)}")
    gt = gt.contiguous()
    B, Hp, Wp = pred.shape
    if gt.shape[0] != B:
        raise ValueError("batch sizes differ")
    H, W = gt.shape[1:]
    if size is not None and pointcloud._size(size, Hp, Wp) != (H, W):
        raise ValueError(f"size must be the ground truth's {(H, W)}, got {tuple(size)}")
    if not float(lo) < float(hi):
        raise ValueError(f"empty depth range [{lo}, {hi}]")
    K = pointcloud._intrinsics(pointcloud.ZJUL5_INTRINSICS if intrinsics is None else intrinsics, B, pred.device)
    interp = int((Hp, Wp) != (H, W))                      # the rule of eval_metrics in EVALUATE_ALL order
    nbytes = hip.load().cfp_normal_metrics_ws_bytes(B, H, W)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=pred.device)
    out = torch.empty(B, 7, dtype=torch.float64, device=pred.device)
    h = torch.empty(B, NORMAL_BINS, dtype=torch.int32, device=pred.device) if hist else None
    amap = torch.empty(B, H, W, dtype=torch.float32, device=pred.device) if angle_map else None
    hip.call("cfp_normal_metrics", pred.data_ptr(), Hp, Wp, gt.data_ptr(), H, W, B, interp, float(lo), float(hi), K.data_ptr(),
             ws.data_ptr(), nbytes, out.data_ptr(), hip.ptr(h), hip.ptr(amap), hip.current_stream())
    if not hist and not angle_map:
        return out
    return (out,) + ((h,) if hist else ()) + ((amap,) if angle_map else ())


class RunningNormalAverage:
    """Means of the normal metrics over a data set: `update` takes the [B,7] rows of `normal_metrics` (and optionally the [B,1800]
    histograms) and keeps them on the device; `get_value` synchronises once and returns the plain means of the six metrics over the
    images with n_valid > 0 plus "images", their number; `histogram` is the sum of the histograms given, as a list of 1800 ints."""

    def __init__(self):
        self._rows, self._hist = [], None

    def update(self, rows: torch.Tensor, hist: Optional[torch.Tensor] = None) -> None:
        if rows.dim() != 2 or rows.shape[1] != 7:
            raise ValueError(f"rows must be [B,7], got {tuple(rows.shape)}")
        self._rows.append(rows)
        if hist is not None:
            h = hist.to(torch.int64).sum(0)
            self._hist = h if self._hist is None else self._hist + h

    def get_value(self) -> Dict[str, float]:
        if not self._rows:
            return {}
        rows = [r for r in torch.cat(self._rows, 0).cpu().tolist() if r[6] > 0]      # the only host synchronisation
        if not rows:
            return {}
        res = {k: sum(r[i] for r in rows) / len(rows) for i, k in enumerate(NORMAL_METRIC_NAMES)}
        res["images"] = len(rows)
        return res

    def histogram(self):
        return [0] * NORMAL_BINS if self._hist is None else self._hist.cpu().tolist()


ZONE_CONSISTENCY_NAMES = ("n_compared", "mae_mu", "rmse_mu", "rel_mu", "mae_sigma", "frac_1bin", "frac_window", "n_lost", "n_unmeasured",
                          "n_measured")                # CFP_ZONE_* order
ZONE_COLUMNS = ("mu_p", "sigma_p", "n_signal", "n_pix", "n_window", "state")
ZONE_STATES = ("compared", "lost", "unmeasured", "neither")


def zone_consistency(pred: torch.Tensor, raw_data: torch.Tensor, rect_data: torch.Tensor, mask: torch.Tensor, lo: float, hi: float,
                     size=None, max_distance: float = 4.0, floor_count: int = tof.AMBIENT_FLOOR, dev_map: bool = False):
    """The ToF zones re-simulated from the prediction against what the sensor measured (`cfp_tof_zone_consistency`, definition in
    include/cfpnet_hip.h): the check that needs no ground truth.  pred [B,h,w] / [B,1,h,w] f32 on the device; raw_data [B,Z,2] the
    measured (mu, sigma) per zone (a rig's `raw_data`, or the `fh` of `tof.TofSimulator.simulate`; converted to float64), rect_data
    [B,Z,4] f32 (sy, sx, ey, ex) in pixels of the H x W grid and mask [B,Z] bool / uint8, all on the device; `size` = (H, W), twice the
    prediction by default; `max_distance` the distance the measurement was made with (bins = int(max_distance / tof.BIN_WIDTH));
    `floor_count` the ambient floor of the sensor model ->(summary [B,10] f64 in `ZONE_CONSISTENCY_NAMES` order, zone
    [B,Z,6] f64 in `ZONE_COLUMNS` order), and with `dev_map` a third tensor [B,H,W] f32: the prediction minus the measured mu of the
    first measured zone that contains the pixel, NaN outside.  No host synchronisation."""
    pred, raw, rect, mk, B, Hp, Wp, H, W, Z, md, bins, interp = tof.zone_inputs(pred, raw_data, rect_data, mask, lo, hi, size, max_distance)
    summary = torch.empty(B, 10, dtype=torch.float64, device=pred.device)
    zone = torch.empty(B, Z, 6, dtype=torch.float64, device=pred.device)
    dmap = torch.empty(B, H, W, dtype=torch.float32, device=pred.device) if dev_map else None
    hip.call("cfp_tof_zone_consistency", pred.data_ptr(), Hp, Wp, H, W, B, interp, float(lo), float(hi), rect.data_ptr(), mk.data_ptr(),
             raw.data_ptr(), Z, md, bins, tof.BIN_WIDTH, int(floor_count), zone.data_ptr(), summary.data_ptr(), hip.ptr(dmap), hip.current_stream())
    return (summary, zone, dmap) if dev_map else (summary, zone)


class RunningZoneConsistency:
    """Means of the zone-consistency summary over a data set: `update` takes the [B,10] rows of `zone_consistency` (and optionally the
    [B,Z,6] zone tables) and keeps them on the device; `get_value` synchronises once and returns the plain means of the ten columns
    over the images with n_compared > 0 (NaN entries, such as frac_window of an image without measured pixels, are left out of that
    column's mean) plus "images", their number; `tables` is the list of per-image zone tables given, as nested lists."""

    def __init__(self):
        self._rows, self._zones = [], []

    def update(self, rows: torch.Tensor, zone: Optional[torch.Tensor] = None) -> None:
        if rows.dim() != 2 or rows.shape[1] != 10:
            raise ValueError(f"rows must be [B,10], got {tuple(rows.shape)}")
        self._rows.append(rows)
        if zone is not None:
            self._zones.append(zone)

    def get_value(self) -> Dict[str, float]:
        if not self._rows:
            return {}
        rows = [r for r in torch.cat(self._rows, 0).cpu().tolist() if r[0] > 0]      # the only host synchronisation
        if not rows:
            return {}
        res = {}
        for i, k in enumerate(ZONE_CONSISTENCY_NAMES):
            v = [r[i] for r in rows if r[i] == r[i]]
            res[k] = sum(v) / len(v) if v else float("nan")
        res["images"] = len(rows)
        return res

    def tables(self):
        return [t for z in self._zones for t in z.cpu().tolist()]


TEMPORAL_CONSISTENCY_NAMES = ("mean_abs", "rmse", "coverage")


def temporal_consistency(prev: torch.Tensor, cur: torch.Tensor, intrinsics, pose, lo: float, hi: float, size=None) -> torch.Tensor:
    """How well two consecutive predictions agree once the first is carried into the second's view: `prev`, `cur` [B,h,w] /
    [B,1,h,w] f32 on the device, `intrinsics` and `size` as in `pointcloud.unproject`, `pose` = [R|t] from the previous camera frame to
    the current one (None: the camera did not move) -> [B,3] f64 in `TEMPORAL_CONSISTENCY_NAMES` order: the mean |difference| and the
    RMSE in metres over the pixels of the H x W grid where the warped `prev` and `cur` are both known, and the share of the grid the
    warped `prev` covers.  A thin wrapper over `temporal.reproject` and `temporal.fuse` (its `stats` and `counts`); NaN for an image
    without a common pixel.  No host synchronisation."""
    from . import temporal
    warped, _ = temporal.reproject(prev, intrinsics, pose, size=size, lo=lo, hi=hi, splat=1)
    B, H, W = warped.shape
    one = torch.ones(B, 1, 1, dtype=torch.float32, device=warped.device)      # the gate and the variances play no part in `stats`
    _, _, counts, stats = temporal.fuse(cur, one, warped, torch.zeros_like(warped), lo=lo, hi=hi)
    n = (counts[:, 1] + counts[:, 2]).to(torch.float64)                       # fused + rejected: both known
    return torch.stack([stats[:, 0] / n, torch.sqrt(stats[:, 1] / n), counts[:, 0].to(torch.float64) / float(H * W)], 1)
