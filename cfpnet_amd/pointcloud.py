"""From the depth map to 3-D points on the device: the step after the model for whoever consumes ToF depth completion.

`unproject` turns the half-resolution prediction into an organised point map in the camera frame (and surface normals) at full
resolution: the depth at a pixel is the value `metrics.eval_metrics` evaluates there (the `np.clip` -> bilinear protocol of
`evaluate_all.py:40-41`, one implementation in `csrc/metrics_pred.h`), back-projected with the pinhole intrinsics the reference's ZJU-L5
loader carries and never uses (`src/dataloader/zjuL5.py:66-71`).  `point_cloud` adds the selection a consumer wants -- a grid stride,
a depth range, an interval of one of the model's uncertainty planes -- as an order-preserving compaction without a host
synchronisation; `write_ply` stores a cloud.  The arithmetic is `cfp_depth_unproject` / `cfp_points_compact` (`csrc/pointcloud.hip`,
definition in include/cfpnet_hip.h); nothing here computes on the CPU except the PLY writer.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import hip

ZJUL5_INTRINSICS = (611.2, 609.6, 323.4, 244.9)     # fx, fy, cx, cy of the 480 x 640 colour image (zjuL5.py:66-71)


def _pred3(pred: torch.Tensor) -> torch.Tensor:
    if not isinstance(pred, torch.Tensor) or pred.dtype != torch.float32 or not pred.is_cuda:
        raise ValueError("pred must be a float32 device tensor")
    if pred.dim() == 4 and pred.shape[1] == 1:
        pred = pred[:, 0]
    if pred.dim() != 3 or min(pred.shape) < 1:
        raise ValueError(f"pred must be [B,h,w] or [B,1,h,w], got {tuple(pred.shape)}")
    return pred.contiguous()


def _intrinsics(intrinsics, B: int, device) -> torch.Tensor:
    """-> [B,4] float32 on the device.  Host numbers are validated; a device tensor cannot be without a synchronisation."""
    if isinstance(intrinsics, torch.Tensor):
        if intrinsics.dtype != torch.float32 or tuple(intrinsics.shape) != (B, 4):
            raise ValueError(f"intrinsics tensor must be float32 [B,4] = {(B, 4)}, got {intrinsics.dtype} {tuple(intrinsics.shape)}")
        return intrinsics.to(device).contiguous()
    try:
        k = [float(v) for v in intrinsics]
    except TypeError:
        raise ValueError("intrinsics must be (fx, fy, cx, cy) or a [B,4] tensor") from None
    if len(k) != 4:
        raise ValueError(f"intrinsics must be (fx, fy, cx, cy), got {len(k)} values")
    if not all(math.isfinite(v) for v in k) or k[0] == 0.0 or k[1] == 0.0:
        raise ValueError(f"intrinsics must be finite with fx, fy != 0, got {tuple(k)}")
    return torch.tensor([k] * B, dtype=torch.float32).to(device)


def _size(size, h: int, w: int) -> Tuple[int, int]:
    if size is None:
        return 2 * h, 2 * w                           # the model's output-to-input ratio
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be (H, W), got {size!r}") from None
    if H < 1 or W < 1:
        raise ValueError(f"size must be positive, got {(H, W)}")
    return H, W


def _check_out(t, shape, dtype, what):
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {dtype} device tensor {tuple(shape)}")
    return t


def unproject(pred: torch.Tensor, intrinsics, size: Optional[Sequence[int]] = None, lo: float = 1e-3, hi: float = 10.0,
              normals: bool = False, out=None):
    """pred [B,h,w] / [B,1,h,w] f32 on the device -> points [B,H,W,3] f32 in the camera frame, or (points, normals) with
    `normals=True` (`cfp_depth_unproject`).  `intrinsics`: (fx, fy, cx, cy) in pixels of the H x W grid -- host numbers, used for every
    image -- or a float32 [B,4] tensor (finite, fx and fy not 0: the caller's contract).  `size` = (H, W), twice the prediction by
    default.  `out`: the tensor (or the pair) of an earlier call to write into.  No host synchronisation."""
    pred = _pred3(pred)
    B, h, w = pred.shape
    H, W = _size(size, h, w)
    if not float(lo) < float(hi):
        raise ValueError(f"empty depth range [{lo}, {hi}]")
    K = _intrinsics(intrinsics, B, pred.device)
    if out is not None:
        if normals and (not isinstance(out, (tuple, list)) or len(out) != 2):
            raise ValueError("out must be (points, normals) when normals=True")
        pts, nrm = out if normals else (out, None)
        _check_out(pts, (B, H, W, 3), torch.float32, "out points")
        if normals:
            _check_out(nrm, (B, H, W, 3), torch.float32, "out normals")
    else:
        pts = torch.empty(B, H, W, 3, dtype=torch.float32, device=pred.device)
        nrm = torch.empty(B, H, W, 3, dtype=torch.float32, device=pred.device) if normals else None
    interp = int((h, w) != (H, W))                    # the rule of metrics.eval_metrics in EVALUATE_ALL order
    hip.call("cfp_depth_unproject", pred.data_ptr(), h, w, H, W, B, interp, float(lo), float(hi), K.data_ptr(), pts.data_ptr(),
             hip.ptr(nrm), hip.current_stream())
    return (pts, nrm) if normals else pts


class PointCloud:
    """Result of `point_cloud`, everything on the device: `points` [B,cap,3] f32, `normals` [B,cap,3] f32 or None, `index` [B,cap]
    i32 (y * W + x of the pixel a row came from), `colors` [B,cap,3] or None, `counts` [B] i32 -- the number of pixels kept per image,
    also when it exceeds `capacity`.  Rows at or beyond min(count, capacity) hold nothing of meaning."""

    def __init__(self, points, normals, index, colors, counts, capacity: int, size: Tuple[int, int]):
        self.points, self.normals, self.index, self.colors, self.counts = points, normals, index, colors, counts
        self.capacity, self.size = capacity, size

    def split(self) -> List[dict]:
        """The one host synchronisation: per image {"points": [n,3], "normals", "index", "colors"} trimmed to its count (None where
        absent).  Raises if an image kept more pixels than `capacity`."""
        counts = self.counts.cpu().tolist()
        over = [(b, n) for b, n in enumerate(counts) if n > self.capacity]
        if over:
            raise RuntimeError(f"point_cloud overflow: (image, kept) = {over} exceeds capacity {self.capacity}")
        trim = lambda t, b, n: None if t is None else t[b, :n]
        return [{"points": trim(self.points, b, n), "normals": trim(self.normals, b, n), "index": trim(self.index, b, n),
                 "colors": trim(self.colors, b, n)} for b, n in enumerate(counts)]


def point_cloud(pred: torch.Tensor, intrinsics, size: Optional[Sequence[int]] = None, lo: float = 1e-3, hi: float = 10.0,
                depth_range: Tuple[float, float] = (0.0, float("inf")), unc: Optional[torch.Tensor] = None, unc_plane: int = hip.UNC_STD,
                unc_range: Tuple[float, float] = (float("-inf"), float("inf")), stride: int = 1, normals: bool = True,
                capacity: Optional[int] = None, colors: Optional[torch.Tensor] = None, out: Optional[PointCloud] = None) -> PointCloud:
    """`unproject`, then the pixels worth keeping, in row-major pixel order per image (`cfp_points_compact`): x and y multiples of
    `stride`, near < Z < far for `depth_range` = (near, far) and -- with `unc`, the [B,3,h,w] tensor of
    `model(x, return_uncertainty=True)[3]` -- plane `unc_plane` (hip.UNC_*) inside the closed interval `unc_range`, the plane brought to
    H x W like the prediction when it is smaller.  `capacity` rows per image, ceil(H/stride) * ceil(W/stride) by default, which cannot
    overflow; with a smaller one `counts` still reports the true number and `split()` raises.  `colors` [B,3,H,W] (any dtype, on the
    device) is gathered with `index`.  `out`: the result of an earlier call with the same shapes to write into.  No host synchronisation."""
    pred = _pred3(pred)
    B, h, w = pred.shape
    H, W = _size(size, h, w)
    stride = int(stride)
    if stride < 1:
        raise ValueError(f"stride must be at least 1, got {stride}")
    near, far = (float(v) for v in depth_range)
    if not near < far:
        raise ValueError(f"empty depth_range {(near, far)}")
    u_lo, u_hi = (float(v) for v in unc_range)
    if not u_lo <= u_hi:
        raise ValueError(f"empty unc_range {(u_lo, u_hi)}")
    if unc is not None:
        if not isinstance(unc, torch.Tensor) or unc.dtype != torch.float32 or not unc.is_cuda:
            raise ValueError("unc must be a float32 device tensor")
        if unc.dim() != 4 or unc.shape[0] != B or unc.shape[1] != 3:
            raise ValueError(f"unc must be [B,3,h,w] with B = {B}, got {tuple(unc.shape)}")
        if unc_plane not in (hip.UNC_STD, hip.UNC_ENTROPY, hip.UNC_PMAX):
            raise ValueError(f"unc_plane must be one of hip.UNC_STD / UNC_ENTROPY / UNC_PMAX, got {unc_plane}")
        unc = unc.contiguous()
    full = -(-H // stride) * -(-W // stride)
    cap = full if capacity is None else int(capacity)
    if cap < 1:
        raise ValueError(f"capacity must be at least 1, got {cap}")
    if colors is not None:
        if not isinstance(colors, torch.Tensor) or not colors.is_cuda or tuple(colors.shape) != (B, 3, H, W):
            raise ValueError(f"colors must be a device tensor [B,3,H,W] = {(B, 3, H, W)}")
    dev = pred.device
    if out is not None:
        if not isinstance(out, PointCloud) or out.capacity != cap or out.size != (H, W) or (out.normals is not None) != bool(normals):
            raise ValueError("out must be the PointCloud of a call with the same size, capacity and normals")
        _check_out(out.points, (B, cap, 3), torch.float32, "out.points")
        _check_out(out.index, (B, cap), torch.int32, "out.index")
        _check_out(out.counts, (B,), torch.int32, "out.counts")
        if normals:
            _check_out(out.normals, (B, cap, 3), torch.float32, "out.normals")
        res = out
    else:
        res = PointCloud(torch.empty(B, cap, 3, dtype=torch.float32, device=dev),
                         torch.empty(B, cap, 3, dtype=torch.float32, device=dev) if normals else None,
                         torch.zeros(B, cap, dtype=torch.int32, device=dev),       # untouched rows stay a valid index for the colour gather
                         None, torch.empty(B, dtype=torch.int32, device=dev), cap, (H, W))
    dense = unproject(pred, intrinsics, (H, W), lo, hi, normals=bool(normals))
    pts, nrm = dense if normals else (dense, None)
    nbytes = hip.load().cfp_points_compact_ws_bytes(B, H, W, stride)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=dev)
    plane = None if unc is None else unc[:, unc_plane]
    hip.call("cfp_points_compact", pts.data_ptr(), hip.ptr(nrm), H, W, B, stride, near, far,
             0 if plane is None else plane.data_ptr(), 0 if unc is None else unc.shape[2], 0 if unc is None else unc.shape[3],
             0 if unc is None else unc.stride(0), u_lo, u_hi, cap, res.points.data_ptr(), hip.ptr(res.normals), res.index.data_ptr(),
             res.counts.data_ptr(), ws.data_ptr(), nbytes, hip.current_stream())
    if colors is not None:
        flat = colors.reshape(B, 3, H * W)
        res.colors = torch.gather(flat, 2, res.index.long().clamp_(0, H * W - 1)[:, None, :].expand(B, 3, cap)).transpose(1, 2).contiguous()
    else:
        res.colors = None
    return res


def _host(a, dtype=None) -> Optional[np.ndarray]:
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    return a if dtype is None else a.astype(dtype, copy=False)


def write_ply(path: str, points, normals=None, colors=None) -> int:
    """Binary little-endian PLY: float32 x y z [nx ny nz] [uchar red green blue] per vertex.  points / normals [N,3] float, colors
    [N,3] uint8, or floating point in 0..1 (scaled, rounded and clamped to 0..255); tensors or arrays.  Host side.  Returns N."""
    p = _host(points, np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"points must be [N,3], got {p.shape}")
    n, c = _host(normals, np.float32), _host(colors)
    for name, a in (("normals", n), ("colors", c)):
        if a is not None and a.shape != p.shape:
            raise ValueError(f"{name} must be {p.shape} like points, got {a.shape}")
    if c is not None and c.dtype != np.uint8:
        c = np.clip(np.rint(c.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if n is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if c is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    v = np.empty(p.shape[0], dtype=np.dtype(fields))
    for i, k in enumerate("xyz"):
        v[k] = p[:, i]
        if n is not None:
            v["n" + k] = n[:, i]
    if c is not None:
        for i, k in enumerate(("red", "green", "blue")):
            v[k] = c[:, i]
    names = {"<f4": "float", "u1": "uchar"}
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {p.shape[0]}\n" + \
        "".join(f"property {names[t]} {k}\n" for k, t in fields) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(v.tobytes())
    return int(p.shape[0])
