"""Depth across views and across time on the device: what a consumer of streaming ToF depth completion does with the previous frame.

`reproject` carries a prediction into another camera -- the same camera one pose later, the ToF sensor, a second colour camera -- as a
forward warp with a z-buffer (`cfp_depth_reproject`): the depth at a source pixel is the value `pointcloud.unproject` back-projects, the
point is moved by the pose, projected with the target intrinsics and the nearest surface wins every target pixel; a map that travels with
the depth (a variance or std plane) is read at the winning source pixel.  `fuse` combines the current prediction with such a warped prior
by their variances, per pixel, behind a gate that keeps a changed scene from being averaged away (`cfp_depth_fuse`).  `TemporalFilter`
is the loop around the two: state, workspaces and outputs allocated once, no host synchronisation, so an `update` can be captured in a
graph.  The arithmetic is `csrc/reproject.hip` (definition in include/cfpnet_hip.h); nothing here computes on the CPU.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import hip
from .pointcloud import _check_out, _intrinsics, _pred3, _size

COUNT_NAMES = ("prior", "fused", "rejected", "filled")     # columns of `counts` (CFP_FUSE_*)


def _pose(pose, B: int, device) -> torch.Tensor:
    """-> [B,12] float32 on the device: the rows of [R|t].  `pose`: None (identity), [3,4], [4,4], [B,3,4] or [B,4,4].  Host numbers
    are validated (finite; a 4 x 4's last row is 0 0 0 1); a float32 device tensor cannot be without a synchronisation."""
    if pose is None:
        pose = np.eye(4)[:3]
    if isinstance(pose, torch.Tensor) and pose.is_cuda:
        if pose.dtype != torch.float32:
            raise ValueError(f"a device pose must be float32, got {pose.dtype}")
        t = pose
    else:
        try:
            a = np.asarray(pose.numpy() if isinstance(pose, torch.Tensor) else pose, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("pose must be [3,4], [4,4], [B,3,4] or [B,4,4]") from None
        if not np.isfinite(a).all():
            raise ValueError("pose must be finite")
        if a.ndim >= 2 and a.shape[-2:] == (4, 4) and not (a[..., 3, :] == np.array([0.0, 0.0, 0.0, 1.0])).all():
            raise ValueError("the last row of a 4 x 4 pose must be 0 0 0 1")
        t = torch.from_numpy(a.astype(np.float32))
    if t.dim() not in (2, 3) or tuple(t.shape[-2:]) not in ((3, 4), (4, 4)) or (t.dim() == 3 and t.shape[0] != B):
        raise ValueError(f"pose must be [3,4], [4,4], [B,3,4] or [B,4,4] with B = {B}, got {tuple(t.shape)}")
    if t.dim() == 2:
        t = t[None].expand(B, -1, -1)
    return t[:, :3, :].reshape(B, 12).contiguous().to(device)


def _plane3(plane, B: int, what: str) -> torch.Tensor:
    """A [B,hu,wu] float32 device map whose images are contiguous (a plane of the model's [B,3,h,w] uncertainty tensor is: no copy)."""
    if not isinstance(plane, torch.Tensor) or plane.dtype != torch.float32 or not plane.is_cuda:
        raise ValueError(f"{what} must be a float32 device tensor")
    if plane.dim() == 4 and plane.shape[1] == 1:
        plane = plane[:, 0]
    if plane.dim() != 3 or plane.shape[0] != B or min(plane.shape) < 1:
        raise ValueError(f"{what} must be [B,hu,wu] or [B,1,hu,wu] with B = {B}, got {tuple(plane.shape)}")
    if plane.stride(2) != 1 or plane.stride(1) != plane.shape[2] or plane.stride(0) < 0:
        plane = plane.contiguous()
    return plane


def _std_plane(unc, B: int) -> torch.Tensor:
    """The std plane of `model(x, return_uncertainty=True)[3]` ([B,3,h,w], plane hip.UNC_STD) or a [B,hu,wu] std map itself."""
    if isinstance(unc, torch.Tensor) and unc.dim() == 4 and unc.shape[1] == 3:
        if unc.dtype != torch.float32 or not unc.is_cuda:
            raise ValueError("unc must be a float32 device tensor")
        unc = unc.contiguous()[:, hip.UNC_STD]
    return _plane3(unc, B, "unc")


def _ws(nbytes: int, ws, device) -> torch.Tensor:
    if ws is None:
        return torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=device)
    if ws.dtype != torch.int64 or ws.numel() * 8 < nbytes or not ws.is_cuda:
        raise ValueError(f"workspace must be an int64 device tensor of at least {nbytes} bytes")
    return ws


def _reproject(pred, K, T, Kd, H, W, Hd, Wd, lo, hi, splat, z_near, plane, out, ws=None):
    """`reproject` after the argument checks, on device tensors K, T, Kd; `ws` is reused when given."""
    B, h, w = pred.shape
    dev = pred.device
    want = 3 if plane is not None else 2
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != want:
            raise ValueError("out must be (depth, index) or, with a plane, (depth, index, plane)")
        _check_out(out[0], (B, Hd, Wd), torch.float32, "out depth")
        _check_out(out[1], (B, Hd, Wd), torch.int32, "out index")
        if plane is not None:
            _check_out(out[2], (B, Hd, Wd), torch.float32, "out plane")
        out = tuple(out)
    else:
        out = (torch.empty(B, Hd, Wd, dtype=torch.float32, device=dev), torch.empty(B, Hd, Wd, dtype=torch.int32, device=dev))
        if plane is not None:
            out += (torch.empty(B, Hd, Wd, dtype=torch.float32, device=dev),)
    nbytes = hip.load().cfp_depth_reproject_ws_bytes(B, Hd, Wd)
    ws = _ws(nbytes, ws, dev)
    interp = int((h, w) != (H, W))                    # the rule of pointcloud.unproject
    hip.call("cfp_depth_reproject", pred.data_ptr(), h, w, H, W, B, interp, float(lo), float(hi), K.data_ptr(), T.data_ptr(),
             Kd.data_ptr(), Hd, Wd, splat, float(z_near), hip.ptr(plane), 0 if plane is None else plane.shape[1],
             0 if plane is None else plane.shape[2], 0 if plane is None else plane.stride(0), out[0].data_ptr(), out[1].data_ptr(),
             0 if plane is None else out[2].data_ptr(), ws.data_ptr(), nbytes, hip.current_stream())
    return out


def reproject(pred: torch.Tensor, intrinsics, pose, dst_intrinsics=None, size: Optional[Sequence[int]] = None,
              dst_size: Optional[Sequence[int]] = None, lo: float = 1e-3, hi: float = 10.0, splat: int = 1, z_near: float = 1e-3,
              plane: Optional[torch.Tensor] = None, out=None):
    """pred [B,h,w] / [B,1,h,w] f32 on the device, seen on the H x W grid of `size` like `pointcloud.unproject` sees it (twice the
    prediction by default; a full-resolution map goes in with size = its own and lo, hi = -inf, inf) -> (depth [B,Hd,Wd] f32, index
    [B,Hd,Wd] i32) in the view `pose` away (`cfp_depth_reproject`): P' = R P + t for pose = [R|t], camera frame x right, y down, z
    forward; [3,4], [4,4], [B,3,4] or [B,4,4], host numbers (validated as finite) or a float32 device tensor (the caller's contract).
    `intrinsics` as in `unproject`; `dst_intrinsics` (the same by default) and `dst_size` (= `size` by default) describe the target
    camera -- given, this is RGB-D registration.  depth is Z' of the nearest source that lands on the pixel, index its y * W + x; NaN
    and -1 where nothing lands.  `splat` 1: nearest target pixel; 2: the four around the projection, which closes the cracks of a mild
    magnification.  Points with Z' < `z_near` are dropped.  `plane` [B,hu,wu] f32 (a variance or std map of the source, brought to H x W
    like the prediction) adds a third result: the plane at the winning source pixel.  `out`: the tuple of an earlier call to write
    into.  Bitwise reproducible; no host synchronisation."""
    pred = _pred3(pred)
    B, h, w = pred.shape
    H, W = _size(size, h, w)
    Hd, Wd = (H, W) if dst_size is None else _size(dst_size, h, w)
    if not float(lo) < float(hi):
        raise ValueError(f"empty depth range [{lo}, {hi}]")
    if splat not in (1, 2):
        raise ValueError(f"splat must be 1 or 2, got {splat!r}")
    if not (float(z_near) > 0.0 and math.isfinite(float(z_near))):
        raise ValueError(f"z_near must be positive and finite, got {z_near}")
    K = _intrinsics(intrinsics, B, pred.device)
    Kd = K if dst_intrinsics is None else _intrinsics(dst_intrinsics, B, pred.device)
    T = _pose(pose, B, pred.device)
    if plane is not None:
        plane = _plane3(plane, B, "plane")
    return _reproject(pred, K, T, Kd, H, W, Hd, Wd, lo, hi, int(splat), z_near, plane, out)


def _fuse_numbers(process_sigma, gate_k, gate_abs, std_floor):
    ps, gk, ga, sf = float(process_sigma), float(gate_k), float(gate_abs), float(std_floor)
    if not (ps >= 0.0 and math.isfinite(ps)):
        raise ValueError(f"process_sigma must be non-negative and finite, got {process_sigma}")
    if not (gk >= 0.0 and ga >= 0.0):
        raise ValueError(f"gate_k and gate_abs must be non-negative, got {(gate_k, gate_abs)}")
    if not (sf > 0.0 and math.isfinite(sf)):
        raise ValueError(f"std_floor must be positive and finite, got {std_floor}")
    return ps * ps, gk, ga, sf


def fuse(cur: torch.Tensor, cur_std: torch.Tensor, prior_depth: torch.Tensor, prior_var: torch.Tensor, process_sigma: float = 0.02,
         gate_k: float = 3.0, gate_abs: float = 0.05, std_floor: float = 1e-3, lo: float = 1e-3, hi: float = 10.0, out=None, ws=None):
    """The current prediction `cur` [B,h,w] / [B,1,h,w] f32 with its std map `cur_std` ([B,hu,wu], or the model's [B,3,h,w] uncertainty
    tensor: plane hip.UNC_STD), both brought to the H x W grid of the prior, fused with `prior_depth`, `prior_var` [B,H,W] f32 -- the
    previous state as `reproject` delivers it, NaN where nothing is known -- per pixel by their variances (`cfp_depth_fuse`): the
    prior's variance grows by `process_sigma`^2 first; where |prior - current| exceeds `gate_k` * sqrt(var_c + var_p) + `gate_abs`
    the current value stands alone (the scene changed or a surface was uncovered); where only one of the two is known it is taken.
    -> (depth [B,H,W] f32, var [B,H,W] f32, counts [B,4] i32 in `COUNT_NAMES` order, stats [B,2] f64 = sum |p - c| and sum (p - c)^2
    over the pixels where both are known).  `out`: the four tensors of an earlier call.  Bitwise reproducible; no host synchronisation."""
    cur = _pred3(cur)
    B, h, w = cur.shape
    std = _std_plane(cur_std, B)
    for name, t in (("prior_depth", prior_depth), ("prior_var", prior_var)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.dim() != 3 or t.shape[0] != B:
            raise ValueError(f"{name} must be a float32 device tensor [B,H,W] with B = {B}")
    if prior_depth.shape != prior_var.shape:
        raise ValueError(f"prior_depth and prior_var differ in shape: {tuple(prior_depth.shape)} and {tuple(prior_var.shape)}")
    prior_depth, prior_var = prior_depth.contiguous(), prior_var.contiguous()
    H, W = prior_depth.shape[1:]
    if not float(lo) < float(hi):
        raise ValueError(f"empty depth range [{lo}, {hi}]")
    pv, gk, ga, sf = _fuse_numbers(process_sigma, gate_k, gate_abs, std_floor)
    dev = cur.device
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 4:
            raise ValueError("out must be (depth, var, counts, stats)")
        _check_out(out[0], (B, H, W), torch.float32, "out depth")
        _check_out(out[1], (B, H, W), torch.float32, "out var")
        _check_out(out[2], (B, 4), torch.int32, "out counts")
        _check_out(out[3], (B, 2), torch.float64, "out stats")
        out = tuple(out)
    else:
        out = (torch.empty(B, H, W, dtype=torch.float32, device=dev), torch.empty(B, H, W, dtype=torch.float32, device=dev),
               torch.empty(B, 4, dtype=torch.int32, device=dev), torch.empty(B, 2, dtype=torch.float64, device=dev))
    nbytes = hip.load().cfp_depth_fuse_ws_bytes(B, H, W)
    ws = _ws(nbytes, ws, dev)
    hip.call("cfp_depth_fuse", cur.data_ptr(), h, w, H, W, B, int((h, w) != (H, W)), float(lo), float(hi), std.data_ptr(), std.shape[1],
             std.shape[2], std.stride(0), sf, prior_depth.data_ptr(), prior_var.data_ptr(), pv, gk, ga, out[0].data_ptr(),
             out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), ws.data_ptr(), nbytes, hip.current_stream())
    return out


class TemporalFilter:
    """A per-pixel depth state (depth, variance) on the H x W grid that follows the camera: every `update` warps the state into the new
    view (`reproject` with the state's variance as the plane, `splat` = 2 by default so that a small motion leaves no cracks) and fuses
    the new prediction into it (`fuse`); without a pose the camera did not move and the state itself is the prior.  `intrinsics`: (fx, fy, cx, cy) of the H x W grid or a float32 [B,4] tensor; `size` = (H, W),
    twice the prediction by default.  State, workspaces and outputs are allocated by the first `update` and reused; `counts` [B,4] i32
    and `stats` [B,2] f64 of the last fusion stay on the device."""

    def __init__(self, intrinsics, size: Optional[Sequence[int]] = None, process_sigma: float = 0.02, gate_k: float = 3.0,
                 gate_abs: float = 0.05, splat: int = 2, lo: float = 1e-3, hi: float = 10.0, std_floor: float = 1e-3,
                 z_near: float = 1e-3):
        if splat not in (1, 2):
            raise ValueError(f"splat must be 1 or 2, got {splat!r}")
        if not float(lo) < float(hi):
            raise ValueError(f"empty depth range [{lo}, {hi}]")
        if not (float(z_near) > 0.0 and math.isfinite(float(z_near))):
            raise ValueError(f"z_near must be positive and finite, got {z_near}")
        _fuse_numbers(process_sigma, gate_k, gate_abs, std_floor)
        if not isinstance(intrinsics, torch.Tensor):
            _intrinsics(intrinsics, 1, "cpu")                             # refuse bad numbers now, not at the first frame
        self.intrinsics, self.size = intrinsics, size
        self.process_sigma, self.gate_k, self.gate_abs, self.std_floor = process_sigma, gate_k, gate_abs, std_floor
        self.splat, self.lo, self.hi, self.z_near = int(splat), float(lo), float(hi), float(z_near)
        self.depth = self.var = self.std = self.counts = self.stats = None
        self._shape = None
        self._primed = False

    def reset(self):
        """Forget the state: the next `update` adopts its frame.  The buffers stay."""
        self._primed = False

    def _allocate(self, B, h, w, dev):
        H, W = _size(self.size, h, w)
        self._shape = (B, h, w)
        self._K = _intrinsics(self.intrinsics, B, dev)
        f = lambda: torch.empty(B, H, W, dtype=torch.float32, device=dev)
        self.depth, self.var, self.std, self._prior_depth, self._prior_var = f(), f(), f(), f(), f()
        self._index = torch.empty(B, H, W, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(B, 4, dtype=torch.int32, device=dev)
        self.stats = torch.zeros(B, 2, dtype=torch.float64, device=dev)
        lib = hip.load()
        self._ws_warp = _ws(lib.cfp_depth_reproject_ws_bytes(B, H, W), None, dev)
        self._ws_fuse = _ws(lib.cfp_depth_fuse_ws_bytes(B, H, W), None, dev)
        self._primed = False

    def update(self, pred: torch.Tensor, unc: torch.Tensor, pose=None):
        """pred [B,h,w] / [B,1,h,w] f32 and its uncertainty (the model's [B,3,h,w] tensor or a [B,hu,wu] std map), `pose` = [R|t] from
        the previous camera frame to this one (None: the camera did not move) -> (depth, std) [B,H,W] f32: the filter's own buffers,
        overwritten by the next call.  The first call (and the first after `reset`) adopts the frame.  No host synchronisation once
        the buffers exist: with `pose` None or a float32 device tensor the call can be captured in a graph."""
        pred = _pred3(pred)
        B, h, w = pred.shape
        if self._shape != (B, h, w):
            self._allocate(B, h, w, pred.device)
        H, W = self.depth.shape[1:]
        out = (self.depth, self.var, self.counts, self.stats)
        if not self._primed:
            self._prior_depth.fill_(float("nan"))                         # no prior: fuse takes the frame as it is
            self._prior_var.fill_(float("nan"))
            prior = (self._prior_depth, self._prior_var)
        elif pose is None:
            prior = (self.depth, self.var)                                # the camera did not move: the state is the prior, fused in place
        else:
            inf = float("inf")
            prior = (self._prior_depth, self._prior_var)
            _reproject(self.depth, self._K, _pose(pose, B, pred.device), self._K, H, W, H, W, -inf, inf, self.splat, self.z_near, self.var,
                       (self._prior_depth, self._index, self._prior_var), self._ws_warp)
        fuse(pred, unc, prior[0], prior[1], self.process_sigma, self.gate_k, self.gate_abs, self.std_floor, self.lo, self.hi, out=out,
             ws=self._ws_fuse)
        self._primed = True
        torch.sqrt(self.var, out=self.std)
        return self.depth, self.std
