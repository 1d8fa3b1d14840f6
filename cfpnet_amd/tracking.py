"""Camera tracking on the device: where the pose of `temporal.TemporalFilter` and `tsdf.TsdfVolume` comes from when no odometry delivers it.

`icp` aligns a frame -- the prediction and its std map -- with a model map in another camera by dense point-to-plane ICP: every source
pixel is back-projected like `pointcloud.unproject` does, moved by the current pose estimate, projected into the model camera and
paired with the model point it lands on (projective data association); the pairs' point-to-plane residuals, weighted by the two
predicted variances, give one 6 x 6 Gauss-Newton step per iteration (`cfp_icp_step`: accumulate and finalize, two launches, no atomics).
The model map is a `TsdfVolume.raycast` (frame-to-model tracking, KinectFusion's other half) or the previous frame's
`pointcloud.unproject(..., normals=True)` (frame-to-frame odometry).  `Tracker` is the loop around a volume: raycast -> track ->
integrate, with nothing synchronising with the host, so an `update` can be captured in a graph.  The arithmetic is `csrc/icp.hip`
(definition in include/cfpnet_hip.h); nothing here computes on the CPU.

`icp_rgb` is `icp` with the image: beside the point-to-plane term every pair compares the frame's luminance with the model's picture
(`TsdfVolume.shade` of the raycast) at the pixel it projects to (`cfp_icp_rgb_step`, `csrc/icp_rgb.hip`).  In front of a
wall, on a floor, along a corridor geometry observes three of the six degrees of freedom and `icp` refuses every step; the texture
observes the other three.  `Tracker(..., photo_std=...)` turns it on for `update_rgb`.  There is ONE image level: the photometric term
pulls over about half the finest texture period -- a pixel or two on natural images --, while geometry keeps its wide basin for the
degrees of freedom it sees.  An image pyramid is a later step.

This is frame-to-model dense ICP and nothing more: no relocalisation, no loop closure, no image pyramid.  It follows a camera that moves
a few degrees and centimetres per frame; a visual-inertial front end remains the answer for fast motion.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import hip, render
from .pointcloud import _check_out, _intrinsics, _pred3, _size
from .temporal import _pose, _std_plane, _ws
from .tsdf import TsdfVolume

STAT_NAMES = ("pairs", "weight", "rms", "rotation", "translation", "accepted")     # columns of `stats`
STAT_NAMES_RGB = STAT_NAMES + ("photo_pairs", "photo_rms")                         # columns of `stats` of `icp_rgb`


class IcpResult(NamedTuple):
    """What `icp` returns, all on the device.  `pose` [B,3,4] f32: [R|t] that takes a point of the current camera into the model camera.
    `world` [B,3,4] f32: the camera-from-world pose of the current frame (None without `ref_pose`).  `stats` [iters,B,6] f32 in
    `STAT_NAMES` order, one row per iteration: the number of pairs, sum w, the weighted rms of the point-to-plane residual BEFORE the
    step (NaN without pairs), |omega| and |v| of the step (0 when refused), and whether the step was accepted (1 / 0).  `sums` [B,32] f64
    of the last iteration: the 21 entries of the upper triangle of A = sum w J J^T by rows, the 6 of g = sum w J r, sum w r r, sum w,
    the pair count, two zeros -- A is the information matrix of the pose at the solution (for a LEFT increment (omega, v) of `pose`), its
    inverse the covariance a pose graph or a filter wants.  `index` [B,H,W] i32 (None unless asked for): the model pixel ym * Wm + xm
    each source pixel was paired with in the last iteration, -1 where none.  `ws`: the workspace, reused when the tuple comes back as
    `out`.

    From `icp_rgb` with an image: `stats` [iters,B,8] in `STAT_NAMES_RGB` order -- the six above (pairs, weight and rms are the
    geometric ones), the number of photometric pairs and their rms intensity residual (NaN without any); `sums` [B,64]: the 30 above,
    the same 30 over the photometric pairs (A and g of the step are the sums of the two halves), four zeros; `residual` [B,H,W] f32 (None
    unless asked for): the intensity residual model - frame of the last iteration where a photometric pair was formed, NaN elsewhere;
    `src_luma` [B,H,W], `mdl_luma` [B,Hm,Wm]: the luminance planes the call computed (None where the caller passed a plane)."""
    pose: torch.Tensor
    world: Optional[torch.Tensor]
    stats: torch.Tensor
    sums: torch.Tensor
    index: Optional[torch.Tensor]
    ws: torch.Tensor
    residual: Optional[torch.Tensor] = None
    src_luma: Optional[torch.Tensor] = None
    mdl_luma: Optional[torch.Tensor] = None


def _map(t, shape, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda:
        raise ValueError(f"{what} must be a float32 device tensor")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must be {tuple(shape)}, got {tuple(t.shape)}")
    return t.contiguous()


def _icp_numbers(cos_min, iters, stride, dist_max, z_near, lo, hi, std_floor, min_pairs, min_pivot):
    if not float(lo) < float(hi):
        raise ValueError(f"empty depth range [{lo}, {hi}]")
    for name, v in (("dist_max", dist_max), ("z_near", z_near), ("std_floor", std_floor)):
        if not (float(v) > 0.0 and math.isfinite(float(v))):
            raise ValueError(f"{name} must be positive and finite, got {v}")
    if not -1.0 <= float(cos_min) <= 1.0:
        raise ValueError(f"cos_min must lie in [-1, 1], got {cos_min}")
    if int(iters) != iters or iters < 1:
        raise ValueError(f"iters must be a positive integer, got {iters!r}")
    if int(stride) != stride or stride < 1:
        raise ValueError(f"stride must be a positive integer, got {stride!r}")
    if int(min_pairs) != min_pairs or min_pairs < 6:
        raise ValueError(f"min_pairs must be an integer of at least 6, got {min_pairs!r}")
    if not 0.0 <= float(min_pivot) < 1.0:
        raise ValueError(f"min_pivot must lie in [0, 1), got {min_pivot}")


def icp(pred: torch.Tensor, intrinsics, model_depth: torch.Tensor, model_normals: torch.Tensor, pose0=None,
        unc: Optional[torch.Tensor] = None, model_std: Optional[torch.Tensor] = None, model_intrinsics=None,
        size: Optional[Sequence[int]] = None, src_normals: Optional[torch.Tensor] = None, cos_min: float = 0.5, iters: int = 10,
        stride: int = 1, dist_max: float = 0.25, z_near: float = 1e-3, lo: float = 1e-3, hi: float = 10.0, std_floor: float = 1e-3,
        min_pairs: int = 100, min_pivot: float = 1e-6, ref_pose=None, index: bool = False, out: Optional[IcpResult] = None) -> IcpResult:
    """pred [B,h,w] / [B,1,h,w] f32 on the device, seen on the H x W grid of `size` like `pointcloud.unproject` sees it (twice the
    prediction by default), aligned with the model map `model_depth` [B,Hm,Wm], `model_normals` [B,Hm,Wm,3] (`model_std` [B,Hm,Wm]
    optional) of the camera `model_intrinsics` (= `intrinsics` by default) -> `IcpResult`.  `iters` Gauss-Newton iterations of
    `cfp_icp_step` on one pose buffer, started from `pose0` ([R|t] current-to-model in every form `TemporalFilter.update` takes; None:
    the identity, "the camera did not move"); the count is fixed, so the call can be captured in a graph.  `unc`: the model's [B,3,h,w]
    uncertainty tensor or a [B,hu,wu] std map; with it or `model_std` a pair weighs 1 / (std^2 + model_std^2), else 1.  Only every
    `stride`-th pixel in x and y is used.  A pair is dropped when its points lie more than `dist_max` apart or -- with `src_normals`
    [B,H,W,3], `unproject`'s -- when the normals' cosine is below `cos_min`.  A step is refused (the pose stays as it is) with fewer than
    `min_pairs` pairs or a pivot of the 6 x 6 system not above `min_pivot` times its largest diagonal entry: a scene that does not
    constrain all six degrees of freedom.  `ref_pose`: camera-from-world of the model camera; given, `world` is the frame's own
    camera-from-world pose.  `index=True` adds the association map.  `out`: the result of an earlier call to write into -- then nothing
    is allocated here.  Bitwise reproducible; no host synchronisation."""
    return _icp(pred, intrinsics, model_depth, model_normals, pose0, unc, model_std, model_intrinsics, size, src_normals, cos_min, iters,
                stride, dist_max, z_near, lo, hi, std_floor, min_pairs, min_pivot, ref_pose, index, out, None)


def _luma(img, shape, mean, std, buf, what: str):
    """A luminance plane [B,H,W] of `shape` out of `img`: a ready plane is used as it is (-> (plane, None)); a planar normalised image
    [B,3,H,W] or an interleaved one [B,H,W,3] in 0..1 goes through `cfp_luma` into `buf` (allocated when None) -> (buf, buf)."""
    B, H, W = shape
    if not isinstance(img, torch.Tensor) or img.dtype != torch.float32 or not img.is_cuda:
        raise ValueError(f"{what} must be a float32 device tensor")
    if tuple(img.shape) == (B, H, W):
        if buf is not None:
            raise ValueError(f"out holds a luminance buffer for {what}, but {what} is a ready plane")
        return img.contiguous(), None
    planar = what == "rgb"
    want = (B, 3, H, W) if planar else (B, H, W, 3)
    if tuple(img.shape) != want:
        raise ValueError(f"{what} must be {want} or a luminance plane {(B, H, W)}, got {tuple(img.shape)}")
    img = img.contiguous()
    if buf is None:
        buf = torch.empty(B, H, W, dtype=torch.float32, device=img.device)
    else:
        _check_out(buf, (B, H, W), torch.float32, f"out luminance of {what}")
    hip.call("cfp_luma", img.data_ptr(), 0 if planar else 1, render._three(mean, "mean") if planar else None,
             render._three(std, "std") if planar else None, H, W, B, buf.data_ptr(), hip.current_stream())
    return buf, buf


def icp_rgb(pred: torch.Tensor, intrinsics, model_depth: torch.Tensor, model_normals: torch.Tensor, pose0=None,
            unc: Optional[torch.Tensor] = None, model_std: Optional[torch.Tensor] = None, model_intrinsics=None,
            size: Optional[Sequence[int]] = None, src_normals: Optional[torch.Tensor] = None, cos_min: float = 0.5, iters: int = 10,
            stride: int = 1, dist_max: float = 0.25, z_near: float = 1e-3, lo: float = 1e-3, hi: float = 10.0, std_floor: float = 1e-3,
            min_pairs: int = 100, min_pivot: float = 1e-6, ref_pose=None, index: bool = False, out: Optional[IcpResult] = None,
            rgb: Optional[torch.Tensor] = None, model_rgb: Optional[torch.Tensor] = None, photo_std: float = 0.04,
            photo_max: float = 0.25, mean=render.IMAGENET_MEAN, std=render.IMAGENET_STD, residual: bool = False) -> IcpResult:
    """`icp` with every argument of `icp`, and the image: `rgb` is the frame's, [B,3,H,W] f32 normalised like the model's input
    (c = rgb * std + mean, as `TsdfVolume.integrate_rgb` reads it) or a ready luminance plane [B,H,W]; `model_rgb` the model's picture on
    the model grid, [B,Hm,Wm,3] in 0..1 -- `TsdfVolume.shade` of the raycast -- or a luminance plane [B,Hm,Wm].  Giving only one of the
    two is an error; giving neither is `icp` itself, with its result shapes.  With both, every pair of `icp` that lands inside the model
    picture also compares luminances (bilinear in the model's, NaN taps and residuals above `photo_max` dropped) and the step solves the
    sum of the two systems (`cfp_icp_rgb_step`); `min_pairs` counts the geometric pairs.

    `photo_std`: the intensity noise in 0..1 units; a photometric pair weighs 1 / photo_std^2, on the maximum-likelihood footing of
    1 / (std^2 + model_std^2) of the depth.  The default 0.04 -- roughly 10 / 255 -- is a stated prior and is NOT measured on any sensor;
    with unit geometric weights (no `unc`, no `model_std`) it has to be chosen against 1 / metre^2 instead.  `residual=True` adds the
    residual map.  `stats` is [iters,B,8] (`STAT_NAMES_RGB`), `sums` [B,64].  The luminance planes are computed once per call (`cfp_luma`)
    into buffers that `out` reuses: with `out` nothing is allocated.  One image level: see the module's docstring.  Bitwise reproducible;
    no host synchronisation."""
    if (rgb is None) != (model_rgb is None):
        raise ValueError("rgb and model_rgb are given together or not at all")
    photo = None
    if rgb is not None:
        for name, v, top in (("photo_std", photo_std, False), ("photo_max", photo_max, True)):
            if not (float(v) > 0.0 and (top or math.isfinite(float(v)))):
                raise ValueError(f"{name} must be positive{'' if top else ' and finite'}, got {v}")
        weight = 1.0 / (float(photo_std) * float(photo_std))
        if not 1e-38 < weight < 3e38:                                     # as a float32: positive and finite
            raise ValueError(f"photo_std gives no finite float32 weight: {photo_std}")
        photo = (rgb, model_rgb, weight, float(photo_max), mean, std, bool(residual))
    elif residual:
        raise ValueError("residual needs rgb and model_rgb")
    return _icp(pred, intrinsics, model_depth, model_normals, pose0, unc, model_std, model_intrinsics, size, src_normals, cos_min, iters,
                stride, dist_max, z_near, lo, hi, std_floor, min_pairs, min_pivot, ref_pose, index, out, photo)


def _icp(pred, intrinsics, model_depth, model_normals, pose0, unc, model_std, model_intrinsics, size, src_normals, cos_min, iters, stride,
         dist_max, z_near, lo, hi, std_floor, min_pairs, min_pivot, ref_pose, index, out, photo) -> IcpResult:
    """`icp` (photo None) and `icp_rgb` (photo = (rgb, model_rgb, weight, photo_max, mean, std, residual))."""
    pred = _pred3(pred)
    B, h, w = pred.shape
    H, W = _size(size, h, w)
    _icp_numbers(cos_min, iters, stride, dist_max, z_near, lo, hi, std_floor, min_pairs, min_pivot)
    dev = pred.device
    if not isinstance(model_depth, torch.Tensor) or model_depth.dim() != 3:
        raise ValueError("model_depth must be a float32 device tensor [B,Hm,Wm]")
    Hm, Wm = model_depth.shape[1:]
    model_depth = _map(model_depth, (B, Hm, Wm), "model_depth")
    model_normals = _map(model_normals, (B, Hm, Wm, 3), "model_normals")
    if model_std is not None:
        model_std = _map(model_std, (B, Hm, Wm), "model_std")
    if src_normals is not None:
        src_normals = _map(src_normals, (B, H, W, 3), "src_normals")
    std = None if unc is None else _std_plane(unc, B)
    K = _intrinsics(intrinsics, B, dev)
    Km = K if model_intrinsics is None else _intrinsics(model_intrinsics, B, dev)
    T0 = None if pose0 is None else _pose(pose0, B, dev)
    Tr = None if ref_pose is None else _pose(ref_pose, B, dev)
    iters, stride = int(iters), int(stride)
    nbytes = (hip.load().cfp_icp_ws_bytes if photo is None else hip.load().cfp_icp_rgb_ws_bytes)(B, H, W, stride)
    ncol, nsum = (6, 32) if photo is None else (8, 64)
    want_res = photo is not None and photo[6]
    if out is not None:
        if not isinstance(out, IcpResult):
            raise ValueError("out must be the IcpResult of an earlier call")
        _check_out(out.pose, (B, 3, 4), torch.float32, "out pose")
        if (out.world is None) != (Tr is None):
            raise ValueError("out world must be given exactly when ref_pose is")
        if Tr is not None:
            _check_out(out.world, (B, 3, 4), torch.float32, "out world")
        _check_out(out.stats, (iters, B, ncol), torch.float32, "out stats")
        _check_out(out.sums, (B, nsum), torch.float64, "out sums")
        if (out.index is None) == bool(index):
            raise ValueError("out index must be given exactly when index is asked for")
        if index:
            _check_out(out.index, (B, H, W), torch.int32, "out index")
        if (out.residual is None) == want_res:
            raise ValueError("out residual must be given exactly when residual is asked for")
        if want_res:
            _check_out(out.residual, (B, H, W), torch.float32, "out residual")
        if photo is None and (out.src_luma is not None or out.mdl_luma is not None):
            raise ValueError("out holds luminance buffers, but no image is given")
        _ws(nbytes, out.ws, dev)
    else:
        out = IcpResult(torch.empty(B, 3, 4, dtype=torch.float32, device=dev),
                        None if Tr is None else torch.empty(B, 3, 4, dtype=torch.float32, device=dev),
                        torch.empty(iters, B, ncol, dtype=torch.float32, device=dev), torch.empty(B, nsum, dtype=torch.float64, device=dev),
                        torch.empty(B, H, W, dtype=torch.int32, device=dev) if index else None, _ws(nbytes, None, dev),
                        torch.empty(B, H, W, dtype=torch.float32, device=dev) if want_res else None)
    if photo is not None:
        sl, sbuf = _luma(photo[0], (B, H, W), photo[4], photo[5], out.src_luma, "rgb")
        ml, mbuf = _luma(photo[1], (B, Hm, Wm), photo[4], photo[5], out.mdl_luma, "model_rgb")
        if sbuf is not out.src_luma or mbuf is not out.mdl_luma:
            out = out._replace(src_luma=sbuf, mdl_luma=mbuf)
    T = out.pose.view(B, 12)
    if T0 is None:
        T.zero_()
        T[:, ::5] = 1.0                                                   # entries 0, 5, 10: the identity, written on the device
    elif T0.data_ptr() != T.data_ptr():
        T.copy_(T0)
    interp = int((h, w) != (H, W))                    # the rule of pointcloud.unproject
    stream = hip.current_stream()
    for it in range(iters):
        last = it == iters - 1
        if photo is not None:
            hip.call("cfp_icp_rgb_step", pred.data_ptr(), h, w, H, W, B, interp, float(lo), float(hi), hip.ptr(std),
                     0 if std is None else std.shape[1], 0 if std is None else std.shape[2], 0 if std is None else std.stride(0),
                     float(std_floor), hip.ptr(src_normals), float(cos_min), K.data_ptr(), model_depth.data_ptr(),
                     model_normals.data_ptr(), hip.ptr(model_std), Hm, Wm, Km.data_ptr(), stride, float(z_near), float(dist_max),
                     int(min_pairs), float(min_pivot), T.data_ptr(), hip.ptr(Tr) if last else 0, hip.ptr(out.world) if last else 0,
                     hip.ptr(out.index) if last else 0, out.sums.data_ptr(), out.stats[it].data_ptr(), out.ws.data_ptr(), nbytes,
                     sl.data_ptr(), ml.data_ptr(), photo[2], photo[3], hip.ptr(out.residual) if last else 0, stream)
            continue
        hip.call("cfp_icp_step", pred.data_ptr(), h, w, H, W, B, interp, float(lo), float(hi), hip.ptr(std),
                 0 if std is None else std.shape[1], 0 if std is None else std.shape[2], 0 if std is None else std.stride(0),
                 float(std_floor), hip.ptr(src_normals), float(cos_min), K.data_ptr(), model_depth.data_ptr(), model_normals.data_ptr(),
                 hip.ptr(model_std), Hm, Wm, Km.data_ptr(), stride, float(z_near), float(dist_max), int(min_pairs), float(min_pivot),
                 T.data_ptr(), hip.ptr(Tr) if last else 0, hip.ptr(out.world) if last else 0, hip.ptr(out.index) if last else 0,
                 out.sums.data_ptr(), out.stats[it].data_ptr(), out.ws.data_ptr(), nbytes, stream)
    return out


_TRACKER_OPTIONS = ("cos_min", "iters", "stride", "dist_max", "min_pairs", "min_pivot")
_TRACKER_PHOTO_OPTIONS = ("photo_std", "photo_max")


class Tracker:
    """Frame-to-model tracking around a `TsdfVolume`: every `update` ray-casts the volume at the last pose, aligns the new frame with that
    raycast (`icp`, started from "the camera did not move") and integrates the frame at the pose it found.  `pose0`: camera-from-world
    of the first frame (None: the identity: the world frame is the first camera's).  `icp_options`: `cos_min`, `iters`, `stride`,
    `dist_max`, `min_pairs`, `min_pivot` of `icp`; the depth range, the std floor, z_near, the camera and the grid are the volume's.
    `.pose` [B,3,4] f32 is the last pose, on the device.  Nothing synchronises with the host: once the first frame is in, an `update`
    can be captured in a graph and replayed on new inputs.

    `photo_std` (None: off) and `photo_max` (0.25) of `icp_rgb`, given among the options, make `update_rgb` track with the image as
    well: raycast -> `shade` -> `icp_rgb` against the shaded picture -> `integrate_rgb`.  `update` has no image and tracks by geometry;
    so does a frame that comes before the map has any colour.

    A lost frame is still integrated: `update` does not look at the result on the host.  `stats[-1, :, 5]` says whether the last step
    was accepted; a caller who wants to keep a doubtful frame out of the map calls `update(..., integrate=False)` (or `track`), reads
    the stats and integrates the frame afterwards."""

    def __init__(self, volume: TsdfVolume, pose0=None, **icp_options):
        if not isinstance(volume, TsdfVolume):
            raise ValueError("volume must be a TsdfVolume")
        unknown = sorted(set(icp_options) - set(_TRACKER_OPTIONS) - set(_TRACKER_PHOTO_OPTIONS))
        if unknown:
            raise ValueError(f"unknown icp option(s) {unknown}: one of {_TRACKER_OPTIONS + _TRACKER_PHOTO_OPTIONS}")
        self.photo_std, self.photo_max = icp_options.pop("photo_std", None), icp_options.pop("photo_max", 0.25)
        if self.photo_std is not None and not (float(self.photo_std) > 0.0 and math.isfinite(float(self.photo_std))):
            raise ValueError(f"photo_std must be positive and finite (or None: off), got {self.photo_std}")
        if not float(self.photo_max) > 0.0:
            raise ValueError(f"photo_max must be positive, got {self.photo_max}")
        defaults = dict(cos_min=0.5, iters=10, stride=1, dist_max=0.25, min_pairs=100, min_pivot=1e-6)
        defaults.update(icp_options)
        _icp_numbers(lo=volume.lo, hi=volume.hi, std_floor=volume.std_floor, z_near=volume.z_near, **defaults)
        if pose0 is not None and not (isinstance(pose0, torch.Tensor) and pose0.is_cuda):
            n = np.ndim(pose0.numpy() if isinstance(pose0, torch.Tensor) else pose0)
            _pose(pose0, len(pose0) if n == 3 else 1, "cpu")              # refuse bad numbers now, not at the first frame
        self.volume, self.pose0, self.options = volume, pose0, defaults
        self.pose = self.stats = None
        self._out = None
        self._primed = False

    def reset(self):
        """Forget the trajectory: the next `update` integrates at `pose0` without tracking.  The volume is not touched."""
        self._primed = False

    def _track(self, pred, unc, image=None) -> IcpResult:
        """`image`: (rgb, mean, std) of the frame when the image takes part in the tracking."""
        if not self._primed:
            raise ValueError("nothing to track against yet: the first update integrates the first frame")
        pred = _pred3(pred)
        vol = self.volume
        depth, std, normals = vol.raycast(self.pose, normals=True)
        photo = image is not None and vol.color is not None
        if self._out is not None and (self._out.pose.shape[0] != pred.shape[0] or self._out.index is not None or
                                      (self._out.mdl_luma is not None) != photo):
            self._out = None
        if photo:
            self._out = icp_rgb(pred, vol.camera, depth, normals, None, unc, std, None, vol.grid_size, None, lo=vol.lo, hi=vol.hi,
                                std_floor=vol.std_floor, z_near=vol.z_near, ref_pose=self.pose, out=self._out, rgb=image[0],
                                model_rgb=vol.shade(depth, self.pose), photo_std=self.photo_std, photo_max=self.photo_max,
                                mean=image[1], std=image[2], **self.options)
        else:
            self._out = icp(pred, vol.camera, depth, normals, None, unc, std, None, vol.grid_size, None, lo=vol.lo, hi=vol.hi,
                            std_floor=vol.std_floor, z_near=vol.z_near, ref_pose=self.pose, out=self._out, **self.options)
        self.stats = self._out.stats
        return self._out

    def track(self, pred: torch.Tensor, unc: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The camera-from-world pose [B,3,4] f32 (device; the tracker's own buffer, overwritten by the next call) of the frame `pred`,
        `unc` against the volume as it is; `.stats` [iters,B,6] is `icp`'s.  Stores nothing: `.pose` and the volume stay."""
        return self._track(pred, unc).world

    def _update(self, pred, unc, integrate, fuse, image=None):
        """`update` and `update_rgb`: `fuse(pose)` integrates the frame."""
        if not self._primed:
            pred = _pred3(pred)
            B = pred.shape[0]
            T0 = _pose(self.pose0, B, pred.device).view(B, 3, 4)
            if self.pose is None or self.pose.shape[0] != B:
                self.pose = torch.empty(B, 3, 4, dtype=torch.float32, device=pred.device)
            self.pose.copy_(T0)
            fuse(self.pose)
            self._primed = True
            self.stats = None
            return self.pose, None
        res = self._track(pred, unc, image)
        self.pose.copy_(res.world)
        if integrate:
            fuse(self.pose)
        return self.pose, res.stats

    def update(self, pred: torch.Tensor, unc: Optional[torch.Tensor] = None, integrate: bool = True):
        """`track`, the pose stored in `.pose` (a device copy), the frame integrated at it -> (pose [B,3,4], stats [iters,B,6]).  The
        first call (and the first after `reset`) integrates at `pose0` without tracking and returns stats None."""
        return self._update(pred, unc, integrate, lambda pose: self.volume.integrate(pred, unc, pose))

    def update_rgb(self, pred: torch.Tensor, rgb: torch.Tensor, unc: Optional[torch.Tensor] = None, integrate: bool = True,
                   mean=render.IMAGENET_MEAN, std=render.IMAGENET_STD):
        """`update` with the frame's image: the frame is integrated by `TsdfVolume.integrate_rgb(pred, rgb, unc, pose, mean, std)`, so the
        map takes the colour along -- `volume.write_ply(pattern, colors=True)` afterwards is the coloured room.  Without the option
        `photo_std` tracking itself does not look at the image: the poses are those of `update`.  With it the frame is tracked by
        `icp_rgb` against the shaded raycast (stats [iters,B,8]), once the map has colour: the first frame is integrated as ever."""
        rgb = render._rgb4(rgb)                                           # refuse a bad image before the frame is tracked
        image = None if self.photo_std is None else (rgb, mean, std)
        return self._update(pred, unc, integrate, lambda pose: self.volume.integrate_rgb(pred, rgb, unc, pose, mean, std), image)
