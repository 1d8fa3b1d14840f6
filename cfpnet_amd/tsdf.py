"""A world-anchored map on the device: what room-scale reconstruction does with streaming ToF depth completion.

`temporal.TemporalFilter` keeps a per-pixel state that follows the camera; whatever leaves the image is forgotten and every warp
re-samples it.  `TsdfVolume` keeps a truncated signed distance field in a fixed world frame instead: `integrate` fuses a prediction and
its std map into the voxels the camera sees (`cfp_tsdf_integrate`: the per-voxel weight is the inverse-variance sum `fuse` keeps per
pixel), `raycast` turns the volume back into depth, std and normals in any view (`cfp_tsdf_raycast`), so two views combine into
something a third can look at, and `surface_points` takes the map out: the zero crossings of F along the voxel lattice's edges as oriented
points in the world frame (`cfp_tsdf_surface`, `csrc/tsdf_surface.hip`), which `write_ply` stores.  The arithmetic is
`csrc/tsdf.hip` (definition in include/cfpnet_hip.h); nothing here computes on the CPU except the PLY writer.

Colour: `integrate_rgb` fuses the frame's RGB image -- the model's own input, already on the device at the grid's size --
into a second volume `.color` of (R, G, B, Wc) per voxel by the same inverse-variance weights (`cfp_tsdf_integrate_rgb`, the same kernel
as `integrate`), `shade` gives the colour image that belongs to a raycast (`cfp_tsdf_shade`), `surface_colors` the colours of the
extracted points (`cfp_tsdf_surface_rgb`, both `csrc/tsdf_color.hip`), and `write_ply(..., colors=True)` stores them.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch

from . import hip, render
from .pointcloud import _check_out, _intrinsics, _pred3, _size, write_ply
from .temporal import _pose, _std_plane

COUNT_NAMES = ("seen", "updated", "behind")           # columns of `counts` (CFP_TSDF_*)
COLOR_COUNT_NAMES = COUNT_NAMES + ("coloured",)       # columns of `color_counts`
_F32_MAX = 3.4028234663852886e38                      # the library wants a finite cap: "no cap" is the largest float32


def _positive(v, what: str) -> float:
    v = float(v)
    if not (v > 0.0 and math.isfinite(v)):
        raise ValueError(f"{what} must be positive and finite, got {v}")
    return v


class SurfacePoints:
    """Result of `TsdfVolume.surface_points`, everything on the device: `points` [B,cap,3] f32 in the world frame, `normals` [B,cap,3]
    f32 or None (towards the free space the observing camera was in; NaN where the volume does not know), `std` [B,cap] f32, `index`
    [B,cap] i32 (the lattice edge 3 * voxel + axis a row came from), `counts` [B] i32 -- the number of crossings per image, also when it
    exceeds `capacity`.  Rows at or beyond min(count, capacity) hold nothing of meaning.  `colors` [B,cap,3] f32 or None: what
    `TsdfVolume.surface_colors` wrote (NaN where the map has no colour)."""

    def __init__(self, points, normals, std, index, counts, capacity: int, colors=None):
        self.points, self.normals, self.std, self.index, self.counts = points, normals, std, index, counts
        self.capacity = capacity
        self.colors = colors

    def split(self) -> List[dict]:
        """The one host synchronisation: per image {"points": [n,3], "normals", "std", "index", "colors"} trimmed to its count (None
        where absent).  Raises if an image has more crossings than `capacity`."""
        counts = self.counts.cpu().tolist()
        over = [(b, n) for b, n in enumerate(counts) if n > self.capacity]
        if over:
            raise RuntimeError(f"surface_points overflow: (image, kept) = {over} exceeds capacity {self.capacity}")
        trim = lambda t, b, n: None if t is None else t[b, :n]
        return [{"points": trim(self.points, b, n), "normals": trim(self.normals, b, n), "std": trim(self.std, b, n),
                 "index": trim(self.index, b, n), "colors": trim(self.colors, b, n)} for b, n in enumerate(counts)]


class TsdfVolume:
    """A TSDF of `dims` = (Dx, Dy, Dz) voxels of edge `voxel` metres per image; voxel (i, j, k) has its centre at `origin` + voxel *
    (i, j, k) in the world frame.  `.volume` [B,Dz,Dy,Dx,2] f32 holds (F, Wt) per voxel: F the signed distance to the surface over
    `trunc` (3 * voxel by default), clipped at 1 in front, and Wt the sum of 1 / std^2 of what was fused, capped at `w_max` (None: no
    cap); empty is (1, 0).  `intrinsics`: (fx, fy, cx, cy) of the H x W grid the predictions are seen on, or a float32 [B,4] tensor;
    `size` = (H, W), twice the prediction by default.  A pose is [R|t], camera-from-world (Pc = R Pw + t), in every form
    `TemporalFilter.update` takes; None is the identity.  The volume, the counts and the raycast's outputs are allocated once and
    reused; nothing synchronises with the host: with a float32 device pose, `integrate` followed by `raycast` can be captured in a
    graph."""

    def __init__(self, dims: Sequence[int], voxel: float, origin: Sequence[float], intrinsics, size: Optional[Sequence[int]] = None,
                 trunc: Optional[float] = None, w_max: Optional[float] = None, lo: float = 1e-3, hi: float = 10.0,
                 std_floor: float = 1e-3, z_near: float = 1e-3):
        try:
            Dx, Dy, Dz = (int(v) for v in dims)
        except (TypeError, ValueError):
            raise ValueError(f"dims must be (Dx, Dy, Dz), got {dims!r}") from None
        if min(Dx, Dy, Dz) < 1 or Dx * Dy * Dz >= 2 ** 31 - 256:
            raise ValueError(f"dims must be positive with fewer than 2^31 voxels, got {(Dx, Dy, Dz)}")
        try:
            ox, oy, oz = (float(v) for v in origin)
        except (TypeError, ValueError):
            raise ValueError(f"origin must be (ox, oy, oz), got {origin!r}") from None
        if not all(math.isfinite(v) for v in (ox, oy, oz)):
            raise ValueError(f"origin must be finite, got {(ox, oy, oz)}")
        self.dims, self.origin = (Dx, Dy, Dz), (ox, oy, oz)
        self.voxel = _positive(voxel, "voxel")
        self.trunc = 3.0 * self.voxel if trunc is None else _positive(trunc, "trunc")
        if w_max is None or float(w_max) == math.inf:
            self.w_max = _F32_MAX
        else:
            self.w_max = _positive(w_max, "w_max")
        if not float(lo) < float(hi):
            raise ValueError(f"empty depth range [{lo}, {hi}]")
        self.lo, self.hi = float(lo), float(hi)
        self.std_floor, self.z_near = _positive(std_floor, "std_floor"), _positive(z_near, "z_near")
        if not isinstance(intrinsics, torch.Tensor):
            _intrinsics(intrinsics, 1, "cpu")                             # refuse bad numbers now, not at the first frame
        self.intrinsics, self.size = intrinsics, size
        self.volume = self.counts = None
        self.color_counts = None
        self._color = None
        self._shape = None
        self._rays = {}
        self._shades = {}
        self._surface_ws = None

    @property
    def camera(self) -> Optional[torch.Tensor]:
        """The intrinsics [B,4] f32 on the device the volume integrates with; None before the first integrate.  Read-only."""
        return None if self._shape is None else self._K

    @property
    def grid_size(self) -> Optional[tuple]:
        """(H, W) of the grid the predictions are seen on; None before the first integrate.  Read-only."""
        return None if self._shape is None else self._hw

    @property
    def color(self) -> Optional[torch.Tensor]:
        """The colour volume [B,Dz,Dy,Dx,4] f32, (R, G, B, Wc) per voxel, on the device; None before the first `integrate_rgb`.
        Read-only."""
        return self._color

    def reset(self):
        """Empty the volume: F = 1, Wt = 0, and the colour volume, if there is one: (0, 0, 0, 0).  The buffers stay."""
        if self.volume is not None:
            self.volume[..., 0] = 1.0
            self.volume[..., 1] = 0.0
        if self._color is not None:
            self._color.zero_()

    def _allocate(self, B, h, w, dev):
        Dx, Dy, Dz = self.dims
        self._shape = (B, h, w)
        self._hw = _size(self.size, h, w)
        self._K = _intrinsics(self.intrinsics, B, dev)
        self.volume = torch.empty(B, Dz, Dy, Dx, 2, dtype=torch.float32, device=dev)
        self.counts = torch.zeros(B, 3, dtype=torch.int32, device=dev)
        self.color_counts = None
        self._color = None
        self._rays = {}
        self._shades = {}
        self._surface_ws = None
        self.reset()

    def integrate(self, pred: torch.Tensor, unc: Optional[torch.Tensor] = None, pose=None) -> torch.Tensor:
        """pred [B,h,w] / [B,1,h,w] f32 on the device and its uncertainty (the model's [B,3,h,w] tensor or a [B,hu,wu] std map; None:
        every observation weighs 1), seen from `pose` -> counts [B,3] i32 in `COUNT_NAMES` order, on the device: the voxels that saw a
        valid depth, that were updated, that lie more than `trunc` behind the surface.  The first call allocates the volume (empty);
        a call with another batch or prediction size starts a new one."""
        pred = _pred3(pred)
        B, h, w = pred.shape
        std = None if unc is None else _std_plane(unc, B)
        if self._shape != (B, h, w):
            self._allocate(B, h, w, pred.device)
        H, W = self._hw
        Dx, Dy, Dz = self.dims
        T = _pose(pose, B, pred.device)
        hip.call("cfp_tsdf_integrate", pred.data_ptr(), h, w, H, W, B, int((h, w) != (H, W)), self.lo, self.hi, hip.ptr(std),
                 0 if std is None else std.shape[1], 0 if std is None else std.shape[2], 0 if std is None else std.stride(0),
                 self.std_floor, self._K.data_ptr(), T.data_ptr(), self.volume.data_ptr(), Dx, Dy, Dz, *self.origin, self.voxel,
                 self.trunc, self.z_near, self.w_max, self.counts.data_ptr(), hip.current_stream())
        return self.counts

    def integrate_rgb(self, pred: torch.Tensor, rgb: torch.Tensor, unc: Optional[torch.Tensor] = None, pose=None,
                      mean=render.IMAGENET_MEAN, std=render.IMAGENET_STD) -> torch.Tensor:
        """`integrate`, and the frame's colour with it in the same pass (`cfp_tsdf_integrate_rgb`): `rgb` [B,3,H,W] f32 on the device is
        the normalised image on the volume's (H, W) grid -- the model's input -- and c = rgb * std + mean is fused into `.color` by the
        weights of the geometry, at the voxels within `trunc` of the surface -> counts [B,4] i32 in `COLOR_COUNT_NAMES` order, on the
        device: `.color_counts`, a buffer of its own (`.counts` is not written).  (F, Wt) and the first three counts are bit for bit
        what `integrate` gives.  The first call allocates the colour volume (zeros); frames with and without an image mix freely, the
        colour keeps its own weight Wc.  No host synchronisation; capturable like `integrate`."""
        rgb = render._rgb4(rgb)
        pred = _pred3(pred)
        B, h, w = pred.shape
        H, W = _size(self.size, h, w)
        if tuple(rgb.shape) != (B, 3, H, W):
            raise ValueError(f"rgb must be [B,3,H,W] = {(B, 3, H, W)}, the volume's grid, got {tuple(rgb.shape)}")
        if rgb.device != pred.device:
            raise ValueError("rgb and pred must be on the same device")
        m, s = render._three(mean, "mean"), render._three(std, "std")
        sd = None if unc is None else _std_plane(unc, B)
        if self._shape != (B, h, w):
            self._allocate(B, h, w, pred.device)
        Dx, Dy, Dz = self.dims
        if self._color is None:
            self._color = torch.zeros(B, Dz, Dy, Dx, 4, dtype=torch.float32, device=pred.device)
            self.color_counts = torch.zeros(B, 4, dtype=torch.int32, device=pred.device)
        T = _pose(pose, B, pred.device)
        hip.call("cfp_tsdf_integrate_rgb", pred.data_ptr(), h, w, H, W, B, int((h, w) != (H, W)), self.lo, self.hi, hip.ptr(sd),
                 0 if sd is None else sd.shape[1], 0 if sd is None else sd.shape[2], 0 if sd is None else sd.stride(0),
                 self.std_floor, self._K.data_ptr(), T.data_ptr(), self.volume.data_ptr(), Dx, Dy, Dz, *self.origin, self.voxel,
                 self.trunc, self.z_near, self.w_max, rgb.data_ptr(), m, s, self._color.data_ptr(), self.color_counts.data_ptr(),
                 hip.current_stream())
        return self.color_counts

    def raycast(self, pose=None, intrinsics=None, size: Optional[Sequence[int]] = None, t_range: Optional[Sequence[float]] = None,
                step: Optional[float] = None, normals: bool = True, out=None):
        """The volume seen from `pose` by the camera `intrinsics` / `size` = (Hd, Wd) (the integrating camera's by default) -> (depth
        [B,Hd,Wd] f32, std [B,Hd,Wd] f32) or, with `normals`, (depth, std, normals [B,Hd,Wd,3] f32 in the camera frame, facing the
        camera like `unproject`'s).  Rays are marched from t_range[0] to t_range[1] ((z_near, hi) by default) in camera depth, every
        `step` (trunc / 2 by default); NaN where a ray meets no surface or leaves what was observed.  The depth is metric depth on the
        (Hd, Wd) grid: it goes straight into `pointcloud.point_cloud(depth, K, size=(Hd, Wd), lo=-inf, hi=inf)`.  The results of a
        view of one size are the volume's own buffers, overwritten by the next raycast of that size; `out`: the tuple of an earlier
        call to write into.  Bitwise reproducible; no host synchronisation."""
        if self.volume is None:
            raise ValueError("nothing was integrated yet: the volume is allocated by the first integrate")
        B = self.volume.shape[0]
        dev = self.volume.device
        Hd, Wd = self._hw if size is None else _size(size, 1, 1)
        K = self._K if intrinsics is None else _intrinsics(intrinsics, B, dev)
        t0, t1 = (self.z_near, self.hi) if t_range is None else (float(v) for v in t_range)
        if not (t0 < t1 and math.isfinite(t0) and math.isfinite(t1)):
            raise ValueError(f"t_range must be finite with t_min < t_max, got {(t0, t1)}")
        step = 0.5 * self.trunc if step is None else _positive(step, "step")
        want = 3 if normals else 2
        if out is not None:
            if not isinstance(out, (tuple, list)) or len(out) != want:
                raise ValueError("out must be (depth, std) or, with normals, (depth, std, normals)")
            out = tuple(out)
        else:
            out = self._rays.get((Hd, Wd, bool(normals)))
            if out is None:
                out = (torch.empty(B, Hd, Wd, dtype=torch.float32, device=dev), torch.empty(B, Hd, Wd, dtype=torch.float32, device=dev))
                if normals:
                    out += (torch.empty(B, Hd, Wd, 3, dtype=torch.float32, device=dev),)
                self._rays[(Hd, Wd, bool(normals))] = out
        _check_out(out[0], (B, Hd, Wd), torch.float32, "out depth")
        _check_out(out[1], (B, Hd, Wd), torch.float32, "out std")
        if normals:
            _check_out(out[2], (B, Hd, Wd, 3), torch.float32, "out normals")
        T = _pose(pose, B, dev)
        Dx, Dy, Dz = self.dims
        hip.call("cfp_tsdf_raycast", self.volume.data_ptr(), Dx, Dy, Dz, B, *self.origin, self.voxel, K.data_ptr(), T.data_ptr(), Hd, Wd,
                 t0, t1, step, out[0].data_ptr(), out[2].data_ptr() if normals else 0, out[1].data_ptr(), hip.current_stream())
        return out

    def shade(self, depth: torch.Tensor, pose=None, intrinsics=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The colour of the map at the points the depth map names (`cfp_tsdf_shade`): `depth` [B,Hd,Wd] f32 on the device is a
        `raycast` result seen from `pose` by `intrinsics` (the integrating camera's by default), or any metric depth on that grid ->
        [B,Hd,Wd,3] f32, c in 0..1 as it was integrated; NaN where the depth is NaN or the map has no colour.  The grid is the depth's.
        The result of one size is the volume's own buffer, overwritten by the next shade of that size; `out`: a tensor to write into.
        Bitwise reproducible; no host synchronisation."""
        if self._color is None:
            raise ValueError("nothing was coloured yet: the colour volume is allocated by the first integrate_rgb")
        B = self._color.shape[0]
        dev = self._color.device
        if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32 or not depth.is_cuda:
            raise ValueError("depth must be a float32 device tensor")
        if depth.dim() != 3 or depth.shape[0] != B or min(depth.shape) < 1:
            raise ValueError(f"depth must be [B,Hd,Wd] with B = {B}, got {tuple(depth.shape)}")
        depth = depth.contiguous()
        Hd, Wd = depth.shape[1:]
        K = self._K if intrinsics is None else _intrinsics(intrinsics, B, dev)
        if out is None:
            out = self._shades.get((Hd, Wd))
            if out is None:
                out = self._shades[(Hd, Wd)] = torch.empty(B, Hd, Wd, 3, dtype=torch.float32, device=dev)
        _check_out(out, (B, Hd, Wd, 3), torch.float32, "out")
        T = _pose(pose, B, dev)
        Dx, Dy, Dz = self.dims
        hip.call("cfp_tsdf_shade", self._color.data_ptr(), Dx, Dy, Dz, B, *self.origin, self.voxel, K.data_ptr(), T.data_ptr(), Hd, Wd,
                 depth.data_ptr(), out.data_ptr(), hip.current_stream())
        return out

    def surface_colors(self, sp: SurfacePoints, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The colours of the points `surface_points` extracted (`cfp_tsdf_surface_rgb`) -> [B,cap,3] f32 on the device, also stored
        as `sp.colors`: the colours of the edge's two voxels blended like the point itself, the colour of the one end that has one, or
        NaN where neither has.  Rows at or beyond min(count, capacity) are not written.  `out`: a tensor to write into (`sp.colors`,
        if there is one, by default).  No host synchronisation; capturable after `surface_points(capacity, out=...)`."""
        if self._color is None:
            raise ValueError("nothing was coloured yet: the colour volume is allocated by the first integrate_rgb")
        if not isinstance(sp, SurfacePoints):
            raise ValueError("sp must be the SurfacePoints of surface_points")
        B, cap = self._color.shape[0], sp.capacity
        _check_out(sp.index, (B, cap), torch.int32, "sp.index")
        _check_out(sp.counts, (B,), torch.int32, "sp.counts")
        if out is None:
            out = sp.colors if sp.colors is not None else torch.empty(B, cap, 3, dtype=torch.float32, device=self._color.device)
        _check_out(out, (B, cap, 3), torch.float32, "out")
        Dx, Dy, Dz = self.dims
        hip.call("cfp_tsdf_surface_rgb", self.volume.data_ptr(), self._color.data_ptr(), Dx, Dy, Dz, B, sp.index.data_ptr(),
                 sp.counts.data_ptr(), cap, out.data_ptr(), hip.current_stream())
        sp.colors = out
        return out

    def _surface_args(self, w_min, max_jump):
        if self.volume is None:
            raise ValueError("nothing was integrated yet: the volume is allocated by the first integrate")
        w_min = float(w_min)
        max_jump = math.inf if max_jump is None else float(max_jump)
        if not w_min >= 0.0:
            raise ValueError(f"w_min must not be negative, got {w_min}")
        if not max_jump >= 0.0:
            raise ValueError(f"max_jump must not be negative, got {max_jump}")
        B = self.volume.shape[0]
        nbytes = hip.load().cfp_tsdf_surface_ws_bytes(B, *self.dims)
        if nbytes == 0:
            raise ValueError(f"dims {self.dims} have too many lattice edges for an int32 index (3 * Dx * Dy * Dz < 2^31)")
        if self._surface_ws is None:
            self._surface_ws = torch.empty(nbytes // 8, dtype=torch.int64, device=self.volume.device)
        return B, w_min, max_jump, nbytes

    def _surface(self, w_min, max_jump, nbytes, res, counts):
        Dx, Dy, Dz = self.dims
        hip.call("cfp_tsdf_surface", self.volume.data_ptr(), Dx, Dy, Dz, self.volume.shape[0], *self.origin, self.voxel, w_min, max_jump,
                 0 if res is None else res.capacity, *((0, 0, 0, 0) if res is None else
                                                       (res.points.data_ptr(), hip.ptr(res.normals), res.std.data_ptr(), res.index.data_ptr())),
                 counts.data_ptr(), self._surface_ws.data_ptr(), nbytes, hip.current_stream())

    def surface_count(self, w_min: float = 0.0, max_jump: Optional[float] = None) -> torch.Tensor:
        """The number of crossings `surface_points` with the same options would keep -> counts [B] i32 on the device.  It only counts
        (the volume is read once); no host synchronisation."""
        B, w_min, max_jump, nbytes = self._surface_args(w_min, max_jump)
        counts = torch.empty(B, dtype=torch.int32, device=self.volume.device)
        self._surface(w_min, max_jump, nbytes, None, counts)
        return counts

    def surface_points(self, capacity: Optional[int] = None, w_min: float = 0.0, max_jump: Optional[float] = None, normals: bool = True,
                       out: Optional[SurfacePoints] = None) -> SurfacePoints:
        """The map as oriented points in the WORLD frame (`cfp_tsdf_surface`): one point per edge of the voxel lattice along which F
        changes sign between two observed voxels, in the order of the edge index 3 * voxel + axis, with the normal (the gradient of F,
        towards the free space the camera saw the surface from: R times it is the raycast's normal) and the std 1 / sqrt(Wt) blended
        along the edge.  `w_min`: both voxels have at least this weight; `max_jump` (None: no filter): |F(p) - F(q)| is at most this --
        2 * voxel / trunc is what a clean surface gives, more is an edge between a surface and something fused behind it.  With an
        explicit `capacity` (rows per image) nothing synchronises with the host -- `counts` still reports the true numbers and `split()`
        raises on overflow -- and `out`, the result of an earlier call with the same capacity and normals, reuses every buffer, so the
        call can be captured in a graph after `integrate`.  `capacity=None` counts first, reads the largest count in one host
        synchronisation and allocates exactly that (at least 1).  After `Tracker.update` has run over a sequence the map is
        `tracker.volume.surface_points()`.  Bitwise reproducible."""
        B, w_min, max_jump, nbytes = self._surface_args(w_min, max_jump)
        dev = self.volume.device
        if out is not None:
            if not isinstance(out, SurfacePoints) or (capacity is not None and out.capacity != int(capacity)) or \
                    (out.normals is not None) != bool(normals):
                raise ValueError("out must be the SurfacePoints of a call with the same capacity and normals")
            cap = out.capacity
            _check_out(out.points, (B, cap, 3), torch.float32, "out.points")
            _check_out(out.std, (B, cap), torch.float32, "out.std")
            _check_out(out.index, (B, cap), torch.int32, "out.index")
            _check_out(out.counts, (B,), torch.int32, "out.counts")
            if normals:
                _check_out(out.normals, (B, cap, 3), torch.float32, "out.normals")
            res = out
        else:
            if capacity is None:
                cap = max(int(self.surface_count(w_min, max_jump).max()), 1)              # the one host synchronisation
            else:
                cap = int(capacity)
                if cap < 1:
                    raise ValueError(f"capacity must be at least 1, got {cap}")
            res = SurfacePoints(torch.empty(B, cap, 3, dtype=torch.float32, device=dev),
                                torch.empty(B, cap, 3, dtype=torch.float32, device=dev) if normals else None,
                                torch.empty(B, cap, dtype=torch.float32, device=dev), torch.empty(B, cap, dtype=torch.int32, device=dev),
                                torch.empty(B, dtype=torch.int32, device=dev), cap)
        self._surface(w_min, max_jump, nbytes, res, res.counts)
        return res

    def write_ply(self, path_pattern: str, **options) -> List[int]:
        """One binary PLY per image (xyz and, unless `normals=False`, the normals) through `pointcloud.write_ply`: image b goes to
        `path_pattern.format(b)` -- a pattern without a field is used as it is for a single image.  `options` are those of
        `surface_points`, and `colors=True`: the points' `surface_colors` as `uchar red green blue` (a point the map has no colour
        for is black); it raises without a colour volume.  Host side after one synchronisation.  Returns the vertex counts."""
        colors = bool(options.pop("colors", False))
        if colors and self._color is None:
            raise ValueError("colors=True, but nothing was coloured yet: the colour volume is allocated by the first integrate_rgb")
        sp = self.surface_points(**options)
        if colors:
            self.surface_colors(sp)
        parts = sp.split()
        paths = [path_pattern.format(b) for b in range(len(parts))]
        if len(set(paths)) != len(paths):
            raise ValueError(f"path_pattern {path_pattern!r} names the same file for several images: put a {{}} field into it")
        if colors:
            return [write_ply(path, part["points"], part["normals"], torch.nan_to_num(part["colors"], nan=0.0))
                    for path, part in zip(paths, parts)]
        return [write_ply(path, part["points"], part["normals"]) for path, part in zip(paths, parts)]
