"""Pictures of the pipeline's inputs and outputs, painted on the device: what the reference's `--save_pred`, `--save_gt`,
`--save_rgb`, `--save_error_map` and `--save_for_demo` switches are for (`colorize`, src/utils/utils.py:44-64).

The depth a picture shows is the value `metrics.eval_metrics` evaluates at that pixel -- the `np.clip` -> bilinear protocol of
`evaluate_all.py:40-41`, one implementation in `csrc/metrics_pred.h` -- so the float32 prediction never crosses to the host: what leaves
the device is uint8 RGB (or uint16 millimetres).  The arithmetic is `cfp_render_depth` / `cfp_render_zones` / `cfp_render_rgb`
(`csrc/render.hip`, definitions in include/cfpnet_hip.h); every function below is one launch without a host synchronisation, and takes
`out=` -- a uint8 [B,H,W,3] tensor or a view of a larger canvas (`demo_panel` renders five pieces into one).  Value ranges are given, never
derived from the data.  The colour tables come from `colormaps.py` (text, written once by tools/gen_colormaps.py); nothing here imports
matplotlib.  `write_png` is the only host-side code.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import colormaps, hip

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
COLORMAPS = ("magma_r", "magma", "viridis", "turbo", "jet")

_tables: Optional[Dict[str, np.ndarray]] = None
_device_tables: Dict[Tuple[str, str], torch.Tensor] = {}


def colormap_table(name: str) -> np.ndarray:
    """The uint8 [256,3] table `name` on the host (read-only)."""
    global _tables
    if _tables is None:
        _tables = {k: colormaps.table(k) for k in colormaps.NAMES}
        for t in _tables.values():
            t.setflags(write=False)
    if name not in _tables:
        raise ValueError(f"cmap must be one of {', '.join(sorted(_tables))}, got {name!r}")
    return _tables[name]


def colormap(name: str, device) -> torch.Tensor:
    """The table `name` as a uint8 [256,3] tensor on `device`, uploaded once per device."""
    key = (name, str(torch.device(device)))
    if key not in _device_tables:
        _device_tables[key] = torch.from_numpy(colormap_table(name).copy()).to(device)
    return _device_tables[key]


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------

def _map3(t, name: str) -> torch.Tensor:
    """A float32 device tensor [B,H,W] / [B,1,H,W] -> contiguous [B,H,W]."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda:
        raise ValueError(f"{name} must be a float32 device tensor")
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3 or min(t.shape) < 1:
        raise ValueError(f"{name} must be [B,H,W] or [B,1,H,W], got {tuple(t.shape)}")
    return t.contiguous()


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


def _range(lo, hi, vmin, vmax) -> Tuple[float, float, float, float]:
    lo, hi = float(lo), float(hi)
    if not lo < hi:
        raise ValueError(f"empty depth range: lo = {lo}, hi = {hi}")
    vmin, vmax = lo if vmin is None else float(vmin), hi if vmax is None else float(vmax)
    if not (np.isfinite(vmin) and np.isfinite(vmax) and vmin < vmax):
        raise ValueError(f"vmin < vmax must be finite, got vmin = {vmin}, vmax = {vmax}")
    return lo, hi, vmin, vmax


def _dest(out, B: int, H: int, W: int, device) -> Tuple[torch.Tensor, int, int]:
    """-> (out, image_stride in bytes, pitch in pixels).  `out`: None (a new tensor) or uint8 [B,H,W,3] on the device whose pixels are
    3 adjacent bytes and whose rows are a whole number of pixels apart -- a tensor of its own or a view of a canvas."""
    if out is None:
        return torch.empty(B, H, W, 3, dtype=torch.uint8, device=device), H * W * 3, W
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or not out.is_cuda or tuple(out.shape) != (B, H, W, 3):
        raise ValueError(f"out must be a uint8 device tensor {(B, H, W, 3)}")
    sb, sy, sx, sc = out.stride()
    pitch = sy // 3 if H > 1 else max(W, sy // 3)
    if sc != 1 or (sx != 3 and W > 1) or (H > 1 and (sy % 3 or pitch < W)):
        raise ValueError(f"out must hold pixels as 3 adjacent bytes in rows a whole number of pixels apart, got strides {out.stride()}")
    if B > 1 and sb < H * pitch * 3:
        raise ValueError(f"out: images overlap (strides {out.stride()})")
    return out, max(sb, H * pitch * 3), pitch


def _lut(cmap: str, device) -> torch.Tensor:
    if not isinstance(cmap, str):
        raise ValueError(f"cmap must be a table name, got {cmap!r}")
    return colormap(cmap, device)


def _render(what: int, pred, gt, H: int, W: int, B: int, lo, hi, vmin, vmax, cmap, out, u16=None, scale: float = 0.0):
    interp = 0
    if pred is not None:
        interp = int(tuple(pred.shape[1:]) != (H, W))         # the rule of metrics.eval_metrics in EVALUATE_ALL order
    dev = (pred if pred is not None else gt).device
    lut = stride = pitch = 0
    if u16 is None:
        lut = _lut(cmap, dev).data_ptr()
        out, stride, pitch = _dest(out, B, H, W, dev)
    hip.call("cfp_render_depth", hip.ptr(pred), 0 if pred is None else pred.shape[1], 0 if pred is None else pred.shape[2], hip.ptr(gt),
             H, W, B, interp, lo, hi, what, vmin, vmax, lut, 0 if u16 is not None else out.data_ptr(), stride, pitch, hip.ptr(u16),
             float(scale), hip.current_stream())
    return u16 if u16 is not None else out


# ---- one launch each ---------------------------------------------------------------------------------------------------------------------

def depth_image(pred: torch.Tensor, size: Optional[Sequence[int]] = None, lo: float = 1e-3, hi: float = 10.0, vmin: Optional[float] = None,
                vmax: Optional[float] = None, cmap: str = "magma_r", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pred [B,h,w] / [B,1,h,w] f32 on the device -> uint8 [B,H,W,3]: the clipped, bilinearly enlarged prediction the metrics evaluate,
    through the table `cmap` over [vmin, vmax] (default [lo, hi]).  `size` = (H, W), twice the prediction by default."""
    pred = _map3(pred, "pred")
    B, h, w = pred.shape
    H, W = _size(size, h, w)
    lo, hi, vmin, vmax = _range(lo, hi, vmin, vmax)
    return _render(hip.RENDER_DEPTH, pred, None, H, W, B, lo, hi, vmin, vmax, cmap, out)


def depth_u16(pred: torch.Tensor, size: Optional[Sequence[int]] = None, lo: float = 1e-3, hi: float = 10.0, scale: float = 1000.0,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The same depth as uint16 [B,H,W]: rint(d * scale), ties to even, saturated to 0 .. 65535 (NaN -> 0); scale = 1000 is the 16-bit
    millimetre convention of the NYU / BTS depth PNGs."""
    pred = _map3(pred, "pred")
    B, h, w = pred.shape
    H, W = _size(size, h, w)
    lo, hi, _, _ = _range(lo, hi, None, None)
    scale = float(scale)
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"scale must be finite and positive, got {scale}")
    if out is None:
        out = torch.empty(B, H, W, dtype=torch.uint16, device=pred.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint16 or not out.is_cuda or tuple(out.shape) != (B, H, W) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint16 device tensor {(B, H, W)}")
    return _render(hip.RENDER_DEPTH, pred, None, H, W, B, lo, hi, 0.0, 1.0, None, None, u16=out, scale=scale)


def gt_image(gt: torch.Tensor, lo: float = 1e-3, hi: float = 10.0, vmin: Optional[float] = None, vmax: Optional[float] = None,
             cmap: str = "magma_r", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gt [B,H,W] / [B,1,H,W] f32 on the device -> uint8 [B,H,W,3]; a pixel outside lo < gt < hi is white."""
    gt = _map3(gt, "gt")
    B, H, W = gt.shape
    lo, hi, vmin, vmax = _range(lo, hi, vmin, vmax)
    return _render(hip.RENDER_GT, None, gt, H, W, B, lo, hi, vmin, vmax, cmap, out)


def error_image(pred: torch.Tensor, gt: torch.Tensor, lo: float = 1e-3, hi: float = 10.0, kind: str = "abs", vmax: float = 1.0,
                cmap: str = "jet", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """|d - gt| (`kind="abs"`, metres) or |d - gt| / gt (`"rel"`) over [0, vmax] at the valid pixels lo < gt < hi, white elsewhere;
    d is the prediction as the metrics evaluate it at the ground truth's size."""
    if kind not in ("abs", "rel"):
        raise ValueError(f"kind must be 'abs' or 'rel', got {kind!r}")
    pred, gt = _map3(pred, "pred"), _map3(gt, "gt")
    B, H, W = gt.shape
    if pred.shape[0] != B:
        raise ValueError(f"pred and gt: batch sizes differ ({pred.shape[0]} and {B})")
    lo, hi, vmin, vmax = _range(lo, hi, 0.0, vmax)
    return _render(hip.RENDER_ABS_ERR if kind == "abs" else hip.RENDER_REL_ERR, pred, gt, H, W, B, lo, hi, vmin, vmax, cmap, out)


def _rgb4(rgb) -> torch.Tensor:
    if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.float32 or not rgb.is_cuda:
        raise ValueError("rgb must be a float32 device tensor")
    if rgb.dim() != 4 or rgb.shape[1] != 3 or min(rgb.shape) < 1:
        raise ValueError(f"rgb must be [B,3,H,W], got {tuple(rgb.shape)}")
    return rgb.contiguous()


def _three(v, name: str):
    try:
        v = [float(x) for x in v]
    except TypeError:
        raise ValueError(f"{name} must be 3 numbers") from None
    if len(v) != 3 or not all(np.isfinite(x) for x in v):
        raise ValueError(f"{name} must be 3 finite numbers, got {v}")
    return (ctypes.c_float * 3)(*v)


def rgb_image(rgb: torch.Tensor, mean=IMAGENET_MEAN, std=IMAGENET_STD, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The normalised image [B,3,H,W] f32 on the device -> uint8 [B,H,W,3]: rint(clip(x * std + mean, 0, 1) * 255)."""
    rgb = _rgb4(rgb)
    B, _, H, W = rgb.shape
    m, s = _three(mean, "mean"), _three(std, "std")
    out, stride, pitch = _dest(out, B, H, W, rgb.device)
    hip.call("cfp_render_rgb", rgb.data_ptr(), m, s, H, W, B, out.data_ptr(), stride, pitch, hip.current_stream())
    return out


def zones_overlay(out: torch.Tensor, hist_data: torch.Tensor, rect_data: torch.Tensor, mask: torch.Tensor, vmin: float, vmax: float,
                  cmap: str = "magma_r", alpha: int = 160) -> torch.Tensor:
    """Draws the ToF input over the picture `out` (uint8 [B,H,W,3], in place): every zone of rect_data [B,Z,4] (sy, sx, ey, ex) gets a
    black one-pixel border and, blended with weight alpha / 256, the colour of the mean of its depth samples hist_data [B,Z,S] -- grey
    where mask [B,Z] is not set.  A pixel belongs to the first zone that contains it (the rule of `metrics.region_metrics`)."""
    if not isinstance(out, torch.Tensor) or out.dim() != 4:
        raise ValueError("out must be a uint8 device tensor [B,H,W,3]")
    B, H, W, _ = out.shape
    out, stride, pitch = _dest(out, B, H, W, out.device)
    for t, name in ((hist_data, "hist_data"), (rect_data, "rect_data")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.dim() != 3 or t.shape[0] != B:
            raise ValueError(f"{name} must be a float32 device tensor [B,Z,*] with B = {B}")
    Z, S = hist_data.shape[1:]
    if not 1 <= Z <= 256 or S < 1:
        raise ValueError(f"hist_data must be [B,Z,S] with 1 <= Z <= 256 and S >= 1, got {tuple(hist_data.shape)}")
    if tuple(rect_data.shape) != (B, Z, 4):
        raise ValueError(f"rect_data must be [B,Z,4] = {(B, Z, 4)}, got {tuple(rect_data.shape)}")
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or not mask.is_cuda or tuple(mask.shape) != (B, Z):
        raise ValueError(f"mask must be a bool / uint8 device tensor [B,Z] = {(B, Z)}")
    alpha = int(alpha)
    if not 0 <= alpha <= 256:
        raise ValueError(f"alpha must be 0..256, got {alpha}")
    _, _, vmin, vmax = _range(0.0, 1.0, vmin, vmax)
    hist_data, rect_data, mask = hist_data.contiguous(), rect_data.contiguous(), mask.contiguous()
    hip.call("cfp_render_zones", hist_data.data_ptr(), rect_data.data_ptr(), mask.data_ptr(), Z, S, H, W, B, vmin, vmax,
             _lut(cmap, out.device).data_ptr(), alpha, out.data_ptr(), stride, pitch, hip.current_stream())
    return out


def demo_panel(rgb: torch.Tensor, pred: torch.Tensor, hist_data: torch.Tensor, rect_data: torch.Tensor, mask: torch.Tensor,
               gt: Optional[torch.Tensor] = None, lo: float = 1e-3, hi: float = 10.0, vmin: Optional[float] = None,
               vmax: Optional[float] = None, cmap: str = "magma_r", alpha: int = 160, error_kind: str = "abs", error_max: float = 1.0,
               error_cmap: str = "jet", mean=IMAGENET_MEAN, std=IMAGENET_STD, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [B,2H,2W,3] for rgb [B,3,H,W]: top left the image, top right the image under the zone overlay, bottom left the prediction,
    bottom right the error map when `gt` is given and white otherwise.  The prediction and the zones share the range [vmin, vmax]
    (default [lo, hi]) and the table `cmap`.  Five launches into one canvas; no intermediate tensor."""
    rgb = _rgb4(rgb)
    B, _, H, W = rgb.shape
    if out is None:
        out = torch.empty(B, 2 * H, 2 * W, 3, dtype=torch.uint8, device=rgb.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or not out.is_cuda or tuple(out.shape) != (B, 2 * H, 2 * W, 3):
        raise ValueError(f"out must be a uint8 device tensor {(B, 2 * H, 2 * W, 3)}")
    lo, hi, vmin, vmax = _range(lo, hi, vmin, vmax)
    rgb_image(rgb, mean, std, out=out[:, :H, :W])
    zones_overlay(rgb_image(rgb, mean, std, out=out[:, :H, W:]), hist_data, rect_data, mask, vmin, vmax, cmap, alpha)
    depth_image(pred, (H, W), lo, hi, vmin, vmax, cmap, out=out[:, H:, :W])
    if gt is not None:
        if tuple(_map3(gt, "gt").shape) != (B, H, W):
            raise ValueError(f"gt must be [B,H,W] = {(B, H, W)} like rgb")
        error_image(pred, gt, lo, hi, error_kind, error_max, error_cmap, out=out[:, H:, W:])
    else:
        out[:, H:, W:] = 255
    return out


# ---- host side -------------------------------------------------------------------------------------------------------------------------

def write_png(path: str, array) -> None:
    """uint8 [H,W,3] -> an RGB PNG, uint16 [H,W] -> a 16-bit greyscale PNG (tensor or array; Pillow)."""
    from PIL import Image
    if isinstance(array, torch.Tensor):
        array = array.detach().cpu().numpy()
    a = np.ascontiguousarray(array)
    if not ((a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3) or (a.dtype == np.uint16 and a.ndim == 2)):
        raise ValueError(f"array must be uint8 [H,W,3] or uint16 [H,W], got {a.dtype} {a.shape}")
    Image.fromarray(a).save(path, format="PNG")             # modes RGB and I;16
