"""`cfp_render_depth` / `cfp_render_zones` / `cfp_render_rgb` on the GPU against the numpy restatement of their definitions
(`render_ref.py`, itself checked in test_render_abi.py), the Python API around them and the picture switches of evaluate_all.py.

Acceptance, none of it measured on the kernels:
  exact tier      inputs on which every float32 intermediate is exact: byte equality on every pixel.
  realistic tier  the kernel's depth may differ from the restatement's by the project's own bound for that value,
                  |dd| <= 2e-5 * max(|d|, 1e-3) (tests/test_metrics.py); every pixel's colour (16-bit count) must be one the definition
                  yields for some d' in that interval -- plain equality wherever the interval crosses no boundary, which
                  test_render_abi.py shows to be all but a few per cent of the pixels.
  zones, rgb      exact-tier inputs (zone samples in multiples of 2^-6, the 256 byte values): byte equality; a random image under the
                  same interval rule for v * 255.
  destinations    the dword path and the byte path give the same bytes; bytes outside the rectangle keep their sentinel."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import pointcloud_ref as P
import render_ref as R

pytestmark = pytest.mark.gpu

from cfpnet_amd import hip, render as RD  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A
KINDS = {"depth": R.DEPTH, "gt": R.GT, "abs_err": R.ABS_ERR, "rel_err": R.REL_ERR}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)              # a copy: the shared inputs are read-only


def u16_filled(n):
    """uint16 [n] on the device holding 0x5A5A."""
    return torch.full((n,), 0x5A5A, dtype=torch.int16, device=DEV).view(torch.uint16)


def render_abi(what, pred, gt, H, W, interp, vmin, vmax, cmap="magma_r", u16=False, colour=True, scale=1000.0):
    """The C entry point itself -> (uint8 [B,H,W,3] or None, uint16 [B,H,W] or None) as numpy; both buffers carry a guard behind them."""
    use_pred, use_gt = what != R.GT, what != R.DEPTH
    p, g = (dev(pred) if use_pred else None), (dev(gt) if use_gt else None)
    B = (pred if use_pred else gt).shape[0]
    guard = 64
    out = torch.full((B * H * W * 3 + guard,), SENTINEL, dtype=torch.uint8, device=DEV) if colour else None
    mm = u16_filled(B * H * W + guard) if u16 else None
    hip.call("cfp_render_depth", hip.ptr(p), pred.shape[1] if use_pred else 0, pred.shape[2] if use_pred else 0, hip.ptr(g), H, W, B, interp,
             R.LO, R.HI, what, vmin, vmax, RD.colormap(cmap, DEV).data_ptr(), hip.ptr(out), H * W * 3, W, hip.ptr(mm), scale, hip.current_stream())
    res = []
    for t, n, shp in ((out, B * H * W * 3, (B, H, W, 3)), (mm, B * H * W, (B, H, W))):
        if t is None:
            res.append(None)
            continue
        a = t.cpu().numpy()
        assert (a[n:] == (SENTINEL if a.dtype == np.uint8 else 0x5A5A)).all()              # nothing beyond the last image
        res.append(a[:n].reshape(shp))
    return tuple(res)


# ---- 1. cfp_render_depth: every shape, every `what`, with and without the 16-bit plane, on both tiers ---------------------------------------

@pytest.mark.parametrize("name", list(R.CASES))
def test_render_depth_exact_tier(name):
    _, _, H, W, _ = R.shape(name)
    pred, gt = R.exact_inputs(name)
    lut = RD.colormap_table("magma_r")
    for kind, what in KINDS.items():
        vmin, vmax = R.EXACT_RANGE if what in (R.DEPTH, R.GT) else (0.0, 1.0)
        want = np.stack([R.render_depth(pred[b], gt[b], H, W, 0, what, vmin, vmax, lut) for b in range(pred.shape[0])])
        got, _ = render_abi(what, pred, gt, H, W, 0, vmin, vmax)
        diff = int((got != want).any(-1).sum())
        print(f"{name} {kind}: {diff} of {want.shape[0] * H * W} pixels differ from the restatement")
        assert diff == 0, (name, kind)
        if what in (R.DEPTH, R.GT):
            want_mm = np.stack([R.render_u16(pred[b], gt[b], H, W, 0, what, 1000.0) for b in range(pred.shape[0])])
            both, mm = render_abi(what, pred, gt, H, W, 0, vmin, vmax, u16=True)
            only, mm2 = render_abi(what, pred, gt, H, W, 0, vmin, vmax, u16=True, colour=False)
            assert only is None and both.tobytes() == got.tobytes() and mm.tobytes() == mm2.tobytes()
            assert np.array_equal(mm, want_mm), (name, kind, int((mm != want_mm).sum()))


@pytest.mark.parametrize("name", list(R.CASES))
def test_render_depth_realistic_tier(name):
    _, _, H, W, interp = R.shape(name)
    pred, gt = R.realistic_inputs(name)
    B = pred.shape[0]
    for i, (kind, what) in enumerate(KINDS.items()):
        vmin, vmax = R.COLOUR_RANGES[i % 3] if what in (R.DEPTH, R.GT) else (0.0, 1.0)
        cmap = "magma_r" if what in (R.DEPTH, R.GT) else "jet"
        lut = RD.colormap_table(cmap)
        got, _ = render_abi(what, pred, gt, H, W, interp, vmin, vmax, cmap)
        for b in range(B):
            R.check_colour(got[b], pred[b], gt[b], H, W, interp, what, vmin, vmax, lut, f"{name}[{b}] {kind}")
        if what in (R.DEPTH, R.GT):
            both, mm = render_abi(what, pred, gt, H, W, interp, vmin, vmax, cmap, u16=True)
            assert both.tobytes() == got.tobytes()
            for b in range(B):
                R.check_u16(mm[b], pred[b], gt[b], H, W, interp, what, 1000.0, f"{name}[{b}] {kind}")
    if name == "batch3_nonfinite":
        d = np.stack([P.depth(pred[b], H, W, interp) for b in range(B)])
        got, mm = render_abi(R.DEPTH, pred, gt, H, W, interp, 0.0, 5.0, u16=True)
        assert np.isnan(d[2]).any() and (got[np.isnan(d)] == 0).all() and (mm[np.isnan(d)] == 0).all() and not (got[~np.isnan(d)] == 0).all(-1).any()
    # the Python API takes the same route when its rule for `interpolate` (sizes differ) is the case's
    h, w = pred.shape[1:]
    if interp == int((h, w) != (H, W)):
        p, g = dev(pred), dev(gt)
        a = RD.depth_image(p, (H, W), vmin=0.0, vmax=5.0)
        assert a.shape == (B, H, W, 3) and a.dtype == torch.uint8 and a.cpu().numpy().tobytes() == render_abi(R.DEPTH, pred, gt, H, W, interp, 0.0, 5.0)[0].tobytes()
        assert RD.depth_image(p[:, None], (H, W)).cpu().numpy().tobytes() == render_abi(R.DEPTH, pred, gt, H, W, interp, R.LO, R.HI)[0].tobytes()
        mm = RD.depth_u16(p, (H, W))
        assert mm.dtype == torch.uint16 and mm.cpu().numpy().tobytes() == render_abi(R.DEPTH, pred, gt, H, W, interp, 0.0, 1.0, u16=True, colour=False)[1].tobytes()
        assert RD.gt_image(g, cmap="viridis").cpu().numpy().tobytes() == render_abi(R.GT, pred, gt, H, W, interp, R.LO, R.HI, "viridis")[0].tobytes()
        for kind in ("abs", "rel"):
            assert RD.error_image(p, g, kind=kind, vmax=0.5).cpu().numpy().tobytes() == \
                render_abi(KINDS[kind + "_err"], pred, gt, H, W, interp, 0.0, 0.5, "jet")[0].tobytes()


# ---- 2. destinations: canvas views, alignment, sentinels, repeatability -----------------------------------------------------------------------

def _canvas(B, Hc, Wc, extra=0):
    """A sentinel-filled uint8 canvas [B,Hc,Wc,3], `extra` bytes into a larger allocation (extra % 4 != 0: no dword path)."""
    buf = torch.full((B * Hc * Wc * 3 + 16,), SENTINEL, dtype=torch.uint8, device=DEV)
    return buf, buf[extra:extra + B * Hc * Wc * 3].view(B, Hc, Wc, 3)


def _only_the_rectangle_changed(buf, canvas, extra, y0, x0, H, W, want):
    a = buf.cpu().numpy()
    B, Hc, Wc, _ = canvas.shape
    img = a[extra:extra + B * Hc * Wc * 3].reshape(B, Hc, Wc, 3)
    assert img[:, y0:y0 + H, x0:x0 + W].tobytes() == want.tobytes()
    rest = np.ones(a.shape, bool)
    inner = np.zeros((B, Hc, Wc, 3), bool)
    inner[:, y0:y0 + H, x0:x0 + W] = True
    rest[extra:extra + B * Hc * Wc * 3] = ~inner.reshape(-1)
    assert (a[rest] == SENTINEL).all()


@pytest.mark.parametrize("name", ["odd_19x27_to_37x53", "same_24x40_interp"])
def test_canvas_destinations_give_the_same_bytes_and_touch_nothing_else(name):
    _, _, H, W, interp = R.shape(name)
    pred, gt = R.realistic_inputs(name)
    pred, gt = np.concatenate([pred, pred[:, ::-1]]), np.concatenate([gt, gt[:, ::-1]])          # two images
    p, g = dev(pred), dev(gt)
    plain = RD.depth_image(p, (H, W)).cpu().numpy()
    assert RD.depth_image(p, (H, W)).cpu().numpy().tobytes() == plain.tobytes()                  # two calls, identical bytes
    err = RD.error_image(p, g).cpu().numpy()
    Hc, Wc = H + 9, 4 * ((W + 13) // 4)                                                           # row pitch a multiple of 4 pixels
    seen = set()
    for extra, x0, wc in ((0, 4, Wc), (0, 5, Wc), (0, 4, Wc + 1), (3, 4, Wc), (8, 0, Wc)):
        buf, canvas = _canvas(2, Hc, wc, extra)
        view = canvas[:, 3:3 + H, x0:x0 + W]
        aligned = view.data_ptr() % 4 == 0 and wc % 4 == 0 and (Hc * wc * 3) % 4 == 0
        seen.add(aligned)
        assert RD.depth_image(p, (H, W), out=view) is view
        _only_the_rectangle_changed(buf, canvas, extra, 3, x0, H, W, plain)
        RD.error_image(p, g, out=view)                                                            # over what the rectangle held
        _only_the_rectangle_changed(buf, canvas, extra, 3, x0, H, W, err)
    assert seen == {True, False}                                                                  # both store paths ran
    # the 16-bit plane from a base that is not dword aligned
    want = RD.depth_u16(p, (H, W)).cpu().numpy()
    buf = u16_filled(2 * H * W + 8)
    hip.call("cfp_render_depth", p.data_ptr(), pred.shape[1], pred.shape[2], 0, H, W, 2, int(pred.shape[1:] != (H, W)), R.LO, R.HI, R.DEPTH, 0.0, 1.0, 0, 0, 0, 0,
             buf.data_ptr() + 2, 1000.0, hip.current_stream())
    a = buf.cpu().numpy()
    assert a[1:1 + 2 * H * W].tobytes() == want.tobytes() and a[0] == 0x5A5A and (a[1 + 2 * H * W:] == 0x5A5A).all()
    buf, canvas = _canvas(2, Hc, Wc)
    for bad in (dict(out=canvas[:, :H, :W + 1]), dict(out=canvas[:, :H, :W].float()), dict(out=canvas[:, :H, :W].cpu()), dict(cmap="rainbow"),
                dict(vmin=2.0, vmax=1.0), dict(lo=1.0, hi=1.0), dict(out=canvas[:, :H, 0:2 * W:2])):
        with pytest.raises(ValueError):
            RD.depth_image(p, (H, W), **bad)
    assert (canvas.cpu().numpy() == SENTINEL).all()                                                # a refusal writes nothing


# ---- 3. cfp_render_zones -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Z", [64, 16])
@pytest.mark.parametrize("kind", ["centered", "pitched", "overhang"])
def test_zones_overlay(kind, Z):
    B, H, W = 2, 45, 62
    hist, mask = R.zone_inputs(Z, B)
    rect = np.stack([R.zone_rects(kind, H, W, Z)] * B)
    if kind == "pitched":
        rect[1] = rect[1] + np.float32(0.5)                                                      # per-image rectangles
    lut = RD.colormap_table("magma_r")
    rng = np.random.default_rng(Z)
    base = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    h, r, m = dev(hist), dev(rect), dev(mask)
    in_zone = np.stack([R.zone_of(rect[b].astype(np.float32), H, W) >= 0 for b in range(B)])
    assert in_zone.any() and (kind == "overhang") == bool(in_zone.all())
    for alpha in (0, 160, 256):
        want = np.stack([R.render_zones(base[b], hist[b], rect[b], mask[b], *R.EXACT_RANGE, lut, alpha) for b in range(B)])
        out = dev(base)
        assert RD.zones_overlay(out, h, r, m, *R.EXACT_RANGE, alpha=alpha) is out
        got = out.cpu().numpy()
        assert np.array_equal(got, want), (kind, Z, alpha, int((got != want).any(-1).sum()))
        assert np.array_equal(got[~in_zone], base[~in_zone])                                      # outside every zone: untouched
        if alpha == 0:
            assert np.array_equal(got, base)
        if alpha == 256:
            assert ((got[in_zone] == 0).all(-1)).any() and (((got == 128).all(-1)) & in_zone).any()      # borders and dropped zones
        # the same into an unaligned view of a wider canvas: same bytes, nothing else touched
        buf, canvas = _canvas(B, H + 4, W + 7, 1)
        view = canvas[:, 2:2 + H, 3:3 + W]
        view.copy_(dev(base))
        RD.zones_overlay(view, h, r, m, *R.EXACT_RANGE, alpha=alpha)
        _only_the_rectangle_changed(buf, canvas, 1, 2, 3, H, W, want)
    for bad in (dict(alpha=257), dict(alpha=-1), dict(vmin=1.0, vmax=1.0), dict(cmap="rainbow")):
        kw = dict(vmin=0.0, vmax=8.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            RD.zones_overlay(dev(base), h, r, m, **kw)
    for args in ((h[:1], r, m), (h, r[:, :3], m), (h, r, m.float()), (h.double(), r, m), (h, r, m[:, :3])):
        with pytest.raises(ValueError):
            RD.zones_overlay(dev(base), *args, 0.0, 8.0)


def test_zones_overlay_with_the_most_zones_and_overlapping_ones():
    """Z = 256 (the kernel looks for candidate zones 64 at a time) on a 16 x 16 grid, and zones that overlap: the first in index order wins."""
    B, H, W = 2, 45, 62
    h64, m64 = R.zone_inputs(64, B)
    hist, mask = np.tile(h64, (1, 4, 1)), np.tile(m64, (1, 4))
    hist[:, 64:] += np.float32(0.5)
    rect = np.stack([R.zone_rects("overhang", H, W, 256), R.zone_rects("centered", H, W, 256)])
    rect[1, 200] = (3.0, 5.0, 40.0, 50.0)                                                         # a late zone under the earlier ones
    rect[1, 0] = (20.0, 30.0, 44.5, 61.5)                                                          # an early one over the later ones
    lut = RD.colormap_table("turbo")
    base = np.random.default_rng(5).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    z_of = R.zone_of(rect[1], H, W)
    assert (z_of == 200).any() and (z_of == 0).sum() > 300 and len(np.unique(z_of)) > 100
    for alpha in (160, 256):
        want = np.stack([R.render_zones(base[b], hist[b], rect[b], mask[b], *R.EXACT_RANGE, lut, alpha) for b in range(B)])
        got = RD.zones_overlay(dev(base), dev(hist), dev(rect), dev(mask), *R.EXACT_RANGE, cmap="turbo", alpha=alpha).cpu().numpy()
        assert np.array_equal(got, want), (alpha, int((got != want).any(-1).sum()))
    with pytest.raises(ValueError, match="Z <= 256"):
        RD.zones_overlay(dev(base), dev(np.tile(hist, (1, 2, 1))), dev(np.tile(rect, (1, 2, 1))), dev(np.tile(mask, (1, 2))), 0.0, 8.0)


# ---- 4. cfp_render_rgb---------------------------------------------------------------------------------------------------------------------

def test_rgb_image():
    x, want = R.byte_round_trip()
    got = RD.rgb_image(dev(x[None]))
    assert got.shape == (1, 16, 16, 3) and np.array_equal(got[0].cpu().numpy(), want)             # every byte value comes back
    from cfpnet_amd import synthetic
    rgb = synthetic.make_inputs(2, seed=11)["rgb"].numpy()[:, :, :37, :53].copy()
    rgb[1, :, 3, 4:7] = (np.nan, -40.0, 40.0)
    got = RD.rgb_image(dev(rgb)).cpu().numpy()
    for b in range(2):
        R.check_rgb(got[b], rgb[b], f"rgb[{b}]")
    assert got[1, 3, 4:7].tolist() == [[0] * 3, [0] * 3, [255] * 3]
    wide = np.ascontiguousarray(np.pad(rgb, ((0, 0), (0, 0), (0, 0), (0, 3))))                    # W = 56: the 16-byte loads
    assert RD.rgb_image(dev(wide)).cpu().numpy()[:, :, :53].tobytes() == got.tobytes()
    for extra, x0 in ((0, 4), (1, 3)):
        buf, canvas = _canvas(2, 40, 64, extra)
        RD.rgb_image(dev(rgb), out=canvas[:, 1:38, x0:x0 + 53])
        _only_the_rectangle_changed(buf, canvas, extra, 1, x0, 37, 53, got)
    other = RD.rgb_image(dev(rgb), mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25)).cpu().numpy()
    assert np.array_equal(other[0], R.render_rgb(rgb[0], (0.5, 0.5, 0.5), (0.25, 0.25, 0.25)))
    for bad in (dict(mean=(0.5, 0.5)), dict(std=(1.0, float("nan"), 1.0)), dict(out=torch.zeros(2, 37, 53, 3, device=DEV))):
        with pytest.raises(ValueError):
            RD.rgb_image(dev(rgb), **bad)
    with pytest.raises(ValueError, match=r"\[B,3,H,W\]"):
        RD.rgb_image(dev(rgb[:, :2]))


# ---- 5. the panel --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(38, 54), (37, 53)])
def test_demo_panel_is_the_five_pieces(H, W):
    from cfpnet_amd import synthetic
    B, Z = 2, 64
    pred = np.stack([synthetic.make_eval_pair(H, W, 19, 27, 41 + b, 0.1, 0.15)[1] for b in range(B)])
    gt = np.stack([synthetic.make_eval_pair(H, W, 19, 27, 41 + b, 0.1, 0.15)[0] for b in range(B)])
    rgb = synthetic.make_inputs(B, seed=12)["rgb"].numpy()[:, :, :H, :W].copy()
    hist, mask = R.zone_inputs(Z, B)
    rect = np.stack([R.zone_rects("pitched", H, W, Z)] * B)
    p, g, x, h, r, m = (dev(a) for a in (pred, gt, rgb, hist, rect, mask))
    panel = RD.demo_panel(x, p, h, r, m, g, vmin=0.0, vmax=5.0, cmap="turbo", alpha=200, error_kind="rel", error_max=0.5)
    assert panel.shape == (B, 2 * H, 2 * W, 3) and panel.dtype == torch.uint8
    tl = RD.rgb_image(x)
    tr = RD.zones_overlay(RD.rgb_image(x), h, r, m, 0.0, 5.0, "turbo", 200)
    bl = RD.depth_image(p, (H, W), vmin=0.0, vmax=5.0, cmap="turbo")
    br = RD.error_image(p, g, kind="rel", vmax=0.5)
    assert not torch.equal(tl, tr)
    for piece, ys, xs in ((tl, 0, 0), (tr, 0, W), (bl, H, 0), (br, H, W)):
        assert torch.equal(panel[:, ys:ys + H, xs:xs + W], piece)
    # without ground truth the fourth quarter is white; `out=` is written in place
    into = torch.full((B, 2 * H, 2 * W, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    res = RD.demo_panel(x, p, h, r, m, out=into)
    assert res is into and (into[:, H:, W:] == 255).all() and torch.equal(into[:, :H, :W], tl)
    assert torch.equal(into[:, H:, :W], RD.depth_image(p, (H, W)))
    assert torch.equal(into[:, :H, W:], RD.zones_overlay(RD.rgb_image(x), h, r, m, R.LO, R.HI))
    with pytest.raises(ValueError, match="out must be"):
        RD.demo_panel(x, p, h, r, m, out=into[:, :-1])
    with pytest.raises(ValueError, match="gt must be"):
        RD.demo_panel(x, p, h, r, m, g[:, :-1])


# ---- 6. the command line -------------------------------------------------------------------------------------------------------------------

BASE = ["@configs/cfpnet_combine1.txt", "--selected_epoch", "best", "--synthetic", "2", "--batch", "2"]


def _cli(argv):
    import evaluate_all
    out, err = io.StringIO(), io.StringIO()
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
            res = evaluate_all.main(list(argv))
    finally:
        os.chdir(cwd)
    return res, out.getvalue().splitlines(), err.getvalue().splitlines()


def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im).copy()


def test_cli_picture_switches(tmp_path, monkeypatch):
    plain, lines0, err0 = _cli(BASE)
    calls = {}
    names = ("depth_image", "depth_u16", "gt_image", "rgb_image", "error_image", "demo_panel")
    real = {n: getattr(RD, n) for n in names}

    def recorder(name):
        def fn(*a, **kw):
            if "out" not in kw:                          # the pieces demo_panel renders into its canvas are not the command line's calls
                keep = lambda v: v.clone() if isinstance(v, torch.Tensor) else v
                calls.setdefault(name, []).append(([keep(v) for v in a], {k: keep(v) for k, v in kw.items()}))
            return real[name](*a, **kw)
        return fn

    for n in names:
        monkeypatch.setattr(RD, n, recorder(n))
    res, lines, err = _cli(BASE + ["--save_pred", "--save_gt", "--save_rgb", "--save_error_map", "--save_for_demo", "--vis_range", "0.5,6",
                                   "--vis_cmap", "viridis", "--error_max", "2", "--save_dir", str(tmp_path)])
    monkeypatch.undo()
    assert res == plain and lines == lines0 and len(lines) == 2                  # stdout does not change
    assert sum(l.startswith("pictures: ") for l in err) == 1 and "12 files" in err[-2] and not any(l.startswith("pictures") for l in err0)
    stems = ("pred_{}.png", "pred_{}_mm.png", "gt_{}.png", "rgb_{}.png", "error_{}.png", "demo_{}.png")
    assert sorted(os.listdir(str(tmp_path))) == sorted(s.format(i) for s in stems for i in range(2))
    assert all(len(calls[n]) == 1 for n in names)
    for name, stem in zip(names, ("pred_{}.png", "pred_{}_mm.png", "gt_{}.png", "rgb_{}.png", "error_{}.png", "demo_{}.png")):
        a, kw = calls[name][0]
        direct = real[name](*a, **kw).cpu().numpy()                               # the API called directly on what the model produced
        for i in range(2):
            got = _png(os.path.join(str(tmp_path), stem.format(i)))
            assert got.shape == direct[i].shape and np.array_equal(got.astype(direct.dtype), direct[i]), (name, i)
    a, _ = calls["depth_image"][0]
    pred = a[0]
    assert tuple(a[1]) == (480, 640) and a[2:] == [1e-3, 10.0, 0.5, 6.0, "viridis"] and calls["error_image"][0][0][2:] == [1e-3, 10.0, "abs", 2.0]
    assert _png(os.path.join(str(tmp_path), "demo_0.png")).shape == (960, 1280, 3)
    pn = pred.cpu().numpy().reshape(2, 240, 320)
    for i in range(2):
        mm = _png(os.path.join(str(tmp_path), f"pred_{i}_mm.png")).astype(np.float64) / 1000.0
        d = P.depth(pn[i], 480, 640, 1).astype(np.float64)
        worst = float((np.abs(mm - d) - R.RTOL * np.maximum(np.abs(d), 1e-3)).max())
        print(f"cli: pred_{i}_mm.png / 1000 vs the clipped, enlarged prediction: worst excess over RTOL {worst * 1e3:.4f} mm (allowed 0.5)")
        assert worst <= 0.5e-3
    with pytest.raises(ValueError, match="need one of --save_pred"):                      # the --vis / --error switches alone are an error
        _cli(BASE + ["--vis_cmap", "jet"])
