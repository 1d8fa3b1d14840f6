"""`cfp_render_depth` / `cfp_render_zones` / `cfp_render_rgb` without a GPU: the symbols, the header and the Makefile, every argument
check (dummy pointers: no kernel is launched), the Python API's and the command line's own refusals, the colour tables against
matplotlib (where it is installed), the numpy restatement (`render_ref.py`) against matplotlib's lookup and on its exact tier, the caps
on the share of pixels whose accepted interval crosses a boundary, and the PNG writer."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import render_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE = -1, -2
NAMES = ("magma_r", "magma", "viridis", "turbo", "jet")


@pytest.fixture(scope="module")
def lib():
    from cfpnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.load()


def test_symbols_header_and_makefile(lib):
    from cfpnet_amd import hip
    for name in ("cfp_render_depth", "cfp_render_zones", "cfp_render_rgb"):
        assert hasattr(lib, name)
    text = open(os.path.join(ROOT, "include", "cfpnet_hip.h")).read()
    assert "int cfp_render_depth(const float* pred, int Hp, int Wp, const float* gt, int H, int W, int B, int interpolate, float lo, float hi," in text
    assert "int cfp_render_zones(const float* hist" in text and "int cfp_render_rgb(const float* rgb" in text
    assert "enum { CFP_RENDER_DEPTH = 0, CFP_RENDER_GT = 1, CFP_RENDER_ABS_ERR = 2, CFP_RENDER_REL_ERR = 3 };" in text
    for cited in ("src/utils/utils.py:44-64", "evaluate_all.py:40-41", "out[b * image_stride + (y * pitch + x) * 3 + c]",
                  "t = (v - vmin) / (vmax - vmin) * 256.f", "lut[(int)t]", "(uint16_t)rintf(m)", "(c * alpha + out * (256 - alpha) + 128) >> 8",
                  "y < sy + 1 || y >= ey - 1 || x < sx + 1 || x >= ex - 1", "v = x * std[c] + mean[c]", "(uint8_t)rintf(v * 255.f)"):
        assert cited in text, cited
    assert (hip.RENDER_DEPTH, hip.RENDER_GT, hip.RENDER_ABS_ERR, hip.RENDER_REL_ERR) == (R.DEPTH, R.GT, R.ABS_ERR, R.REL_ERR) == (0, 1, 2, 3)
    assert len(hip.SIGNATURES["cfp_render_depth"][1]) == 20 and len(hip.SIGNATURES["cfp_render_zones"][1]) == 16
    assert len(hip.SIGNATURES["cfp_render_rgb"][1]) == 10
    mk = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "Makefile")).read()
    dep = [l for l in mk.splitlines() if l.endswith(": metrics_pred.h")]
    assert " render.hip " in mk and len(dep) == 1 and " render.o " in dep[0] and "-ffp-contract=off" in mk
    src = open(os.path.join(ROOT, "cfpnet_amd", "csrc", "render.hip")).read()
    assert '#include "metrics_pred.h"' in src and "met_pred(" in src and "atomic" not in src.replace("no atomics", "")
    for py in sorted(f for f in os.listdir(os.path.join(ROOT, "cfpnet_amd")) if f.endswith(".py")):        # nothing in the package imports it
        assert not re.search(r"^\s*(import|from)\s+matplotlib", open(os.path.join(ROOT, "cfpnet_amd", py)).read(), re.M), py


# ---- argument checks of the C entry points -------------------------------------------------------------------------------------------------

P = 16        # a non-null, aligned dummy device pointer: every case below fails a check before anything is dereferenced or launched


def test_render_depth_refuses_bad_arguments_with_a_message(lib):
    from cfpnet_amd import hip

    def call(pred=P, hp=8, wp=8, gt=P, h=8, w=8, b=1, interp=0, lo=1e-3, hi=10.0, what=R.DEPTH, vmin=0.0, vmax=1.0, lut=P, out=P,
             stride=8 * 8 * 3, pitch=8, u16=0, scale=1000.0):
        rc = lib.cfp_render_depth(pred, hp, wp, gt, h, w, b, interp, lo, hi, what, vmin, vmax, lut, out, stride, pitch, u16, scale, 0)
        return rc, hip.last_error()

    for kw in (dict(b=0), dict(h=0), dict(w=-1), dict(hp=0), dict(wp=-3), dict(what=R.ABS_ERR, hp=-1)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "cfp_render_depth: non-positive" in msg, (kw, rc, msg)
    for kw in (dict(hp=4, wp=4), dict(hp=8, wp=4), dict(h=16, w=16, stride=16 * 16 * 3, pitch=16), dict(what=R.REL_ERR, hp=4)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "sizes differ" in msg, (kw, rc, msg)
    rc, msg = call(h=70000, w=70000, interp=1)
    assert rc == ESHAPE and "too large" in msg
    for kw in (dict(pitch=7), dict(pitch=0), dict(pitch=-8)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "pitch is smaller than W" in msg, (kw, rc, msg)
    for kw in (dict(stride=8 * 8 * 3 - 1), dict(stride=0), dict(pitch=9), dict(stride=-192)):
        rc, msg = call(**kw)
        assert rc == ESHAPE and "image_stride is smaller" in msg, (kw, rc, msg)
    # a NULL pointer the chosen `what` needs
    for kw in (dict(pred=0), dict(what=R.GT, gt=0), dict(what=R.ABS_ERR, gt=0), dict(what=R.ABS_ERR, pred=0), dict(what=R.REL_ERR, pred=0),
               dict(what=R.REL_ERR, gt=0)):
        rc, msg = call(**kw)
        assert rc == EINVAL and "cfp_render_depth: null pointer" in msg, (kw, rc, msg)
    rc, msg = call(lut=0)
    assert rc == EINVAL and "null pointer (lut)" in msg
    rc, msg = call(out=0)
    assert rc == EINVAL and "both null" in msg
    for what in (R.ABS_ERR, R.REL_ERR):
        rc, msg = call(what=what, u16=P)
        assert rc == EINVAL and "DEPTH and GT only" in msg, (what, rc, msg)
    for what in (-1, 4, 17):
        rc, msg = call(what=what)
        assert rc == EINVAL and "unknown what" in msg, (what, rc, msg)
    for vmin, vmax in ((1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.0, float("nan")), (0.0, float("inf")), (float("-inf"), 1.0)):
        rc, msg = call(vmin=vmin, vmax=vmax)
        assert rc == EINVAL and "vmin < vmax" in msg, (vmin, vmax, rc, msg)
    for lo, hi in ((2.0, 1.0), (1.0, 1.0), (float("nan"), 1.0), (0.0, float("nan"))):
        rc, msg = call(lo=lo, hi=hi)
        assert rc == EINVAL and "empty depth range" in msg, (lo, hi, rc, msg)
    for scale in (0.0, -1000.0, float("nan"), float("inf")):
        rc, msg = call(u16=P, scale=scale)
        assert rc == EINVAL and "u16_scale" in msg, (scale, rc, msg)
    with pytest.raises(RuntimeError, match="cfp_render_depth failed"):
        hip.call("cfp_render_depth", P, 4, 4, 0, 8, 8, 1, 0, 1e-3, 10.0, 0, 0.0, 1.0, P, P, 192, 8, 0, 1000.0, 0)


def test_render_zones_and_rgb_refuse_bad_arguments_with_a_message(lib):
    from cfpnet_amd import hip

    def zones(hist=P, rect=P, mask=P, z=64, s=16, h=8, w=8, b=1, vmin=0.0, vmax=1.0, lut=P, alpha=160, out=P, stride=192, pitch=8):
        rc = lib.cfp_render_zones(hist, rect, mask, z, s, h, w, b, vmin, vmax, lut, alpha, out, stride, pitch, 0)
        return rc, hip.last_error()

    for kw in (dict(b=0), dict(h=-1), dict(w=0)):
        rc, msg = zones(**kw)
        assert rc == ESHAPE and "cfp_render_zones: non-positive" in msg, (kw, rc, msg)
    for kw in (dict(z=0), dict(z=-4), dict(s=0), dict(z=257)):
        rc, msg = zones(**kw)
        assert rc == ESHAPE and "Z must be 1..256 and S positive" in msg, (kw, rc, msg)
    for kw, text in ((dict(pitch=7), "pitch is smaller"), (dict(stride=191), "image_stride is smaller")):
        rc, msg = zones(**kw)
        assert rc == ESHAPE and "cfp_render_zones: " + text in msg, (kw, rc, msg)
    for name in ("hist", "rect", "mask", "lut", "out"):
        rc, msg = zones(**{name: 0})
        assert rc == EINVAL and "cfp_render_zones: null pointer" in msg, (name, rc, msg)
    for alpha in (-1, 257, 1000):
        rc, msg = zones(alpha=alpha)
        assert rc == EINVAL and "alpha must be 0..256" in msg, (alpha, rc, msg)
    for vmin, vmax in ((1.0, 1.0), (float("nan"), 1.0), (0.0, float("inf"))):
        rc, msg = zones(vmin=vmin, vmax=vmax)
        assert rc == EINVAL and "vmin < vmax" in msg, (vmin, vmax, rc, msg)

    three = ctypes.c_float * 3
    mean, std = three(*R.MEAN), three(*R.STD)

    def rgb(src=P, mean=mean, std=std, h=8, w=8, b=1, out=P, stride=192, pitch=8):
        rc = lib.cfp_render_rgb(src, mean, std, h, w, b, out, stride, pitch, 0)
        return rc, hip.last_error()

    for kw in (dict(b=0), dict(h=0), dict(w=-2)):
        rc, msg = rgb(**kw)
        assert rc == ESHAPE and "cfp_render_rgb: non-positive" in msg, (kw, rc, msg)
    for kw, text in ((dict(pitch=4), "pitch is smaller"), (dict(pitch=16), "image_stride is smaller")):
        rc, msg = rgb(**kw)
        assert rc == ESHAPE and "cfp_render_rgb: " + text in msg, (kw, rc, msg)
    for kw in (dict(src=0), dict(out=0), dict(mean=None), dict(std=None)):
        rc, msg = rgb(**kw)
        assert rc == EINVAL and "cfp_render_rgb: null pointer" in msg, (kw, rc, msg)
    rc, msg = rgb(std=three(0.2, float("nan"), 0.2))
    assert rc == EINVAL and "finite" in msg


# ---- Python and command line ---------------------------------------------------------------------------------------------------------------

def test_python_api_refuses_before_anything_runs():
    import torch
    from cfpnet_amd import render as RD
    assert list(inspect.signature(RD.depth_image).parameters) == ["pred", "size", "lo", "hi", "vmin", "vmax", "cmap", "out"]
    sig = inspect.signature(RD.error_image)
    assert list(sig.parameters) == ["pred", "gt", "lo", "hi", "kind", "vmax", "cmap", "out"]
    assert sig.parameters["kind"].default == "abs" and sig.parameters["vmax"].default == 1.0 and sig.parameters["cmap"].default == "jet"
    assert inspect.signature(RD.depth_image).parameters["cmap"].default == "magma_r"
    assert inspect.signature(RD.depth_u16).parameters["scale"].default == 1000.0
    assert inspect.signature(RD.zones_overlay).parameters["alpha"].default == 160
    assert np.array_equal(np.float32(RD.IMAGENET_MEAN), R.MEAN) and np.array_equal(np.float32(RD.IMAGENET_STD), R.STD)
    host = torch.ones(1, 4, 6)
    for fn in (RD.depth_image, RD.depth_u16, RD.gt_image):
        for bad in (host, host.double(), np.ones((1, 4, 6), np.float32)):
            with pytest.raises(ValueError, match="(pred|gt) must be a float32 device tensor"):
                fn(bad)
    with pytest.raises(ValueError, match="pred must be a float32 device tensor"):
        RD.error_image(host, host)
    with pytest.raises(ValueError, match="kind must be"):
        RD.error_image(host, host, kind="squared")
    with pytest.raises(ValueError, match="rgb must be a float32 device tensor"):
        RD.rgb_image(torch.ones(1, 3, 4, 6))
    with pytest.raises(ValueError, match="out must be a uint8 device tensor"):
        RD.zones_overlay(torch.zeros(1, 4, 6, 3, dtype=torch.uint8), host, host, host, 0.0, 1.0)
    with pytest.raises(ValueError, match="rgb must be a float32 device tensor"):
        RD.demo_panel(torch.ones(1, 3, 4, 6), host, host, host, host)
    # the helpers behind the remaining refusals take no device
    for bad in (torch.ones(4, 6), torch.ones(1, 2, 4, 6), torch.ones(0, 4, 6)):
        with pytest.raises(ValueError):
            RD._map3(bad, "pred")
    for bad in ((0, 4), (4, -1), 7, (1, 2, 3), "ab"):
        with pytest.raises(ValueError, match="size"):
            RD._size(bad, 4, 4)
    assert RD._size(None, 120, 160) == (240, 320)
    assert RD._range(1e-3, 10.0, None, None) == (1e-3, 10.0, 1e-3, 10.0) and RD._range(1e-3, 10.0, 0.0, 5) == (1e-3, 10.0, 0.0, 5.0)
    for bad in ((2.0, 1.0, None, None), (float("nan"), 1.0, None, None)):
        with pytest.raises(ValueError, match="lo = .* hi = "):
            RD._range(*bad)
    for bad in ((0.0, 1.0, 1.0, 1.0), (0.0, 1.0, 3.0, 2.0), (0.0, 1.0, float("nan"), 2.0), (0.0, float("inf"), None, None)):
        with pytest.raises(ValueError, match="vmin = .* vmax = "):
            RD._range(*bad)
    with pytest.raises(ValueError, match="cmap must be one of .*magma_r"):
        RD.colormap_table("rainbow")
    with pytest.raises(ValueError, match="cmap"):
        RD._lut(3, "cpu")
    for bad in ((1.0, 2.0), (1.0, float("nan"), 2.0), 5.0):
        with pytest.raises(ValueError, match="mean must be 3"):
            RD._three(bad, "mean")
    # `out`: shape, dtype, device and layout.  _dest looks at the device first, so host tensors show the other refusals through a
    # stand-in that claims to be on the device
    class OnDevice(torch.Tensor):
        is_cuda = property(lambda self: True)

    def fake(t):
        return t.as_subclass(OnDevice)

    canvas = torch.zeros(2, 10, 12, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="out must be a uint8 device tensor"):
        RD._dest(canvas[:, :5, :6], 2, 5, 6, "cpu")                      # not on the device
    with pytest.raises(ValueError, match="out must be a uint8 device tensor"):
        RD._dest(fake(canvas[:, :5, :6]), 2, 5, 7, "cpu")                # another shape
    with pytest.raises(ValueError, match="out must be a uint8 device tensor"):
        RD._dest(fake(canvas.float()[:, :5, :6]), 2, 5, 6, "cpu")
    view = fake(canvas[:, 5:, 6:])
    out, stride, pitch = RD._dest(view, 2, 5, 6, "cpu")
    assert out is view and stride == 10 * 12 * 3 and pitch == 12
    with pytest.raises(ValueError, match="3 adjacent bytes"):
        RD._dest(fake(canvas[:, :5, ::2]), 2, 5, 6, "cpu")               # every other pixel
    with pytest.raises(ValueError, match="3 adjacent bytes"):
        RD._dest(fake(torch.zeros(2, 3, 5, 6, dtype=torch.uint8).permute(0, 2, 3, 1)), 2, 5, 6, "cpu")     # planar
    with pytest.raises(ValueError, match="images overlap"):
        RD._dest(fake(torch.zeros(1, 5, 6, 3, dtype=torch.uint8).expand(2, 5, 6, 3)), 2, 5, 6, "cpu")
    with pytest.raises(ValueError, match=r"uint8 \[H,W,3\] or uint16 \[H,W\]"):
        RD.write_png("x.png", np.zeros((4, 4), np.uint8))
    assert not os.path.exists("x.png")


def test_evaluate_all_refuses_the_vis_switches_alone_and_an_unknown_table():
    import evaluate_all
    argv = ["--synthetic", "2", "--save_pred", "--vis_cmap", "turbo", "--vis_range", "0.5,3", "--error_max", "0.5", "--error_rel", "--save_dir", "o"]
    assert evaluate_all._pop(argv, "--vis_cmap", None) == "turbo"
    assert evaluate_all._pop(argv, "--vis_range", None, evaluate_all._vis_range) == (0.5, 3.0)
    assert evaluate_all._pop(argv, "--error_max", None, float) == 0.5 and evaluate_all._pop(argv, "--error_rel", False, None) is True
    assert argv == ["--synthetic", "2", "--save_pred", "--save_dir", "o"]          # the reference's own switches stay for its parser
    for bad in ("1", "3,1", "1,1", "1,2,3"):
        with pytest.raises(ValueError, match="--vis_range"):
            evaluate_all._vis_range(bad)
    src = inspect.getsource(evaluate_all.main)
    for flag in ("--vis_cmap", "--vis_range", "--error_max", "--error_rel"):
        assert f'_pop(argv, "{flag}"' in src, flag
    # raised before a device or a model is touched
    for extra in (["--vis_cmap", "jet"], ["--vis_range", "0,5"], ["--error_max", "2"], ["--error_rel"]):
        with pytest.raises(ValueError, match="need one of --save_pred, --save_gt, --save_rgb, --save_error_map, --save_for_demo"):
            evaluate_all.main(["--synthetic", "2"] + extra)
    for switch in ("--save_pred", "--save_for_demo"):
        with pytest.raises(ValueError, match="cmap must be one of"):
            evaluate_all.main(["--synthetic", "2", switch, "--vis_cmap", "rainbow"])
    with pytest.raises(ValueError, match="--error_max must be positive"):
        evaluate_all.main(["--synthetic", "2", "--save_error_map", "--error_max", "0"])


# ---- the tables and the lookup against matplotlib ---------------------------------------------------------------------------------------------

def test_tables():
    from cfpnet_amd import render as RD
    assert RD.COLORMAPS == NAMES
    from cfpnet_amd import colormaps
    assert colormaps.NAMES == NAMES and not [f for f in os.listdir(os.path.join(ROOT, "cfpnet_amd")) if f.endswith((".npz", ".npy"))]
    # the bytes of the five tables, pinned where matplotlib is not installed
    import hashlib
    assert hashlib.sha256(b"".join(colormaps.table(n).tobytes() for n in NAMES)).hexdigest() == \
        "1e78a3e33b3574360f47b9af53c3edbb1d9ab0a596dadae3b3633a3605f43cfb"
    for n in NAMES:
        t = RD.colormap_table(n)
        assert t.shape == (256, 3) and t.dtype == np.uint8 and not t.flags.writeable
    assert np.array_equal(RD.colormap_table("magma_r"), RD.colormap_table("magma")[::-1])
    assert RD.colormap("jet", "cpu") is RD.colormap("jet", "cpu") and RD.colormap("jet", "cpu").dtype.__str__() == "torch.uint8"
    assert np.array_equal(RD.colormap("jet", "cpu").numpy(), RD.colormap_table("jet"))
    matplotlib = pytest.importorskip("matplotlib")
    for n in NAMES:
        assert np.array_equal(RD.colormap_table(n), matplotlib.colormaps[n](np.arange(256), bytes=True)[:, :3]), n


def test_the_restatements_lookup_is_matplotlibs_rule_for_float_input():
    matplotlib = pytest.importorskip("matplotlib")
    from cfpnet_amd import render as RD
    # x in [-0.5, 1.5] in steps of 2^-12 (x * 256 exact in float32), 1.0 among them, and the specials
    x = np.concatenate([np.arange(-2048, 6145, dtype=np.float32) / np.float32(4096), np.array([np.nan, np.inf, -np.inf, 1.0, 0.0, -0.0], np.float32)])
    for n in NAMES:
        lut = RD.colormap_table(n)
        want = matplotlib.colormaps[n](x.copy(), bytes=True)[:, :3]
        got = R.lookup(x, 0.0, 1.0, lut)
        assert np.array_equal(got, want), n
        assert (got[-6] == 0).all() and (got[-5] == lut[255]).all() and (got[-4] == lut[0]).all() and (got[-3] == lut[255]).all()
    # through a range: v = vmin + x * (vmax - vmin) with everything exact
    v = np.float32(0.5) + x[:-6] * np.float32(4)
    assert np.array_equal(R.lookup(v, 0.5, 4.5, RD.colormap_table("jet")), matplotlib.colormaps["jet"](x[:-6].copy(), bytes=True)[:, :3])


# ---- the restatement on its exact tier -----------------------------------------------------------------------------------------------------

def test_exact_tier_is_exact_in_float32():
    """t = k / 2 and v * 1000 = k * 15.625 without a rounding for the depths k / 64, 60 of the 481 values are .5 ties in millimetres
    (which pins round-half-even), the zone samples sum without a rounding, and every byte value comes back through the normalisation."""
    k = np.arange(32, 513)
    v = k.astype(np.float32) / np.float32(64)
    t = ((v - np.float32(0)) / (np.float32(8) - np.float32(0))) * np.float32(256)
    assert np.array_equal(t.astype(np.float64), k / 2) and np.array_equal(R.lut_index(v, *R.EXACT_RANGE), np.minimum(k // 2, 255))
    mm = v * np.float32(1000)
    assert np.array_equal(mm.astype(np.float64), k * 15.625)
    ties = (k * 15.625) % 1 == 0.5
    assert ties.sum() == 60
    want = np.floor(k * 15.625 + 0.5)
    want[ties] = 2 * np.round(k[ties] * 15.625 / 2)                         # the even neighbour
    assert np.array_equal(R.u16_count(v, 1000.0), want.astype(np.uint16)) and (want[ties] % 2 == 0).all()
    assert R.u16_count(np.array([np.nan, -1.0, 0.0, 65.5345, 65.535, 70.0, np.inf], np.float32), 1000.0).tolist() == [0, 0, 0, 65534, 65535, 65535, 65535]
    pred, gt = R.exact_inputs("same_24x40_direct")
    finite = pred[np.isfinite(pred) & (pred >= 0.5) & (pred <= 8)]
    assert set(np.rint(finite * 64).astype(int)) == set(range(32, 513)) and np.isnan(pred).sum() == 1 and np.isinf(pred).sum() == 2
    ok = R.painted(R.ABS_ERR, gt[0], R.LO, R.HI, gt[0].shape)
    assert 0 < (~ok).sum() <= 6 and np.isnan(pred[0][ok]).any() and (pred[0][ok] > 30).any()      # special predictions on valid ground truth
    hist, mask = R.zone_inputs(64)
    s32 = hist[..., 0].copy()
    for j in range(1, 16):
        s32 = s32 + hist[..., j]
    assert np.array_equal(s32.astype(np.float64), hist.astype(np.float64).sum(-1))
    assert np.array_equal((s32 / np.float32(16)).astype(np.float64) * 16, hist.astype(np.float64).sum(-1))
    x, want = R.byte_round_trip()
    v = R.denorm(x)
    worst = float(np.abs(v.astype(np.float64) * 255 - want).max())
    print(f"byte round trip: de-normalised value within {worst / 255:.2e} of u / 255")
    assert worst <= 255 * 1.8e-5 and np.array_equal(R.render_rgb(x), want)
    assert R.render_rgb(np.array([np.nan, -9.0, 9.0], np.float32).reshape(1, 1, 3).repeat(3, 0)).reshape(-1).tolist() == [0] * 3 + [0] * 3 + [255] * 3


def test_restated_pictures_on_the_exact_tier():
    from cfpnet_amd import render as RD
    lut = RD.colormap_table("magma_r")
    pred, gt = R.exact_inputs("same_24x40_direct")
    d = R.render_depth(pred[0], None, 24, 40, 0, R.DEPTH, *R.EXACT_RANGE, lut)
    flat_p, flat_d = pred[0].reshape(-1), d.reshape(-1, 3)
    assert (flat_d[np.isnan(flat_p)] == 0).all() and (flat_d[flat_p == np.inf] == lut[255]).all() and (flat_d[flat_p == -np.inf] == lut[0]).all()
    assert (flat_d[flat_p == 8.0] == lut[255]).all() and (flat_d[flat_p == 0.5] == lut[16]).all()
    g = R.render_depth(None, gt[0], 24, 40, 0, R.GT, *R.EXACT_RANGE, lut)
    invalid = ~((gt[0] > np.float32(R.LO)) & (gt[0] < np.float32(R.HI)))
    assert invalid.sum() == 5 and (g[invalid] == 255).all()
    u = R.render_u16(pred[0], None, 24, 40, 0, R.DEPTH, 1000.0).reshape(-1)
    assert u[np.isnan(flat_p)].tolist() == [0] and u[flat_p == np.inf].tolist() == [10000] and u[flat_p == -np.inf].tolist() == [1]
    assert (R.render_u16(None, gt[0], 24, 40, 0, R.GT, 1000.0)[invalid] == 0).all()
    # on this tier the accepted interval of a GT picture is a single entry everywhere; zones: first zone wins, border, grey, untouched
    n_lo, n_hi, _ = R.accepted(None, gt[0], 24, 40, 0, R.GT, lambda v: R.lut_index(v, *R.EXACT_RANGE))
    assert np.array_equal(n_lo, n_hi)
    hist, mask = R.zone_inputs(16)
    rect = R.zone_rects("overhang", 30, 45, 16)
    base = np.full((30, 45, 3), 200, np.uint8)
    z_of = R.zone_of(rect, 30, 45)
    assert z_of[0, 0] == 0 and z_of.max() == 15 and (z_of >= 0).all()
    over = R.render_zones(base, hist[0], rect, mask[0], *R.EXACT_RANGE, lut, 256)
    assert np.array_equal(R.render_zones(base, hist[0], rect, mask[0], *R.EXACT_RANGE, lut, 0), base)
    dropped = int(np.flatnonzero(~mask[0])[0])
    inner = (z_of == dropped)
    assert ((over[inner] == 128).all(-1) | (over[inner] == 0).all(-1)).all() and (over[inner] == 128).any() and (over[inner] == 0).any()
    rect_c = R.zone_rects("centered", 30, 45, 16)
    over_c = R.render_zones(base, hist[0], rect_c, mask[0], *R.EXACT_RANGE, lut, 160)
    outside = R.zone_of(rect_c, 30, 45) < 0
    assert outside.any() and (over_c[outside] == 200).all() and (over_c[~outside] != 200).any()


# ---- the caps on the share of pixels whose accepted interval crosses a boundary ----------------------------------------------------------------

@pytest.mark.parametrize("name", ["odd_19x27_to_37x53", "full_240x320_to_480x640"])
def test_few_pixels_cross_a_boundary(name):
    """The realistic tier accepts two adjacent table entries (counts) where the interval |dd| <= RTOL * max(|d|, 1e-3) crosses a
    boundary, and plain equality elsewhere.  That only means something while few pixels cross one: colour <= 2 %, absolute error over
    [0, 1] <= 5 % of the valid pixels, 16-bit millimetres <= 15 %; and no interval spans more than two entries."""
    h, w, H, W, interp = R.shape(name)
    pred, gt = R.realistic_inputs(name)
    for vmin, vmax in R.COLOUR_RANGES:
        share, gap = R.crossing_share(pred[0], None, H, W, interp, R.DEPTH, lambda v: R.lut_index(v, vmin, vmax))
        print(f"{name}: colour over ({vmin}, {vmax}): {100 * share:.2f} % cross a boundary, largest gap {gap}")
        assert share <= 0.02 and gap <= 1
    share, gap = R.crossing_share(pred[0], gt[0], H, W, interp, R.ABS_ERR, lambda v: R.lut_index(v, 0.0, 1.0))
    print(f"{name}: absolute error over (0, 1): {100 * share:.2f} % of the valid pixels cross a boundary, largest gap {gap}")
    assert share <= 0.05 and gap <= 1
    share, gap = R.crossing_share(pred[0], None, H, W, interp, R.DEPTH, lambda v: R.u16_count(v, 1000.0))
    print(f"{name}: 16-bit millimetres: {100 * share:.2f} % cross a boundary, largest gap {gap}")
    assert share <= 0.15 and gap <= 1
    share, gap = R.crossing_share(None, gt[0], H, W, interp, R.GT, lambda v: R.u16_count(v, 1000.0))
    assert share == 0.0 and gap == 0                                            # nothing of the ground truth is uncertain


# ---- the PNG writer ------------------------------------------------------------------------------------------------------------------------

def test_write_png_round_trip(tmp_path):
    import torch
    from PIL import Image
    from cfpnet_amd import render as RD
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (13, 17, 3), dtype=np.uint8)
    f = str(tmp_path / "a.png")
    RD.write_png(f, rgb)
    with Image.open(f) as im:
        assert im.mode == "RGB" and im.size == (17, 13) and np.array_equal(np.asarray(im), rgb)
    RD.write_png(f, torch.from_numpy(rgb))
    with Image.open(f) as im:
        assert np.array_equal(np.asarray(im), rgb)
    mm = rng.integers(0, 65536, (13, 17), dtype=np.uint16)
    mm[0, :3] = (0, 65535, 256)
    RD.write_png(f, mm)
    with Image.open(f) as im:
        assert im.mode in ("I;16", "I;16B", "I") and im.size == (17, 13)
        assert np.array_equal(np.asarray(im).astype(np.uint16), mm)
    for bad in (np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4), np.int32), np.zeros((4, 4, 3), np.uint16)):
        with pytest.raises(ValueError):
            RD.write_png(f, bad)
