"""`cfp_resize_bilinear` and `cfp_resize_bilinear_bwd` on the GPU against the float64 restatement of their definition
(`resample_ref.py`, itself checked against torch in test_resample_ref.py), at every relation between a source and a destination size:
unchanged, exact and non-integer up, down, scale > 1, one-pixel / one-row sources and destinations (scale == 0), one axis only; rectangles
inside the map, hanging over every side and wholly outside it; zone flags on a NON-SQUARE zone grid; `accumulate` in every storage type.

Bounds, none of them measured on the kernels:
  forward    the suite's own `close()` / `tol(dtype)` (test_ops_gpu.py) against float64 on inputs quantised to the storage type.  The
             float32 case needs no comparative form: an emulation of the kernel's float32 source coordinates in numpy stays below 13 %
             of `tol(float32)` at every size pair (worst: 32 -> 28, 7.7e-6 on N(0,1) data), and so did the kernel when measured.
  16-bit +=  one rounding step of the storage type at the expected value (load, add in float32, round once).
  backward   `OUT_TOL[dtype]` (test_train_kernels_gpu.py) times the largest expected gradient, against the float64 transpose.
Every test prints its worst error as a share of its bound (`pytest -s`)."""
import functools

import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu

from cfpnet_amd import ops, train_ops  # noqa: E402
from test_ops_gpu import DEV, DTYPES, HALF, close, from_nhwc, nhwc, q, rnd, to_act, tol  # noqa: E402
from test_train_kernels_gpu import OUT_TOL  # noqa: E402

SENTINEL = -77.0            # exactly representable in all three storage types
PAD, C0 = 16, 8             # the pitched views: ld = C + PAD, the view starts at column C0 (16-byte aligned in every type)
WHOLE_GRID = (0, 0, R.GRID_H, R.GRID_W)


def guarded_dst(B, H, W, C, dtype, init=None):
    """A [B*H*W, C] destination view at column C0 of a sentinel-filled [B*H*W + 1, C + PAD] buffer (one spare row behind the view);
    the view itself holds `init` [B,C,H,W], or the sentinel too (a pixel the kernel skips then shows)."""
    rows = B * H * W
    buf = torch.full((rows + 1, C + PAD), SENTINEL, dtype=dtype, device=DEV)
    if init is not None:
        buf[:rows, C0:C0 + C] = nhwc(init).to(dtype).to(DEV)
    return ops.Act(buf, C0, C), buf


def read_dst(buf, B, H, W, C):
    """-> (the view as [B,C,H,W] float32 on the CPU, True when the columns beside the view and the spare row still hold the sentinel)."""
    rows = B * H * W
    b = buf.float().cpu()
    intact = bool((b[:rows, :C0] == SENTINEL).all() and (b[:rows, C0 + C:] == SENTINEL).all() and (b[rows:] == SENTINEL).all())
    return from_nhwc(b[:rows, C0:C0 + C], B, H, W), intact


def pitched_src(x, dtype):
    """[B,C,H,W] -> Act view with ld = C + PAD at column C0; the columns around it hold zeros."""
    return to_act(nhwc(x), dtype, ld=x.shape[1] + PAD, c0=C0)


def check_close(got, ref, dtype, what):
    ref = torch.as_tensor(ref)
    rt, at = tol(dtype)
    bound = at * ref.abs().max().clamp(min=1e-3) + rt * ref.abs()
    err = (got.double() - ref).abs()
    print(f"  {what}: worst err {float(err.max()):.3e} = {float((err / bound).max()):.3f} of the bound")
    close(got.double(), ref, dtype, what)


def storage_step(v, dtype):
    """Spacing of the storage type's values at |v| (float64 tensor): 2^(exponent - mantissa bits), the subnormal spacing below."""
    mant, emin = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}[dtype]
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** emin))).clamp(min=emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


# ---- whole maps ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,src,dst", R.SIZE_PAIRS, ids=R.PAIR_IDS)
def test_whole_map_resize_at_every_size_relation(name, src, dst, dtype):
    """Catches: `y1` / `x1` not clamped at the last row (one_pixel_source, identity: the +1 tap reads the next image or row), a missing
    `n_dst == 1 -> scale 0` rule (one_pixel_destination divides by zero), an integer-ratio shortcut (non_integer_up, strong_down),
    swapped axes (every pair is non-square), a wrong fast division of the element index (C / ve = 1, 2, 3 and 6: a divisor of 1, even,
    odd), the pitch of either side ignored, and a store outside the view (sentinel columns and spare row)."""
    (Hs, Ws), (Hd, Wd), B = src, dst, 2
    for C in (8, 24):
        x = q(rnd(B, C, Hs, Ws, seed=1), dtype)
        d, buf = guarded_dst(B, Hd, Wd, C, dtype)
        ops.resize_bilinear(pitched_src(x, dtype), Hs, Ws, (0, 0, Hs, Ws), d, Hd, Wd, (0, 0, Hd, Wd), B)
        torch.cuda.synchronize()
        got, intact = read_dst(buf, B, Hd, Wd, C)
        assert intact, f"{name} C={C}: the kernel wrote outside the destination view"
        check_close(got, R.resize_whole_ref(x.numpy(), Hd, Wd), dtype, f"resize {name} C={C} {dtype}")
        if name == "identity":
            assert torch.equal(got, x), "an unchanged size must copy the map exactly (every weight is 1 or 0)"


# ---- rectangles and zone flags ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _rect_inputs(dtype, B, C=8):
    """(map [B,C,9,11], grid [B,C,6,8]) quantised to `dtype`, shared by the rectangle tests and never modified."""
    return q(rnd(B, C, R.MAP_H, R.MAP_W, seed=11), dtype), q(rnd(B, C, R.GRID_H, R.GRID_W, seed=12), dtype)


def _inside_mask(rect):
    y0, x0, h, w = rect
    m = np.zeros((R.MAP_H, R.MAP_W), bool)
    m[max(y0, 0):max(min(y0 + h, R.MAP_H), 0), max(x0, 0):max(min(x0 + w, R.MAP_W), 0)] = True
    return torch.from_numpy(m)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,rect", R.RECTS, ids=R.RECT_IDS)
def test_crop_a_rectangle_of_the_map_onto_the_grid(name, rect, dtype):
    """Rectangle of the 9 x 11 map -> the whole 6 x 8 grid.  Catches: the zero extension applied on one side only (overhang bottom /
    right / all sides: a clamped address used as a value), the rectangle origin added to the wrong axis (non-square map and grid), a
    one-pixel rectangle dividing by `sh - 1 == 0`, and an out-of-map rectangle that reads the clamped border instead of zeros."""
    B, C = 2, 8
    x, _ = _rect_inputs(dtype, B)
    d, buf = guarded_dst(B, R.GRID_H, R.GRID_W, C, dtype)
    ops.resize_bilinear(pitched_src(x, dtype), R.MAP_H, R.MAP_W, rect, d, R.GRID_H, R.GRID_W, WHOLE_GRID, B)
    torch.cuda.synchronize()
    got, intact = read_dst(buf, B, R.GRID_H, R.GRID_W, C)
    assert intact
    ref = R.resize_ref(x.numpy(), rect, np.zeros((B, C, R.GRID_H, R.GRID_W)), WHOLE_GRID)
    check_close(got, ref, dtype, f"crop {name} {dtype}")
    if name in R.RECTS_OUTSIDE:
        assert not ref.any() and not bool(got.any()), "a crop wholly outside the map is all zeros"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,rect", R.RECTS, ids=R.RECT_IDS)
def test_paste_the_grid_onto_a_rectangle_of_the_map_with_zone_flags(name, rect, dtype):
    """The whole 6 x 8 grid -> a rectangle of the 9 x 11 map, written and accumulated, without flags and with three flag patterns on the
    2 x 2 grid of 3 x 4-pixel zones (flags are indexed by the SOURCE coordinates, here the grid's).  Catches: `p1` used for both axes or
    the zone index computed as `zy * zn + zx` with the axes swapped (p1 != p2, and `mixed` is not symmetric), flags of image 0 used for
    every image, the in-map test done on the rectangle instead of the map (overhangs: a store outside the map lands in a neighbouring
    row or image and breaks the bit-identity of the pixels outside the rectangle), `accumulate` ignored or applied twice, and a
    wholly-outside paste that writes anything at all."""
    B, C = 3, 8
    y0, x0, h, w = rect
    init, z = _rect_inputs(dtype, B)
    inside = _inside_mask(rect)
    for zones, valid in [(None, None)] + sorted(R.zone_patterns(B).items()):
        zv = None if valid is None else torch.from_numpy(valid).to(DEV)
        for accumulate in (False, True):
            what = f"paste {name} zones={zones} accumulate={accumulate} {dtype}"
            d, buf = guarded_dst(B, R.MAP_H, R.MAP_W, C, dtype, init=init)
            ops.resize_bilinear(pitched_src(z, dtype), R.GRID_H, R.GRID_W, WHOLE_GRID, d, R.MAP_H, R.MAP_W, rect, B,
                                zone_valid=zv, zn=R.ZN, p1=R.P1, p2=R.P2, accumulate=accumulate)
            torch.cuda.synchronize()
            got, intact = read_dst(buf, B, R.MAP_H, R.MAP_W, C)
            assert intact, what
            ref = R.resize_ref(z.numpy(), WHOLE_GRID, init.numpy(), rect, valid, R.ZN, R.P1, R.P2, accumulate)
            check_close(got, ref, dtype, what)
            assert torch.equal(got[:, :, ~inside], init[:, :, ~inside]), what + ": a pixel outside the rectangle changed"
            if name in R.RECTS_OUTSIDE:
                assert not bool(inside.any()) and torch.equal(got, init), what
            if zones == "none":
                want = init[:, :, inside] if accumulate else torch.zeros_like(init[:, :, inside])
                assert torch.equal(got[:, :, inside], want), what + ": no valid zone"


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("name,rect", [r for r in R.RECTS if r[0] not in R.RECTS_OUTSIDE], ids=[i for i in R.RECT_IDS if i not in R.RECTS_OUTSIDE])
def test_accumulate_in_16_bit_storage_rounds_once(name, rect, dtype):
    """The kernel loads the stored destination, adds the blend in float32 and rounds ONCE: the result is within one rounding step of
    the storage type of round(q(dst) + blend).  Catches: the blend rounded to the storage type before the add (two roundings: up to
    1.5 steps, and a systematic half step on many elements), the add done in the storage type, and the destination read after a
    partial store.  Both inputs are positive here, so that no element is a near-cancellation: the float32 error of the blend (1e-6)
    would exceed a storage step of a result below 3e-4, and the bound would then test float32, not the rounding."""
    B, C = 3, 8
    init, z = _rect_inputs(dtype, B)
    init, z = q(init.abs() + 0.5, dtype), q(z.abs() + 0.5, dtype)
    valid = R.zone_patterns(B)["mixed"]
    d, buf = guarded_dst(B, R.MAP_H, R.MAP_W, C, dtype, init=init)
    ops.resize_bilinear(pitched_src(z, dtype), R.GRID_H, R.GRID_W, WHOLE_GRID, d, R.MAP_H, R.MAP_W, rect, B,
                        zone_valid=torch.from_numpy(valid).to(DEV), zn=R.ZN, p1=R.P1, p2=R.P2, accumulate=True)
    torch.cuda.synchronize()
    got, intact = read_dst(buf, B, R.MAP_H, R.MAP_W, C)
    assert intact
    exact = torch.from_numpy(R.resize_ref(z.numpy(), WHOLE_GRID, init.numpy(), rect, valid, R.ZN, R.P1, R.P2, True))
    ref = exact.to(dtype).double()
    err, step = (got.double() - ref).abs(), storage_step(ref, dtype)
    print(f"  16-bit accumulate {name} {dtype}: worst err {float((err / step).max()):.2f} steps, {int((err > 0).sum())} of {err.numel()} elements differ")
    assert bool((err <= step).all()), f"{name}: {float((err / step).max()):.2f} rounding steps"


# ---- backward ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,src,dst", R.SIZE_PAIRS, ids=R.PAIR_IDS)
def test_resize_backward_is_the_transpose_at_every_size_relation(name, src, dst, dtype):
    """`cfp_resize_bilinear_bwd` (a gather over a window of destination rows and columns computed from 1 / scale) against the float64
    transpose, written and accumulated.  Catches: a window one row or column too narrow (the `- 1` / `+ 1` margins dropped: a source
    pixel loses its farthest contributor -- zone_pair_down and strong_down have the widest windows, two_pixels_stretched the longest),
    the `scale == 0` window (one_pixel_source gathers EVERY destination pixel, one_pixel_destination leaves all but row 0 at zero), both
    taps on the last row counted once instead of twice (identity, one_row_source), and `accumulate` ignored."""
    (Hs, Ws), (Hd, Wd), B, C = src, dst, 2, 8
    dy = q(rnd(B, C, Hd, Wd, seed=2), dtype)
    prev = q(rnd(B, C, Hs, Ws, seed=3), dtype)
    want = torch.from_numpy(R.resize_adjoint_ref(dy.numpy(), Hs, Ws))
    dyd = torch.zeros(B * Hd * Wd, C + PAD, dtype=dtype, device=DEV)
    dyd[:, C0:C0 + C] = nhwc(dy).to(dtype).to(DEV)
    scale = float(want.abs().max())
    for accumulate in (False, True):
        buf = torch.full((B * Hs * Ws + 1, C + PAD), SENTINEL, dtype=dtype, device=DEV)
        view = buf[:B * Hs * Ws, C0:C0 + C]
        if accumulate:
            view.copy_(nhwc(prev).to(dtype).to(DEV))
        out = train_ops.resize_bilinear_bwd(dyd[:, C0:C0 + C], B, Hs, Ws, Hd, Wd, dx=view, accumulate=accumulate)
        torch.cuda.synchronize()
        assert out is view
        got, intact = read_dst(buf, B, Hs, Ws, C)
        assert intact
        ref = want + prev.double() if accumulate else want
        err = float((got.double() - ref).abs().max())
        bound = OUT_TOL[dtype] * (scale + (float(prev.abs().max()) if accumulate else 0.0))
        print(f"  resize_bwd {name} accumulate={accumulate} {dtype}: worst err {err:.3e} = {err / bound:.3f} of the bound")
        assert err <= bound, (name, accumulate, err, bound)
    if name == "one_pixel_destination":
        g = got.double() - prev.double()          # the accumulate run: every source pixel but (0, 0) received nothing
        g[:, :, 0, 0] = 0
        assert float(g.abs().max()) == 0.0


@pytest.mark.parametrize("name,src,dst", R.SIZE_PAIRS, ids=R.PAIR_IDS)
def test_forward_and_backward_kernels_are_adjoint(name, src, dst):
    """<resize(x), dy> == <x, resize_bwd(dy)> between the two HIP kernels in float32, both sides summed in float64 from the kernels'
    outputs.  The two kernels compute indices and weights separately; a disagreement between them (a window that misses a tap the
    forward uses, a weight taken from the other tap) takes about one row's share, 1 / H, off one side.  x and dy are positive, so that
    nothing cancels and that share stands against the whole sum; the bound below is about 2e-4 of it.
    Bound: each forward element is within tol(float32) of exact (<= 4e-5 max|y|), each backward element within OUT_TOL (2e-5 max|dx|),
    so |lhs - rhs| <= 4e-5 max|y| sum|dy| + 2e-5 max|dx| sum|x|."""
    (Hs, Ws), (Hd, Wd), B, C = src, dst, 2, 8
    x, dy = rnd(B, C, Hs, Ws, seed=4).abs(), rnd(B, C, Hd, Wd, seed=5).abs()
    y = ops.new_act(B * Hd * Wd, C, torch.float32, DEV)
    ops.resize_bilinear(to_act(nhwc(x), torch.float32), Hs, Ws, (0, 0, Hs, Ws), y, Hd, Wd, (0, 0, Hd, Wd), B)
    dx = train_ops.resize_bilinear_bwd(nhwc(dy).to(DEV), B, Hs, Ws, Hd, Wd)
    torch.cuda.synchronize()
    yv, dxv = from_nhwc(y.torch(), B, Hd, Wd).double(), from_nhwc(dx, B, Hs, Ws).double()
    lhs, rhs = float((yv * dy.double()).sum()), float((x.double() * dxv).sum())
    rt, at = tol(torch.float32)
    bound = (rt + at) * float(yv.abs().max()) * float(dy.abs().sum()) + OUT_TOL[torch.float32] * float(dxv.abs().max()) * float(x.abs().sum())
    print(f"  adjoint identity {name}: lhs {lhs:.6f} rhs {rhs:.6f} diff {abs(lhs - rhs):.3e} = {abs(lhs - rhs) / bound:.4f} of the bound")
    assert abs(lhs - rhs) <= bound
