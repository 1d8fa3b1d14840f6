"""The float64 restatement of bilinear resampling (`resample_ref.py`) against torch on the CPU: what the GPU tests of
`cfp_resize_bilinear` / `cfp_resize_bilinear_bwd` compare the kernels with is itself checked here, without a GPU.  torch computes the
same float64 expression ((n_src - 1) / (n_dst - 1) * index, two taps per axis), so the two agree to rounding: 1e-12 on O(1) data."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resample_ref as R

TOL = 1e-12


def _rnd(*shape, seed=0):
    return np.random.default_rng(seed).standard_normal(shape)


def _interp(x, size):
    return F.interpolate(x, size=list(size), mode="bilinear", align_corners=True)


@pytest.mark.parametrize("name,src,dst", R.SIZE_PAIRS, ids=R.PAIR_IDS)
def test_whole_map_resize_equals_interpolate(name, src, dst):
    x = _rnd(2, 3, *src, seed=1)
    want = _interp(torch.from_numpy(x), dst).numpy()
    got = R.resize_whole_ref(x, *dst)
    assert got.shape == want.shape and np.abs(got - want).max() <= TOL


@pytest.mark.parametrize("name,src,dst", R.SIZE_PAIRS, ids=R.PAIR_IDS)
def test_adjoint_equals_autograd_and_is_the_transpose(name, src, dst):
    x = torch.from_numpy(_rnd(2, 3, *src, seed=2)).requires_grad_(True)
    dy = _rnd(2, 3, *dst, seed=3)
    _interp(x, dst).backward(torch.from_numpy(dy))
    got = R.resize_adjoint_ref(dy, *src)
    assert got.shape == tuple(x.shape) and np.abs(got - x.grad.numpy()).max() <= TOL * max(1.0, dst[0] * dst[1] / (src[0] * src[1]))
    # <resize(x), dy> == <x, adjoint(dy)>: the tap form and the matrix form of the reference describe one operator
    xn = x.detach().numpy()
    lhs, rhs = float((R.resize_whole_ref(xn, *dst) * dy).sum()), float((xn * got).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, np.abs(dy).sum())


def _zone_mask(valid):
    """[B, ZN*ZN] flags -> [B,1,GRID_H,GRID_W] float64 mask, written with torch ops."""
    B = valid.shape[0]
    v = torch.from_numpy(valid != 0).reshape(B, 1, R.ZN, 1, R.ZN, 1)
    return v.expand(B, 1, R.ZN, R.P1, R.ZN, R.P2).reshape(B, 1, R.GRID_H, R.GRID_W).double()


def _inside(rect, H, W):
    """(rows of the rectangle inside the map, the map rows they are), same for columns, as slices."""
    y0, x0, h, w = rect
    ya, yb, xa, xb = max(y0, 0), min(y0 + h, H), max(x0, 0), min(x0 + w, W)
    if ya >= yb or xa >= xb:
        return None
    return slice(ya - y0, yb - y0), slice(ya, yb), slice(xa - x0, xb - x0), slice(xa, xb)


@pytest.mark.parametrize("name,rect", R.RECTS, ids=R.RECT_IDS)
def test_crop_equals_pad_slice_interpolate(name, rect):
    """Rectangle of the map -> the whole grid."""
    y0, x0, h, w = rect
    x = torch.from_numpy(_rnd(2, 3, R.MAP_H, R.MAP_W, seed=4))
    P = 16                                                       # more than any rectangle overhangs
    crop = F.pad(x, (P, P, P, P))[:, :, P + y0:P + y0 + h, P + x0:P + x0 + w]
    want = _interp(crop, (R.GRID_H, R.GRID_W)).numpy()
    got = R.resize_ref(x.numpy(), rect, _rnd(2, 3, R.GRID_H, R.GRID_W, seed=5), (0, 0, R.GRID_H, R.GRID_W))
    assert np.abs(got - want).max() <= TOL
    if name in R.RECTS_OUTSIDE:
        assert not got.any()


@pytest.mark.parametrize("zones", [None, "mixed", "all", "none"])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("name,rect", R.RECTS, ids=R.RECT_IDS)
def test_paste_equals_mask_interpolate_paste(name, rect, accumulate, zones):
    """The whole grid -> rectangle of the map, zone flags on the grid."""
    y0, x0, h, w = rect
    B = 3
    z = torch.from_numpy(_rnd(B, 3, R.GRID_H, R.GRID_W, seed=6))
    init = _rnd(B, 3, R.MAP_H, R.MAP_W, seed=7)
    valid = None if zones is None else R.zone_patterns(B)[zones]
    back = _interp(z if valid is None else z * _zone_mask(valid), (h, w))
    want = torch.from_numpy(init.copy())
    ins = _inside(rect, R.MAP_H, R.MAP_W)
    if ins is not None:
        ry, my, rx, mx = ins
        want[:, :, my, mx] = (want[:, :, my, mx] if accumulate else 0.0) + back[:, :, ry, rx]
    got = R.resize_ref(z.numpy(), (0, 0, R.GRID_H, R.GRID_W), init, rect, valid, R.ZN, R.P1, R.P2, accumulate)
    assert np.abs(got - want.numpy()).max() <= TOL
    outside = np.ones((R.MAP_H, R.MAP_W), bool)
    if ins is not None:
        outside[ins[1], ins[3]] = False
    assert np.array_equal(got[:, :, outside], init[:, :, outside])          # pixels outside the rectangle: untouched, bit for bit
    if name in R.RECTS_OUTSIDE:
        assert np.array_equal(got, init)
    if zones == "none" and ins is not None:
        assert np.array_equal(got[:, :, ins[1], ins[3]], init[:, :, ins[1], ins[3]] if accumulate else np.zeros_like(got[:, :, ins[1], ins[3]]))


def test_the_shared_lists_are_what_the_gpu_tests_expect():
    assert len(R.SIZE_PAIRS) == 12 and len(R.RECTS) == 9 and (R.GRID_H, R.GRID_W) == (6, 8)
    for _, (y0, x0, h, w) in R.RECTS:
        assert h <= 41 and w <= 41
    # the weights of one axis sum to 1 and never reach outside the source
    for _, (hs, ws), (hd, wd) in R.SIZE_PAIRS:
        for ns, nd in ((hs, hd), (ws, wd)):
            i0, i1, l1 = R.axis_taps(ns, nd)
            assert i0.min() >= 0 and i1.max() <= ns - 1 and l1.min() >= 0.0 and l1.max() <= 1.0
            assert np.abs(R.axis_matrix(ns, nd).sum(1) - 1.0).max() <= 1e-15
