"""numpy float64 restatement of the definition of `cfp_resize_bilinear` and of the transpose `cfp_resize_bilinear_bwd` computes
(include/cfpnet_hip.h, csrc/misc_ops.hip) -- TEST INFRASTRUCTURE.

The definition, in the kernel header's words: the source rectangle is cut from the ZERO-EXTENDED source map; taps whose zone
(`ry // p1`, `rx // p2` in rectangle coordinates, clamped to the zn x zn grid) is flagged invalid are zeroed; the rectangle is blended
to dh x dw with align-corners bilinear weights (source coordinate = (n_src - 1) / (n_dst - 1) * destination index, 0 when n_dst == 1);
the blend is written, or added, onto the part of the destination rectangle that lies inside the destination map; every other element of
the destination keeps what it held.  `resize_ref` is checked against torch in test_resample_ref.py (CPU); the GPU tests compare the
kernels with it.  Also the size pairs and rectangles every bilinear test shares, kept here once."""
import numpy as np

# (Hs, Ws) -> (Hd, Wd): every relation between a source and a destination size the kernels meet or could meet
SIZE_PAIRS = [
    ("identity", (7, 9), (7, 9)),
    ("exact_2x", (5, 7), (10, 14)),
    ("non_integer_up", (13, 17), (30, 40)),
    ("zone_pair_up", (28, 28), (32, 32)),
    ("zone_pair_down", (32, 32), (28, 28)),
    ("strong_down", (33, 41), (5, 6)),               # scale > 1: the two taps skip source rows
    ("one_pixel_source", (1, 1), (6, 5)),
    ("one_row_source", (1, 5), (4, 13)),
    ("one_pixel_destination", (6, 5), (1, 1)),       # scale == 0 by the n_dst == 1 rule
    ("one_row_destination", (9, 4), (1, 7)),
    ("two_pixels_stretched", (2, 2), (31, 37)),
    ("one_axis_changes", (7, 9), (7, 20)),
]
PAIR_IDS = [p[0] for p in SIZE_PAIRS]

# the rectangle tests: a 9 x 11 map against a zn x zn zone grid of p1 x p2 pixels per zone (grid extent 6 x 8)
MAP_H, MAP_W = 9, 11
ZN, P1, P2 = 2, 3, 4
GRID_H, GRID_W = ZN * P1, ZN * P2
RECTS = [                                            # (y0, x0, h, w) on the map
    ("interior_1to1", (1, 2, 6, 8)),
    ("interior_resampled", (2, 1, 5, 7)),
    ("overhang_top_left", (-2, -3, 6, 8)),
    ("overhang_bottom_right", (5, 6, 6, 8)),
    ("overhang_all_sides", (-1, -1, 11, 13)),
    ("outside_below", (9, 0, 4, 4)),
    ("outside_left", (0, -8, 5, 8)),
    ("one_pixel_inside", (4, 5, 1, 1)),
    ("one_pixel_corner", (8, 10, 1, 1)),
]
RECT_IDS = [r[0] for r in RECTS]
RECTS_OUTSIDE = ("outside_below", "outside_left")


def axis_taps(n_src, n_dst):
    """Align-corners bilinear along one axis -> (i0 [n_dst], i1 [n_dst], l1 [n_dst]): out[d] = (1 - l1) * in[i0] + l1 * in[i1]."""
    scale = (n_src - 1) / (n_dst - 1) if n_dst > 1 else 0.0
    f = scale * np.arange(n_dst, dtype=np.float64)
    i0 = np.minimum(np.floor(f).astype(np.int64), n_src - 1)
    i1 = np.minimum(i0 + 1, n_src - 1)
    return i0, i1, f - i0


def axis_matrix(n_src, n_dst):
    """The same blend as a dense [n_dst, n_src] matrix (rows sum to 1)."""
    i0, i1, l1 = axis_taps(n_src, n_dst)
    a = np.zeros((n_dst, n_src), np.float64)
    d = np.arange(n_dst)
    np.add.at(a, (d, i0), 1.0 - l1)
    np.add.at(a, (d, i1), l1)
    return a


def resize_ref(x, srect, dst_init, drect, zone_valid=None, zn=0, p1=0, p2=0, accumulate=False):
    """x [B,C,Hs,Ws], srect (sy0, sx0, sh, sw), dst_init [B,C,Hd,Wd], drect (dy0, dx0, dh, dw), zone_valid [B, zn*zn] (0 = invalid) or
    None -> the destination [B,C,Hd,Wd] after the call, float64.  Neither input is modified."""
    x = np.asarray(x, np.float64)
    out = np.array(dst_init, np.float64, copy=True)
    B, C, Hs, Ws = x.shape
    Hd, Wd = out.shape[2:]
    sy0, sx0, sh, sw = srect
    dy0, dx0, dh, dw = drect
    assert out.shape[:2] == (B, C) and min(sh, sw, dh, dw) > 0
    # the source rectangle, cut from the zero-extended map
    gy, gx = sy0 + np.arange(sh), sx0 + np.arange(sw)
    ky, kx = (gy >= 0) & (gy < Hs), (gx >= 0) & (gx < Ws)
    rect = np.zeros((B, C, sh, sw), np.float64)
    rect[:, :, np.where(ky)[0][:, None], np.where(kx)[0][None, :]] = x[:, :, gy[ky][:, None], gx[kx][None, :]]
    if zone_valid is not None:
        zv = np.asarray(zone_valid).reshape(B, zn, zn) != 0
        zy = np.clip(np.arange(sh) // p1, 0, zn - 1)
        zx = np.clip(np.arange(sw) // p2, 0, zn - 1)
        rect = rect * zv[:, zy[:, None], zx[None, :]][:, None]
    y0, y1, ly = axis_taps(sh, dh)
    x0, x1, lx = axis_taps(sw, dw)
    top = rect[:, :, y0][:, :, :, x0] * (1.0 - lx) + rect[:, :, y0][:, :, :, x1] * lx
    bot = rect[:, :, y1][:, :, :, x0] * (1.0 - lx) + rect[:, :, y1][:, :, :, x1] * lx
    blend = top * (1.0 - ly)[:, None] + bot * ly[:, None]
    # the part of the destination rectangle inside the destination map
    oy, ox = dy0 + np.arange(dh), dx0 + np.arange(dw)
    iy, ix = (oy >= 0) & (oy < Hd), (ox >= 0) & (ox < Wd)
    if iy.any() and ix.any():
        ys, xs = oy[iy][:, None], ox[ix][None, :]
        part = blend[:, :, np.where(iy)[0][:, None], np.where(ix)[0][None, :]]
        out[:, :, ys, xs] = out[:, :, ys, xs] + part if accumulate else part
    return out


def resize_whole_ref(x, Hd, Wd):
    """Whole map -> whole map."""
    B, C, Hs, Ws = x.shape
    return resize_ref(x, (0, 0, Hs, Ws), np.zeros((B, C, Hd, Wd)), (0, 0, Hd, Wd))


def resize_adjoint_ref(dy, Hs, Ws):
    """dy [B,C,Hd,Wd] -> [B,C,Hs,Ws]: the exact transpose of the whole-map resize Hs x Ws -> Hd x Wd (resize = Ay . x . Ax^T)."""
    dy = np.asarray(dy, np.float64)
    Hd, Wd = dy.shape[2:]
    ay, ax = axis_matrix(Hs, Hd), axis_matrix(Ws, Wd)
    return np.einsum("ds,bcde,et->bcst", ay, dy, ax)


def zone_patterns(B=3):
    """zone_valid [B, ZN*ZN] uint8 patterns for the paste tests: `mixed` has every one of the four zones invalid in at least one image
    and valid in at least one; `all` / `none` are the two uniform images."""
    mixed = np.array([[0, 1, 1, 0], [1, 0, 1, 1], [1, 1, 0, 1]], np.uint8)[:B]
    assert B < 3 or ((mixed == 0).any(0).all() and (mixed != 0).any(0).all())
    return {"mixed": mixed, "all": np.ones((B, ZN * ZN), np.uint8), "none": np.zeros((B, ZN * ZN), np.uint8)}
