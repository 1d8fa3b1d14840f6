"""The positional tables: `cfp_add_rowtable` (out = x + table[oy:oy+H, ox:ox+W]) and `cfp_rowtable_grad` (dtable[window] = beta * old +
sum over B of dx), with host offsets and with the `_dev` forms that read an int32[2] offset from device memory and clamp it to
[0, Ht - H] x [0, Wt - W] -- the forms the captured training step replays with a new random window every step.  References are plain
numpy in float64 on inputs quantised to the storage type.

Bounds: `add` stores in the activation type, so the suite's `close()` / `tol(dtype)` (test_ops_gpu.py); `grad` sums exactly representable
inputs into a FLOAT32 table whatever the activation type, so `OUT_TOL[float32]` (test_train_kernels_gpu.py) times the largest expected
entry for all three types (a float32 sum of up to 576 terms in lane order: its worst-case rounding, 50 x 2^-24 x sum|v|, is below that).
Device offsets against host offsets, and everything outside a window, are compared bit for bit.
Every test prints its worst error as a share of its bound (`pytest -s`)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cfpnet_amd import hip, ops, train_ops  # noqa: E402
from test_ops_gpu import DEV, DTYPES, close, q, rnd, tol  # noqa: E402
from test_train_kernels_gpu import OUT_TOL  # noqa: E402

SENTINEL = -77.0
PAD, C0 = 16, 8             # pitched views: ld = C + PAD, the view starts at column C0
CFP_ESHAPE = -2

# (B, H, W, C, Ht, Wt), then the `ibits` rowtable_grad_impl picks (2^ibits items per workgroup, 256 >> ibits batch lanes; the same for
# 4- and 8-wide vectors at these sizes) -- derived from the host loop restated in host_ibits() and asserted below
SHAPES = [
    ((1, 5, 7, 8, 9, 12), 8),           # 1 lane: one image, one ragged workgroup
    ((3, 15, 20, 136, 30, 40), 7),      # 2 lanes, B odd: lane 0 adds two images, lane 1 one
    ((40, 3, 5, 16, 6, 9), 3),          # 32 lanes, B not a multiple: lanes 0-7 add two images, the others one
    ((576, 1, 16, 32, 1, 16), 3),       # 32 lanes x 18 images: the [16, D] second table of a fusion block against B * Z "images"
    ((2, 13, 17, 24, 13, 17), 7),       # 2 lanes; the window is the whole table; 1326 / 663 items are no multiple of 128
    ((9, 3, 5, 16, 6, 9), 5),           # 8 lanes, B = 9: lane 0 adds two images
]
SHAPE_IDS = ["x".join(map(str, s)) for s, _ in SHAPES]


def host_ibits(B, H, W, C, ve):
    """The loop of rowtable_grad_impl (csrc/train_misc.hip)."""
    total, ibits = H * W * (C // ve), 8
    while ibits > 3 and (total >> ibits) < 512 and (256 >> (ibits - 1)) <= B:
        ibits -= 1
    return ibits


def test_the_shapes_reach_the_lane_counts_their_comments_state():
    lanes = set()
    for (B, H, W, C, Ht, Wt), want in SHAPES:
        for ve in (4, 8):
            assert host_ibits(B, H, W, C, ve) == want, (B, H, W, C, ve)
        lanes.add(256 >> want)
    assert len(lanes) >= 3 and 32 in lanes and 1 in lanes, lanes


def offsets(H, W, Ht, Wt):
    """The two corners and one interior point (fewer where they coincide)."""
    return sorted({(0, 0), (Ht - H, Wt - W), ((Ht - H) // 2, (Wt - W + 1) // 2)})


def pitched(x2d, dtype):
    """[rows, C] -> (view [rows, C] of a zeroed [rows, C + PAD] device buffer at column C0, holding x2d in `dtype`)."""
    buf = torch.zeros(x2d.shape[0], x2d.shape[1] + PAD, dtype=dtype, device=DEV)
    buf[:, C0:C0 + x2d.shape[1]] = x2d.to(dtype).to(DEV)
    return buf[:, C0:C0 + x2d.shape[1]], buf


def guarded_out(rows, C, dtype):
    """Output view at column C0 of a sentinel-filled [rows + 1, C + PAD] buffer: guard columns and one spare row."""
    buf = torch.full((rows + 1, C + PAD), SENTINEL, dtype=dtype, device=DEV)
    return ops.Act(buf, C0, C), buf


def guards_intact(buf, rows, C):
    b = buf.float().cpu()
    return bool((b[:rows, :C0] == SENTINEL).all() and (b[:rows, C0 + C:] == SENTINEL).all() and (b[rows:] == SENTINEL).all())


def _data(shape, dtype):
    B, H, W, C, Ht, Wt = shape
    x = q(rnd(B * H * W, C, seed=1), dtype)
    table = rnd(Ht * Wt, C, seed=2)
    return x, table


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,ibits", SHAPES, ids=SHAPE_IDS)
def test_add_rowtable_host_offsets(shape, ibits, dtype):
    """Catches: the window origin added to the wrong axis or scaled by W instead of Wt (Ht != Wt, H != W, interior offset with
    oy != ox), the image index not removed from the row (B > 1: image 1 would read past the window), the fast division of the element
    index by C / ve (1, 2, 3, 4, 6, 17 and 34 here), a skipped ragged last workgroup, the input's or the output's pitch ignored, and a
    store outside the output view."""
    B, H, W, C, Ht, Wt = shape
    rows = B * H * W
    x, table = _data(shape, dtype)
    xv, xbuf = pitched(x, dtype)
    tab = table.to(DEV)
    for oy, ox in offsets(H, W, Ht, Wt):
        out, buf = guarded_out(rows, C, dtype)
        ops.add_rowtable(ops.Act(xbuf, C0, C), tab, out, rows, H, W, Wt, oy, ox)
        torch.cuda.synchronize()
        assert guards_intact(buf, rows, C), (oy, ox)
        ref = x.double().reshape(B, H, W, C) + table.double().reshape(Ht, Wt, C)[oy:oy + H, ox:ox + W]
        got = buf[:rows, C0:C0 + C].float().cpu().double().reshape(B, H, W, C)
        err = (got - ref).abs()
        rt, at = tol(dtype)
        print(f"  add_rowtable {shape} ({oy},{ox}) {dtype}: worst err {float(err.max()):.3e} = "
              f"{float((err / (at * ref.abs().max() + rt * ref.abs())).max()):.3f} of the bound")
        close(got, ref, dtype, f"add_rowtable {shape} at ({oy}, {ox})")


def _grad_ref(dx, old, shape, oy, ox, beta):
    B, H, W, C, Ht, Wt = shape
    ref = old.double().reshape(Ht, Wt, C).clone()
    ref[oy:oy + H, ox:ox + W] = beta * ref[oy:oy + H, ox:ox + W] + dx.double().reshape(B, H, W, C).sum(0)
    return ref


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,ibits", SHAPES, ids=SHAPE_IDS)
def test_rowtable_grad_host_offsets_and_beta(shape, ibits, dtype):
    """dtable pre-filled with random values; beta 0 overwrites the window, 1 and 0.5 give beta * old + sum; the rows outside the
    window stay bit-identical.  Catches: `beta` ignored or applied to the sum, beta = 0 computed as 0 * old (a NaN or Inf in an
    uninitialised table would survive: the window holds Inf here), the batch-lane sum stopping one lane early or the lane stride
    dropping images when B is no multiple of the lane count (1, 2, 8 and 32 lanes; B = 3, 9, 40), lanes combined before the barrier,
    a workgroup's idle tail threads writing (ragged item counts), and dx's pitch ignored."""
    B, H, W, C, Ht, Wt = shape
    dx, _ = _data(shape, dtype)
    dxv, _ = pitched(dx, dtype)
    old = rnd(Ht * Wt, C, seed=3)
    for oy, ox in offsets(H, W, Ht, Wt):
        for beta in (0.0, 1.0, 0.5):
            start = old.clone()
            if beta == 0.0:
                start.reshape(Ht, Wt, C)[oy:oy + H, ox:ox + W] = float("inf")
            tab = start.to(DEV)
            out = train_ops.rowtable_grad(dxv, tab, B, H, W, Wt, oy, ox, beta=beta)
            torch.cuda.synchronize()
            assert out is tab
            got = tab.cpu().reshape(Ht, Wt, C)
            ref = _grad_ref(dx, old, shape, oy, ox, beta)          # from `old`: beta = 0 must not read the Inf
            err = float((got.double() - ref).abs().max())
            bound = OUT_TOL[torch.float32] * float(ref[oy:oy + H, ox:ox + W].abs().max())
            print(f"  rowtable_grad {shape} ({oy},{ox}) beta={beta} {dtype}: worst err {err:.3e} = {err / bound:.3f} of the bound")
            assert err <= bound, (shape, oy, ox, beta, err, bound)
            outside = torch.ones(Ht, Wt, dtype=torch.bool)
            outside[oy:oy + H, ox:ox + W] = False
            assert torch.equal(got[outside], start.reshape(Ht, Wt, C)[outside]), "a table row outside the window changed"


def _dev_offsets(H, W, Ht, Wt):
    my, mx = Ht - H, Wt - W
    return [((my + 1) // 2, mx // 2),        # in range
            (-3, -5),                         # both negative
            (my + 2, mx + 7),                 # both beyond the last window
            (-1, mx + 3), (my + 4, -2),       # one coordinate of each kind
            (my // 2, mx + 1), (-7, mx // 3),
            (my, mx), (0, 0)]                 # the limits themselves: not moved


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,ibits", SHAPES, ids=SHAPE_IDS)
def test_device_offsets_equal_the_host_call_at_the_clamped_offset(shape, ibits, dtype):
    """`cfp_add_rowtable_dev` / `cfp_rowtable_grad_dev` with an int32[2] tensor whose CONTENTS change between launches (one
    allocation, as under a replayed graph) against the host-offset call at min(max(off, 0), (Ht - H, Wt - W)), bit for bit, guard
    columns included.  Catches: the clamp applied in the forward only (the gradient would land on other table rows than the forward
    read), clamped to Ht / Wt instead of Ht - H / Wt - W, the two coordinates swapped, a missing lower clamp, and an offset read on the
    host at launch time (the second launch would then repeat the first window)."""
    B, H, W, C, Ht, Wt = shape
    rows = B * H * W
    x, table = _data(shape, dtype)
    xv, xbuf = pitched(x, dtype)
    tab = table.to(DEV)
    old = rnd(Ht * Wt, C, seed=3).to(DEV)
    off = torch.zeros(2, dtype=torch.int32, device=DEV)
    off_ptr, dt = off.data_ptr(), ops.DT[dtype]
    seen = {}
    for oy, ox in _dev_offsets(H, W, Ht, Wt):
        cy, cx = min(max(oy, 0), Ht - H), min(max(ox, 0), Wt - W)
        off.copy_(torch.tensor([oy, ox], dtype=torch.int32))
        assert off.data_ptr() == off_ptr
        out_d, buf_d = guarded_out(rows, C, dtype)
        hip.call("cfp_add_rowtable_dev", xv.data_ptr(), xv.stride(0), tab.data_ptr(), out_d.ptr, out_d.ld, rows, C, H, W, Ht, Wt, off_ptr, dt,
                 hip.current_stream())
        g_d = old.clone()
        hip.call("cfp_rowtable_grad_dev", xv.data_ptr(), xv.stride(0), g_d.data_ptr(), B, H, W, C, Ht, Wt, off_ptr, 0.5, dt, hip.current_stream())
        out_h, buf_h = guarded_out(rows, C, dtype)
        ops.add_rowtable(ops.Act(xbuf, C0, C), tab, out_h, rows, H, W, Wt, cy, cx)
        g_h = train_ops.rowtable_grad(xv, old.clone(), B, H, W, Wt, cy, cx, beta=0.5)
        torch.cuda.synchronize()
        assert torch.equal(buf_d, buf_h), f"add: device offset ({oy}, {ox}) is not the host call at ({cy}, {cx})"
        assert torch.equal(g_d, g_h), f"grad: device offset ({oy}, {ox}) is not the host call at ({cy}, {cx})"
        seen.setdefault((cy, cx), (buf_d, g_d))
    if len(seen) > 1:          # the launches did follow the tensor: different windows gave different results
        (a, ga), (b, gb) = list(seen.values())[:2]
        assert not torch.equal(a, b) and not torch.equal(ga, gb)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rowtable_shape_errors_are_refused_before_any_launch(dtype):
    """A `_dev` call with Ht < H and a host call with Wt < ox + W return CFP_ESHAPE and leave their outputs untouched (either would
    index past the table: the device clamp min(max(off, 0), Ht - H) turns negative)."""
    B, H, W, C, Ht, Wt = 2, 5, 7, 8, 9, 12
    rows = B * H * W
    lib, dt, s = hip.load(), ops.DT[dtype], hip.current_stream()
    xv, _ = pitched(q(rnd(rows, C, seed=1), dtype), dtype)
    tab = rnd(Ht * Wt, C, seed=2).to(DEV)
    off = torch.zeros(2, dtype=torch.int32, device=DEV)
    out, buf = guarded_out(rows, C, dtype)
    dtab = torch.full((Ht * Wt, C), SENTINEL, device=DEV)
    assert lib.cfp_add_rowtable_dev(xv.data_ptr(), xv.stride(0), tab.data_ptr(), out.ptr, out.ld, rows, C, H, W, H - 1, Wt, off.data_ptr(), dt, s) == CFP_ESHAPE
    assert lib.cfp_rowtable_grad_dev(xv.data_ptr(), xv.stride(0), dtab.data_ptr(), B, H, W, C, H - 1, Wt, off.data_ptr(), 0.0, dt, s) == CFP_ESHAPE
    assert lib.cfp_add_rowtable(xv.data_ptr(), xv.stride(0), tab.data_ptr(), out.ptr, out.ld, rows, C, H, W, Wt, 0, Wt - W + 1, dt, s) == CFP_ESHAPE
    assert lib.cfp_rowtable_grad(xv.data_ptr(), xv.stride(0), dtab.data_ptr(), B, H, W, C, Wt, 0, Wt - W + 1, 0.0, dt, s) == CFP_ESHAPE
    assert "bad shape" in hip.last_error()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()) and bool((dtab == SENTINEL).all())
    # the same calls with the limits themselves are taken
    hip.call("cfp_add_rowtable_dev", xv.data_ptr(), xv.stride(0), tab.data_ptr(), out.ptr, out.ld, rows, C, H, W, H, Wt, off.data_ptr(), dt, s)
    hip.call("cfp_rowtable_grad", xv.data_ptr(), xv.stride(0), dtab.data_ptr(), B, H, W, C, Wt, 0, Wt - W, 0.0, dt, s)
    torch.cuda.synchronize()
    assert guards_intact(buf, rows, C) and not bool((buf[:rows, C0:C0 + C] == SENTINEL).any())
