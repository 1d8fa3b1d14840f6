"""`cfp_depth_reproject` / `cfp_depth_fuse` on the GPU against the numpy restatement of their definition (`reproject_ref.py`, itself checked
in test_reproject_abi.py) and the Python API around them (`cfpnet_amd/temporal.py`).

Tolerances, none of them measured on the kernels:
  index    exactly the float64 reference's, and NaN / -1 at exactly its holes, outside the pixels a rounding or a tie in Z' could decide
           either way (`R.reproject_excluded`: GUARD = 4 x the worst distance between the float32 and the float64 projections of these
           inputs, 1e-5 relative in Z'; at most 1 % of a case, asserted on the CPU).
  values   depth, plane, fused depth and variance within the project's own bound (tests/test_metrics.py), |got - want| <= 2e-5 *
           max(|want|, 1e-3), of the float32 restatement at the pixels where both took the same source / the same row of the table.
  counts   exactly the float64 reference's over the pixels farther than 1e-4 relative from the gate; the excluded pixels may go either way.
  stats    within 1e-12 relative of the float64 sums of the float32 terms (the sum of up to 3e5 float64 terms in another order)."""
import numpy as np
import pytest
import torch

import pointcloud_ref as P
import reproject_ref as R

pytestmark = pytest.mark.gpu

from cfpnet_amd import hip, metrics, pointcloud as PC, temporal as TP  # noqa: E402

DEV = "cuda:0"
GUARD_VALUE = -77.0


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)             # a copy: the shared inputs are read-only


def guarded(shape, dtype, pad=64):
    """A tensor of `shape` inside a larger buffer of guard values -> (view, whole buffer, slice)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), GUARD_VALUE, dtype=dtype, device=DEV)
    return buf[pad:pad + n].view(*shape), buf, slice(pad, pad + n)


def guards_intact(buf, sl):
    b = buf.cpu().numpy()
    return (b[:sl.start] == GUARD_VALUE).all() and (b[sl.stop:] == GUARD_VALUE).all()


def run_case(name, splat=None, with_plane=True, out=None):
    c = R.REPROJECT_CASES[name]
    pred, K, T, Kd, plane = R.reproject_inputs(name)
    res = TP.reproject(dev(pred), dev(K), dev(T.reshape(-1, 3, 4)), dst_intrinsics=dev(Kd), size=(c["H"], c["W"]), dst_size=(c["Hd"], c["Wd"]),
                       lo=R.LO, hi=R.HI, splat=splat or c["splat"], z_near=R.Z_NEAR, plane=dev(plane) if with_plane else None, out=out)
    return res


# ---- 1. reproject against the reference --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.REPROJECT_CASES))
def test_reproject_matches_the_reference(name):
    c = R.REPROJECT_CASES[name]
    if c["interp"] == 0:                                  # the C entry point decides by the flag; the Python API by the sizes
        assert (c["h"], c["w"]) == (c["H"], c["W"])
    depth, index, plane = (t.cpu().numpy() for t in run_case(name))
    want_d, want_i32, want_p, _ = R.reproject_reference(name)
    _, want_i, _, _ = R.reproject_reference(name, np.float64)
    ex = R.reproject_excluded(name)
    keep = ~ex
    assert depth.dtype == np.float32 and index.dtype == np.int32 and plane.dtype == np.float32 and index.shape == want_i.shape
    wrong = (index != want_i) & keep
    print(f"{name}: {int((index != want_i).sum())} winners differ from the float64 reference, {int(wrong.sum())} outside the "
          f"{int(ex.sum())} excluded pixels of {ex.size}; {int((index < 0).sum())} holes")
    assert not wrong.any()
    assert np.array_equal(np.isnan(depth), index < 0) and np.array_equal(np.isnan(plane), index < 0)      # holes agree with each other ...
    assert np.array_equal((index < 0) & keep, (want_i < 0) & keep)                                          # ... and with the reference
    same = keep & (index == want_i32)                     # the float32 restatement took the same source here
    assert same.sum() >= 0.98 * keep.sum()
    R.close(depth, want_d, f"{name} depth", same)
    R.close(plane, want_p, f"{name} plane", same)
    src_max = c["H"] * c["W"]
    assert index.max() < src_max and index.min() >= -1
    # splat 2 covers a superset of what splat 1 covers
    i1 = run_case(name, splat=1, with_plane=False)[1].cpu().numpy()
    i2 = run_case(name, splat=2, with_plane=False)[1].cpu().numpy()
    assert not ((i1 >= 0) & (i2 < 0)).any() and (i2 >= 0).sum() >= (i1 >= 0).sum()      # floorf(u + 0.5f) is floorf(u) or floorf(u) + 1
    d_only, i_only = run_case(name, with_plane=False)
    assert i_only.cpu().numpy().tobytes() == index.tobytes() and d_only.cpu().numpy().tobytes() == depth.tobytes()


def test_occlusion_through_the_kernel():
    depth, index, _ = (t.cpu().numpy() for t in run_case("two_planes_occlusion"))
    want_d, want_i, _, _ = R.reproject_reference("two_planes_occlusion")
    assert np.array_equal(index, want_i) and depth.tobytes() == want_d.tobytes()      # no arithmetic rounds here: bit for bit
    assert (depth[0][:, 38:44] == np.float32(R.PLANES_NEAR)).all()                    # both planes land here, the near one wins


# ---- 2. reproducibility and bounds ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["odd_splat2", "register_37x53_to_29x61", "full_240x320_to_480x640"])
def test_reproject_is_reproducible_and_stays_inside_its_buffers(name):
    c = R.REPROJECT_CASES[name]
    B = len(c["K"])
    shape = (B, c["Hd"], c["Wd"])
    (d, db, ds), (i, ib, isl), (p, pb, ps) = guarded(shape, torch.float32), guarded(shape, torch.int32), guarded(shape, torch.float32)
    first = run_case(name)
    res = run_case(name, out=(d, i, p))
    assert res[0].data_ptr() == d.data_ptr() and res[1].data_ptr() == i.data_ptr() and res[2].data_ptr() == p.data_ptr()      # `out` is reused
    torch.cuda.synchronize()
    assert guards_intact(db, ds) and guards_intact(ib, isl) and guards_intact(pb, ps)
    for a, b in zip(first, res):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()                 # two launches, bitwise equal
    again = run_case(name, out=(d, i, p))
    for a, b in zip(first, again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="out"):
        run_case(name, out=(d, i))
    with pytest.raises(ValueError, match="out index"):
        run_case(name, out=(d, d, p))


def test_reproject_workspace_is_exactly_what_the_query_says():
    """The C entry point with a workspace of exactly the queried size between guards."""
    name = "register_37x53_to_29x61"
    c = R.REPROJECT_CASES[name]
    pred, K, T, Kd, _ = R.reproject_inputs(name)
    B = 1
    n = hip.load().cfp_depth_reproject_ws_bytes(B, c["Hd"], c["Wd"])
    assert n == 8 * c["Hd"] * c["Wd"]
    ws, wb, wsl = guarded((n // 8,), torch.int64)
    d = torch.empty(B, c["Hd"], c["Wd"], dtype=torch.float32, device=DEV)
    i = torch.empty(B, c["Hd"], c["Wd"], dtype=torch.int32, device=DEV)
    p, k, t, kd = dev(pred), dev(K), dev(T), dev(Kd)
    hip.call("cfp_depth_reproject", p.data_ptr(), c["h"], c["w"], c["H"], c["W"], B, 1, R.LO, R.HI, k.data_ptr(), t.data_ptr(), kd.data_ptr(),
             c["Hd"], c["Wd"], c["splat"], R.Z_NEAR, 0, 0, 0, 0, d.data_ptr(), i.data_ptr(), 0, ws.data_ptr(), n, hip.current_stream())
    torch.cuda.synchronize()
    assert guards_intact(wb, wsl)
    assert i.cpu().numpy().tobytes() == run_case(name, with_plane=False)[1].cpu().numpy().tobytes()


# ---- 3. the identity pose ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["odd_19x27_to_37x53", "same_24x40_direct", "full_240x320_to_480x640"])
def test_identity_pose_through_the_kernel(name):
    c = R.REPROJECT_CASES[name]
    pred, K, _, _, _ = R.reproject_inputs(name)
    p, k = dev(pred), dev(K)
    depth, index = TP.reproject(p, k, None, size=(c["H"], c["W"]), lo=R.LO, hi=R.HI, splat=1)
    z = PC.unproject(p, k, size=(c["H"], c["W"]), lo=R.LO, hi=R.HI)[..., 2].contiguous().cpu().numpy()
    depth, index = depth.cpu().numpy(), index.cpu().numpy()
    fin = np.isfinite(z)
    ident = np.broadcast_to(np.arange(c["H"] * c["W"], dtype=np.int32).reshape(c["H"], c["W"]), index.shape)
    assert np.array_equal(index[fin], ident[fin]) and (index[~fin] == -1).all()
    assert depth[fin].tobytes() == z[fin].tobytes() and np.isnan(depth[~fin]).all()
    # host numbers for the pose and the intrinsics, and a 4 x 4 matrix, give the same bits
    d2, i2 = TP.reproject(p[:1], tuple(float(v) for v in K[0]), np.eye(4), size=(c["H"], c["W"]), lo=R.LO, hi=R.HI)
    assert i2.cpu().numpy().tobytes() == index[:1].tobytes() and d2.cpu().numpy().tobytes() == depth[:1].tobytes()


# ---- 4. fuse -------------------------------------------------------------------------------------------------------------------------------

def run_fuse(name, out=None):
    cur, std, pd, pv = R.fuse_inputs(name)
    return TP.fuse(dev(cur), dev(std), dev(pd), dev(pv), lo=R.LO, hi=R.HI, out=out, **R.FUSE_NUMBERS)


@pytest.mark.parametrize("name", list(R.FUSE_CASES))
def test_fuse_matches_the_reference(name):
    depth, var, counts, stats = (t.cpu().numpy() for t in run_fuse(name))
    ref32, ref64, ex = R.fuse_reference(name), R.fuse_reference(name, np.float64), R.fuse_excluded(name)
    assert counts.dtype == np.int32 and stats.dtype == np.float64 and counts.shape == (len(ref32), 4) and stats.shape == (len(ref32), 2)
    for b, (a, d, e) in enumerate(zip(ref32, ref64, ex)):
        same = ~e & (a["row"] == d["row"])
        assert same.sum() == (~e).sum()
        R.close(depth[b], a["depth"], f"{name} image {b} depth", same)
        R.close(var[b], a["var"], f"{name} image {b} var", same)
        lo, n_ex = np.array(R.counts_of(d["row"], d["present"], ~e)), int(e.sum())
        print(f"{name} image {b}: counts {counts[b].tolist()}, reference outside the {n_ex} excluded pixels {lo.tolist()}")
        assert counts[b, 0] == d["present"].sum()                                     # no gate in this one
        assert ((counts[b, 1:] >= lo[1:]) & (counts[b, 1:] <= lo[1:] + n_ex)).all()    # exact when nothing is excluded
        assert counts[b, 1] + counts[b, 2] == (d["row"] >= 3).sum() and counts[b, 3] == lo[3]
        want = np.array([a["abs"].astype(np.float64).sum(), a["sq"].astype(np.float64).sum()])
        rel = np.abs(stats[b] - want) / want
        print(f"{name} image {b}: stats {stats[b].tolist()}, relative distance from the float64 sums of the float32 terms {rel.tolist()}")
        assert (rel <= 1e-12).all()


@pytest.mark.parametrize("name", ["odd_half_res", "full"])
def test_fuse_is_reproducible_and_stays_inside_its_buffers(name):
    cur, _, pd, _ = R.fuse_inputs(name)
    B, H, W = pd.shape
    (d, db, ds), (v, vb, vs) = guarded((B, H, W), torch.float32), guarded((B, H, W), torch.float32)
    (n, nb, ns), (s, sb, ss) = guarded((B, 4), torch.int32), guarded((B, 2), torch.float64)
    first = run_fuse(name)
    res = run_fuse(name, out=(d, v, n, s))
    assert all(r.data_ptr() == o.data_ptr() for r, o in zip(res, (d, v, n, s)))
    torch.cuda.synchronize()
    assert guards_intact(db, ds) and guards_intact(vb, vs) and guards_intact(nb, ns) and guards_intact(sb, ss)
    for a, b in zip(first, res):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    # the C entry point with a workspace of exactly the queried size between guards
    nbytes = hip.load().cfp_depth_fuse_ws_bytes(B, H, W)
    ws, wb, wsl = guarded((nbytes // 8,), torch.int64)
    again = TP.fuse(dev(cur), dev(R.fuse_inputs(name)[1]), dev(pd), dev(R.fuse_inputs(name)[3]), lo=R.LO, hi=R.HI, ws=ws, **R.FUSE_NUMBERS)
    torch.cuda.synchronize()
    assert guards_intact(wb, wsl)
    for a, b in zip(first, again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_fuse_takes_the_models_uncertainty_tensor():
    cur, std, pd, pv = R.fuse_inputs("odd_half_res")
    unc = np.stack([std, std * 0 + 7, std * 0 + 9], 1)                                # [B,3,h,w]: plane hip.UNC_STD is the std
    a = run_fuse("odd_half_res")
    b = TP.fuse(dev(cur), dev(unc), dev(pd), dev(pv), lo=R.LO, hi=R.HI, **R.FUSE_NUMBERS)
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


# ---- 5. the metric wrapper -----------------------------------------------------------------------------------------------------------------

def test_temporal_consistency():
    name = "odd_19x27_to_37x53"
    c = R.REPROJECT_CASES[name]
    pred, K, T, _, _ = R.reproject_inputs(name)
    rng = np.random.default_rng(5)
    cur = (np.nan_to_num(pred, nan=1.0, posinf=R.HI, neginf=R.LO) * (1 + rng.normal(0, 0.01, pred.shape))).astype(np.float32)
    got = metrics.temporal_consistency(dev(pred), dev(cur), dev(K), dev(T.reshape(-1, 3, 4)), R.LO, R.HI, size=(c["H"], c["W"])).cpu().numpy()
    assert got.shape == (3, 3) and got.dtype == np.float64
    warped, index = (t.cpu().numpy() for t in TP.reproject(dev(pred), dev(K), dev(T.reshape(-1, 3, 4)), size=(c["H"], c["W"]), lo=R.LO, hi=R.HI))
    for b in range(3):
        cg = P.depth(cur[b], c["H"], c["W"], 1)
        both = np.isfinite(warped[b]) & np.isfinite(cg)
        diff = (warped[b][both] - cg[both]).astype(np.float64)
        want = np.array([np.abs(diff).mean(), np.sqrt((diff * diff).mean()), float((index[b] >= 0).sum()) / (c["H"] * c["W"])])
        print(f"image {b}: {got[b].tolist()} against {want.tolist()}")
        # the current depth on the device is within RTOL * max(|c|, 1e-3) of the restatement's: every difference moves by at most
        # RTOL * HI, and so do their mean and (triangle inequality) their root mean square; the coverage is a ratio of integers, formed
        # on the device as a product with the reciprocal of H * W: an ulp or two of a number below 1
        assert abs(got[b, 2] - want[2]) <= 2.0 ** -51 and np.abs(got[b, :2] - want[:2]).max() <= R.RTOL * R.HI and 0 < want[0] < want[1]
