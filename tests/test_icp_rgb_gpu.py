"""`cfp_luma` and `cfp_icp_rgb_step` through `tracking.icp_rgb` / `tracking.Tracker` on the GPU against the numpy restatement
(`icp_rgb_ref.py`, which extends `icp_ref.py`).

The geometric half is `icp`'s bit for bit: the association map always, and pose, stats and sums too once the model picture holds no
colour.  The photometric pairing (the residual map's mask) is exact against the float64 restatement outside the excluded set fixed on
the CPU (test_icp_rgb_abi.py: at most 1 % of the stride grid, and numpy's float32 agrees with float64 on the rest).  The 60 sums are
compared with the float32 restatement on the GPU's own pairings, each within the project's 2e-5 of the sum of the absolute values of its
terms (the float32-vs-float64 gap of the restatement is below half of that for both halves: test_icp_rgb_abi.py); the counts are exact.
Behaviour: identical bits from call to call, capture and replay, the wall that `icp` refuses and the image resolves, convergence like
the float64 restatement's, and the `Tracker` with and without the option."""
import ctypes

import numpy as np
import pytest
import torch

import icp_ref as I
import icp_rgb_ref as C
import pointcloud_ref as P

pytestmark = pytest.mark.gpu

from cfpnet_amd import hip, tracking as TR, tsdf as TS  # noqa: E402

DEV = "cuda:0"
ROT_MARGIN, TRANS_MARGIN = 0.02, 2e-4                 # those of test_icp_gpu.py: degrees, metres


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)      # a copy: the shared inputs are read-only


def bits(t):
    return None if t is None else t.cpu().numpy().tobytes()


def pose_dev(T):
    return dev(np.asarray(T, np.float32).reshape(-1, 3, 4))


def all_bits(r):
    return tuple(bits(t) for t in r[:5]) + (bits(r.residual),)


def case_args(name):
    c, x = I.ICP_CASES[name], I.inputs(name)
    return (dev(x["pred"]), dev(x["K"]), dev(x["md"]), dev(x["mn"]), pose_dev(x["T"]), dev(x["std"]), dev(x["ms"]), dev(x["Km"]), I.GRID,
            dev(x["nsrc"]))


def case_call(name, iters=1, image=True, out=None, lumas=None, **over):
    """`icp_rgb` (or, without the image, `icp`) on the inputs of the case from its start pose, with the association and residual maps."""
    kw = dict(I.case_kw(name), iters=iters, ref_pose=pose_dev(np.stack([I.T_REF] * I.B)), index=True, out=out)
    kw.update(over)
    if not image:
        return TR.icp(*case_args(name), **kw)
    sl, ml = C.lumas(name) if lumas is None else lumas
    return TR.icp_rgb(*case_args(name), rgb=dev(sl), model_rgb=dev(ml), residual=True, **kw)


@pytest.fixture(scope="module")
def single_steps():
    """One step of every case with the image, without it, and with a model picture that holds no colour -- computed once, read-only."""
    out = {}
    for name in C.CASES:
        sl, ml = C.lumas(name)
        runs = dict(rgb=case_call(name), geo=case_call(name, image=False), blank=case_call(name, lumas=(sl, np.full_like(ml, np.nan))))
        out[name] = {k: {f: (None if t is None else t.cpu().numpy()) for f, t in r._asdict().items() if f != "ws"} for k, r in runs.items()}
    return out


# ---- cfp_luma ----------------------------------------------------------------------------------------------------------------------------------

def luma_dev(img, layout, mean=C.MEAN, std=C.STD):
    t = dev(img)
    B, H, W = (t.shape[0], t.shape[2], t.shape[3]) if layout == 0 else t.shape[:3]
    out = torch.full((B, H, W), -7.0, device=DEV)
    m, s = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    hip.call("cfp_luma", t.data_ptr(), layout, m if layout == 0 else None, s if layout == 0 else None, H, W, B, out.data_ptr(),
             hip.current_stream())
    return out.cpu().numpy()


def test_luma_against_numpy_for_both_layouts():
    """Odd sizes, more than one workgroup, NaN and Inf channels.  numpy's float32 rounds every operation once, like the library built
    without fused multiply-adds: the planes are equal bit for bit."""
    rng = np.random.default_rng(21)
    for B, H, W in ((3, 48, 64), (2, 37, 53), (1, 1, 5)):
        inter = rng.random((B, H, W, 3), dtype=np.float32)
        inter[0, 0, 0, 1], inter[-1, H // 2, W // 2, 2], inter[0, H - 1, W - 1, 0] = np.nan, np.inf, -np.inf
        got, want = luma_dev(inter, 1), C.luma(inter, 1)
        assert got.tobytes() == want.tobytes() and np.isnan(got[0, 0, 0]) and np.isnan(got[-1, H // 2, W // 2]) and np.isnan(got[0, H - 1, W - 1])
        assert np.isfinite(got).sum() == got.size - len({(0, 0, 0), (B - 1, H // 2, W // 2), (0, H - 1, W - 1)})
        planar = ((np.moveaxis(inter, -1, 1) - np.array(C.MEAN, np.float32)[:, None, None]) / np.array(C.STD, np.float32)[:, None, None])
        planar = np.ascontiguousarray(planar, np.float32)
        got, want = luma_dev(planar, 0), C.luma(planar, 0)
        assert got.tobytes() == want.tobytes() and np.isnan(got[0, 0, 0]) and np.nanmax(np.abs(got - C.luma(inter, 1))) < 1e-6
        other = luma_dev(planar, 0, (0.1, 0.2, 0.3), (1.5, 0.5, 2.0))
        assert other.tobytes() == C.luma(planar, 0, (0.1, 0.2, 0.3), (1.5, 0.5, 2.0)).tobytes() and other.tobytes() != got.tobytes()


def test_the_images_icp_rgb_accepts_give_the_planes_of_cfp_luma():
    """`rgb` as the normalised planar image and `model_rgb` as an interleaved picture in 0..1 equal the call on the ready planes."""
    name = "stride2_std"
    sl, ml = C.lumas(name)
    rgb = np.stack([sl * 1.1, sl, sl * 0.7], 1)
    rgb = np.ascontiguousarray((rgb - np.array(C.MEAN, np.float32)[:, None, None]) / np.array(C.STD, np.float32)[:, None, None], np.float32)
    pic = np.ascontiguousarray(np.stack([ml * 0.9, ml, ml * 1.2], -1), np.float32)
    kw = dict(I.case_kw(name), iters=2, residual=True)
    a = TR.icp_rgb(*case_args(name), rgb=dev(rgb), model_rgb=dev(pic), **kw)
    assert bits(a.src_luma) == C.luma(rgb, 0).tobytes() and bits(a.mdl_luma) == C.luma(pic, 1).tobytes()
    b = TR.icp_rgb(*case_args(name), rgb=dev(C.luma(rgb, 0)), model_rgb=dev(C.luma(pic, 1)), **kw)
    assert b.src_luma is None and b.mdl_luma is None and all_bits(a) == all_bits(b) and a.stats.shape == (2, I.B, 8)
    before = (a.src_luma.data_ptr(), a.mdl_luma.data_ptr(), a.pose.data_ptr())
    c = TR.icp_rgb(*case_args(name), rgb=dev(rgb), model_rgb=dev(pic), out=a, **kw)
    assert c is a and (c.src_luma.data_ptr(), c.mdl_luma.data_ptr(), c.pose.data_ptr()) == before and all_bits(c) == all_bits(b)
    with pytest.raises(ValueError, match="luminance plane"):
        TR.icp_rgb(*case_args(name), rgb=dev(rgb[:, :2]), model_rgb=dev(pic), **kw)
    with pytest.raises(ValueError, match="given together"):
        TR.icp_rgb(*case_args(name), rgb=dev(rgb), **kw)
    geo = TR.icp_rgb(*case_args(name), **I.case_kw(name), iters=2)                     # neither: `icp`, with its shapes
    assert geo.stats.shape == (2, I.B, 6) and geo.sums.shape == (I.B, 32) and geo.residual is None
    assert bits(geo.pose) == bits(TR.icp(*case_args(name), **I.case_kw(name), iters=2).pose)


# ---- one step ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.CASES)
def test_association_is_icps_and_the_residual_mask_is_the_restatements(single_steps, name):
    got, geo = single_steps[name]["rgb"], single_steps[name]["geo"]
    assert got["index"].tobytes() == geo["index"].tobytes()                           # bit for bit
    res = got["residual"]
    assert res.shape == (I.B,) + I.GRID and res.dtype == np.float32
    for b in range(I.B):
        d, ex = C.case_pairs(name, b, np.float64), C.case_excluded(name, b)
        mask = np.isfinite(res[b])
        differ = mask != d["photo"]
        print(f"{name} image {b}: {int(mask.sum())} photometric pairs, {int(differ.sum())} differ from the float64 restatement, "
              f"{int((differ & ~ex).sum())} outside the {int(ex.sum())} excluded pixels")
        assert not (differ & ~ex).any()
        assert np.isnan(res[b][~d["on"]]).all() and np.isnan(res[b][~mask]).all()     # off the stride grid: written, and NaN
        assert not (mask & (got["index"][b] < 0)).any() and mask.sum() > 0.5 * (got["index"][b] >= 0).sum()
        both = mask & d["photo"]
        # the residual itself, float32 against float64: the projections differ by less than GUARD / 4 pixels, where the picture changes by
        # less than 0.25 * 2 pi / 8 < 0.2 per pixel (test_the_painted_scene); the float32 blend and difference of values below 1 add 1e-6
        assert np.abs(res[b][both] - d["rI"][both]).max() <= 0.2 * I.guard_measured() / 4 + 1e-6


@pytest.mark.parametrize("name", C.CASES)
def test_without_colour_in_the_model_the_step_is_icps(single_steps, name):
    blank, geo = single_steps[name]["blank"], single_steps[name]["geo"]
    assert blank["sums"][:, :30].tobytes() == geo["sums"][:, :30].tobytes() and (blank["sums"][:, 30:] == 0).all()
    assert blank["pose"].tobytes() == geo["pose"].tobytes() and blank["world"].tobytes() == geo["world"].tobytes()
    assert blank["stats"][:, :, :6].tobytes() == geo["stats"].tobytes() and blank["index"].tobytes() == geo["index"].tobytes()
    assert (blank["stats"][:, :, 6] == 0).all() and np.isnan(blank["stats"][:, :, 7]).all() and np.isnan(blank["residual"]).all()
    rgb = single_steps[name]["rgb"]
    assert rgb["sums"][:, :30].tobytes() == geo["sums"][:, :30].tobytes()             # the geometric sums do not see the image either
    assert rgb["pose"].tobytes() != geo["pose"].tobytes()


@pytest.mark.parametrize("name", C.CASES)
def test_sums_against_the_float32_restatement_on_the_gpus_own_pairs(single_steps, name):
    got = single_steps[name]["rgb"]
    assert got["sums"].shape == (I.B, 64) and got["sums"].dtype == np.float64 and (got["sums"][:, 60:] == 0).all()
    for b in range(I.B):
        geo, lum = C.case_maps(name, b, np.float32)
        mask = np.isfinite(got["residual"][b])
        want, scale = C.sums(C.pairs(*geo, I.inputs(name)["T"][b], *lum, index=got["index"][b].astype(np.int64), photo=mask,
                                     **I.case_kw(name)))
        worst = float((np.abs(got["sums"][b, :60] - want) / np.maximum(scale, 1e-300)).max())
        print(f"{name} image {b}: {int(want[29])} + {int(want[59])} pairs, worst |got - want| / (sum of |terms|) = {worst:.3e} (bound {I.RTOL:.1e})")
        assert got["sums"][b, 29] == want[29] == (got["index"][b] >= 0).sum() and got["sums"][b, 59] == want[59] == mask.sum()
        assert (np.abs(got["sums"][b, :60] - want) <= I.RTOL * scale).all()
        st = got["stats"][0, b]
        assert st[0] == want[29] and st[6] == want[59] and abs(st[7] - np.sqrt(want[57] / want[58])) <= 1e-5 * st[7]
        assert abs(got["sums"][b, 58] - want[59] * np.float64(np.float32(C.PHOTO_WEIGHT))) <= 1e-9 * got["sums"][b, 58]


@pytest.mark.parametrize("name", C.CASES)
def test_one_step_against_the_restatement(single_steps, name):
    got = single_steps[name]["rgb"]
    tol = 1e-6                                                                        # max(2 x the gap measured on the CPU (<= 5e-7 asserted there), 1e-6)
    for b in range(I.B):
        T0 = I.inputs(name)["T"][b]
        want, ok, xi = C.step(got["sums"][b, :60], T0)
        assert ok and got["stats"][0, b, 5] == 1.0
        T = got["pose"][b].ravel()
        worst = float(np.abs(T.astype(np.float64) - want).max())
        ww = float(np.abs(got["world"][b].ravel().astype(np.float64) - I.world(T, I.T_REF)).max())
        print(f"{name} image {b}: worst |T' - want| = {worst:.3e}, |T_world - want| = {ww:.3e} (bound {tol:.1e})")
        assert worst <= tol and ww <= tol
        assert abs(got["stats"][0, b, 3] - np.linalg.norm(xi[:3])) <= 1e-6 and abs(got["stats"][0, b, 4] - np.linalg.norm(xi[3:])) <= 1e-6


def test_photo_max_gates_and_infinity_does_not():
    name = "stride1_plain"
    tight, loose = case_call(name, photo_max=0.02), case_call(name, photo_max=float("inf"))
    nt, nl = tight.stats[0, :, 6].cpu().numpy(), loose.stats[0, :, 6].cpu().numpy()
    rt = tight.residual.cpu().numpy()
    assert (nt < nl).all() and (nt > 0).all() and np.nanmax(np.abs(rt)) <= 0.02 and np.nanmax(np.abs(loose.residual.cpu().numpy())) > 0.02
    for b in range(I.B):                                                              # with no gate: every pair whose cell and frame pixel hold a luminance
        d = C.pairs(*C.case_maps(name, b, np.float64)[0], I.inputs(name)["T"][b], *C.case_maps(name, b, np.float64)[1],
                    photo_max=np.inf, **I.case_kw(name))
        assert abs(int(nl[b]) - int(d["photo"].sum())) <= C.case_excluded(name, b).sum()


# ---- behaviour ---------------------------------------------------------------------------------------------------------------------------------

def test_two_calls_give_identical_bits_and_out_is_written_in_place():
    name = "stride1_normals_std"
    a, b = case_call(name, iters=3), case_call(name, iters=3)
    assert all_bits(a) == all_bits(b) and a.stats.shape == (3, I.B, 8) and a.sums.shape == (I.B, 64)
    c = case_call(name, iters=3, out=b)
    assert c.pose.data_ptr() == b.pose.data_ptr() and c.residual.data_ptr() == b.residual.data_ptr() and all_bits(c) == all_bits(a)
    with pytest.raises(ValueError, match="out stats"):
        case_call(name, iters=2, out=b)
    with pytest.raises(ValueError, match="out stats"):                                # the result of `icp` does not fit
        case_call(name, iters=3, out=case_call(name, iters=3, image=False))
    with pytest.raises(ValueError, match="out residual"):
        TR.icp_rgb(*case_args(name), rgb=dev(C.lumas(name)[0]), model_rgb=dev(C.lumas(name)[1]), iters=3, index=True,
                   ref_pose=pose_dev(np.stack([I.T_REF] * I.B)), out=b, **I.case_kw(name))


def test_icp_rgb_under_graph_capture():
    """A captured `icp_rgb` (10 iterations, images in, luminance planes inside the graph) replayed on a second frame equals the eager call."""
    name, other = "stride1_normals_std", "stride2_std"
    x, y = I.inputs(name), I.inputs(other)
    kw = dict(I.case_kw(name), iters=10, index=True, residual=True)
    K, md, mn, ms, ref = dev(x["K"]), dev(x["md"]), dev(x["mn"]), dev(x["ms"]), pose_dev(np.stack([I.T_REF] * I.B))
    nsrc_y = np.stack([P.normals(P.depth(y["pred"][b], *I.GRID, 0), I.K_GRID[b]) for b in range(I.B)])
    pic = dev(np.ascontiguousarray(np.stack([C.lumas(name)[1]] * 3, -1)))             # the model's picture, interleaved
    img = [C.to_rgb(C.lumas(n)[0].astype(np.float64) / C.tint_luma(1.0)) for n in (name, other)]
    ident = I.ID12.reshape(1, 12).repeat(I.B, 0)
    frames = ((x["pred"], x["std"], x["nsrc"], x["T"], img[0]), (y["pred"], y["std"], nsrc_y, ident, img[1]))

    def eager(pred, std, nsrc, T, rgb):
        return all_bits(TR.icp_rgb(dev(pred), K, md, mn, pose_dev(T), dev(std), ms, None, I.GRID, dev(nsrc), ref_pose=ref, rgb=dev(rgb),
                                   model_rgb=pic, **kw))

    want = [eager(*f) for f in frames]
    assert want[0] != want[1]
    sp, su, sn, sT, sr = dev(x["pred"]), dev(x["std"]), dev(x["nsrc"]), pose_dev(x["T"]), dev(img[0])

    def run(out=None):
        return TR.icp_rgb(sp, K, md, mn, sT, su, ms, None, I.GRID, sn, ref_pose=ref, out=out, rgb=sr, model_rgb=pic, **kw)

    out = run()
    assert all_bits(out) == want[0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                             # warm-up on the side stream, as capture asks for
        run(out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(out)
    for k, (pred, std, nsrc, T, rgb) in enumerate(frames):
        sp.copy_(dev(pred)); su.copy_(dev(std)); sn.copy_(dev(nsrc)); sT.copy_(pose_dev(T)); sr.copy_(dev(rgb))
        graph.replay()
        torch.cuda.synchronize()
        assert all_bits(out) == want[k], k


def test_the_wall():
    """One fronto-parallel textured plane at 2 m, the camera a degree about every axis and 1 to 3 cm away: `icp` refuses every step;
    with the image every step is accepted and the pose ends within twice the float64 restatement's error plus the margins."""
    x = C.wall_inputs()
    args = (dev(x["pred"]), dev(x["K"]), dev(x["md"]), dev(x["mn"]), None, dev(x["std"]), dev(x["ms"]), None, I.GRID)
    r = TR.icp(*args, iters=C.WALL_ITERS)
    st = r.stats.cpu().numpy()
    assert (st[..., 5] == 0).all() and (st[..., 0] > 2500).all() and bits(r.pose) == np.stack([I.ID12] * I.B).tobytes()
    r = TR.icp_rgb(*args, iters=C.WALL_ITERS, rgb=dev(x["sl"]), model_rgb=dev(x["ml"]))
    st, T = r.stats.cpu().numpy(), r.pose.cpu().numpy().reshape(I.B, 12)
    for b, (_, st0, (deg0, tr0)) in enumerate(C.wall_reference(True)):
        deg, tr = I.pose_error(T[b], x["T_true"][b])
        print(f"wall image {b}: error {deg:.4f} deg / {1e3 * tr:.3f} mm (float64 restatement {deg0:.4f} / {1e3 * tr0:.3f}), photo rms "
              f"{st[0, b, 7]:.4f} -> {st[-1, b, 7]:.5f}, {int(st[-1, b, 6])} photometric pairs")
        assert st[:, b, 5].all() and st[-1, b, 6] > 2500
        assert deg <= 2 * deg0 + ROT_MARGIN and tr <= 2 * tr0 + TRANS_MARGIN
        assert st[-1, b, 7] < 0.05 * st[0, b, 7]


def test_convergence_from_the_identity_on_the_painted_scene():
    x = I.converge_inputs(C.CONVERGE_MOTION)
    sl, ml = C.converge_lumas()
    H, W = I.GRID
    std, ms = torch.full((I.B, H, W), C.FRAME_STD, device=DEV), torch.full((I.B, H, W), C.MODEL_STD, device=DEV)
    for stride in (1, 2):
        r = TR.icp_rgb(dev(x["pred"]), dev(x["K"]), dev(x["md"]), dev(x["mn"]), None, std, ms, size=I.GRID, iters=C.CONVERGE_ITERS,
                       stride=stride, rgb=dev(sl), model_rgb=dev(ml))
        T, st = r.pose.cpu().numpy().reshape(I.B, 12), r.stats.cpu().numpy()
        for b, (_, _, (deg0, tr0)) in enumerate(C.converge_reference(stride)):
            deg, tr = I.pose_error(T[b], x["T_true"][b])
            print(f"stride {stride} image {b}: error {deg:.4f} deg / {1e3 * tr:.3f} mm (float64 restatement {deg0:.4f} / {1e3 * tr0:.3f})")
            assert deg <= 2 * deg0 + ROT_MARGIN and tr <= 2 * tr0 + TRANS_MARGIN
            assert st[:, b, 5].all() and st[-1, b, 7] < st[0, b, 7] and st[-1, b, 2] < st[0, b, 2]


# ---- Tracker -------------------------------------------------------------------------------------------------------------------------------

def make_volume():
    return TS.TsdfVolume(I.TRACK_DIMS, I.TRACK_VOXEL, I.TRACK_ORIGIN, dev(np.array(I.K_GRID, np.float32)), size=I.GRID, trunc=I.TRACK_TRUNC,
                         hi=I.TRACK_HI)


def make_tracker(**kw):
    return TR.Tracker(make_volume(), pose_dev(I.track_frames()[0][2]), iters=I.TRACK_ITERS, **kw)


def test_tracker_with_the_image_against_raw_calls_and_capture():
    fr, im = I.track_frames(), C.track_images()
    t = make_tracker(photo_std=C.PHOTO_STD)
    poses, stats = [], []
    for f, (pred, std, _) in enumerate(fr):
        p, s = t.update_rgb(dev(pred), dev(im[f]), dev(std))
        poses.append(p.clone())
        stats.append(None if s is None else s.clone())
    assert stats[0] is None and bits(poses[0]) == fr[0][2].tobytes() and all(s.shape == (I.TRACK_ITERS, I.B, 8) for s in stats[1:])
    volume, color = bits(t.volume.volume), bits(t.volume.color)
    # the same sequence of raw calls by hand
    v = make_volume()
    last = pose_dev(fr[0][2])
    v.integrate_rgb(dev(fr[0][0]), dev(im[0]), dev(fr[0][1]), last)
    for f in range(1, I.TRACK_FRAMES):
        pred, std, rgb = dev(fr[f][0]), dev(fr[f][1]), dev(im[f])
        d, s, n = v.raycast(last, normals=True)
        r = TR.icp_rgb(pred, v.camera, d, n, None, std, s, None, v.grid_size, iters=I.TRACK_ITERS, lo=v.lo, hi=v.hi, std_floor=v.std_floor,
                       z_near=v.z_near, ref_pose=last, rgb=rgb, model_rgb=v.shade(d, last), photo_std=C.PHOTO_STD)
        last = r.world.clone()
        v.integrate_rgb(pred, rgb, std, last)
        assert bits(last) == bits(poses[f]) and bits(r.stats) == bits(stats[f]), f
    assert bits(v.volume) == volume and bits(v.color) == color
    for f in range(1, I.TRACK_FRAMES):                                                # the image takes part, and the track holds
        st = stats[f].cpu().numpy()
        got = poses[f].cpu().numpy().reshape(I.B, 12)
        assert st[-1, :, 5].all() and (st[-1, :, 6] > 0.5 * st[-1, :, 0]).all() and (st[-1, :, 7] < C.PHOTO_MAX).all()
        for b in range(I.B):
            deg, tr = I.pose_error(got[b], I.track_pose(f, b))
            print(f"frame {f} image {b}: error {deg:.4f} deg / {1e3 * tr:.3f} mm, {int(st[-1, b, 6])} photometric of {int(st[-1, b, 0])} pairs, "
                  f"photo rms {st[-1, b, 7]:.4f}")
            assert deg < 0.5 and tr < 0.5 * I.TRACK_VOXEL                             # the figures test_icp_gpu.py holds its bounds against
    # a captured update_rgb replayed on the frames equals the eager calls
    g = make_tracker(photo_std=C.PHOTO_STD)
    sp, su, sr = dev(fr[0][0]), dev(fr[0][1]), dev(im[0])
    g.update_rgb(sp, sr, su)
    sp.copy_(dev(fr[1][0])); su.copy_(dev(fr[1][1])); sr.copy_(dev(im[1]))
    state = (g.volume.volume.clone(), g.volume.color.clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                             # warm-up on the side stream, as capture asks for
        g.update_rgb(sp, sr, su)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = g.update_rgb(sp, sr, su)
    g.volume.volume.copy_(state[0]); g.volume.color.copy_(state[1])      # the warm-up advanced the volumes and the pose: put the first frame's back
    g.pose.copy_(pose_dev(fr[0][2]))
    for f in range(1, I.TRACK_FRAMES):
        sp.copy_(dev(fr[f][0])); su.copy_(dev(fr[f][1])); sr.copy_(dev(im[f]))
        graph.replay()
        torch.cuda.synchronize()
        assert bits(out[0]) == bits(poses[f]) and bits(out[1]) == bits(stats[f]), f
    assert bits(g.volume.volume) == volume and bits(g.volume.color) == color


def test_tracker_without_the_option_is_as_it_was():
    """photo_std=None: `update_rgb` gives `update`'s poses and stats and `integrate_rgb`'s volumes, bit for bit."""
    fr, im = I.track_frames(), C.track_images()
    a, b = make_tracker(), make_tracker(photo_std=None)
    v = make_volume()
    for f, (pred, std, _) in enumerate(fr):
        pa, sa = a.update(dev(pred), dev(std))
        pb, sb = b.update_rgb(dev(pred), dev(im[f]), dev(std))
        assert bits(pa) == bits(pb) and bits(sa) == bits(sb) and (sb is None or sb.shape == (I.TRACK_ITERS, I.B, 6)), f
        v.integrate_rgb(dev(pred), dev(im[f]), dev(std), pa)
    assert bits(b.volume.volume) == bits(a.volume.volume) == bits(v.volume) and bits(b.volume.color) == bits(v.color)
    # and with the option, a frame without an image still tracks by geometry
    c = make_tracker(photo_std=C.PHOTO_STD)
    c.update_rgb(dev(fr[0][0]), dev(im[0]), dev(fr[0][1]))
    p, s = c.update(dev(fr[1][0]), dev(fr[1][1]))
    assert s.shape == (I.TRACK_ITERS, I.B, 6)
    p2, s2 = c.update_rgb(dev(fr[2][0]), dev(im[2]), dev(fr[2][1]))
    assert s2.shape == (I.TRACK_ITERS, I.B, 8) and s2[-1, :, 5].cpu().numpy().all()
