"""Colour in the TSDF map on the GPU: `TsdfVolume.integrate_rgb` / `shade` / `surface_colors`, `write_ply(colors=True)` and
`Tracker.update_rgb` against the numpy restatement (`tsdf_color_ref.py`), at the shapes of test_tsdf_gpu.py.

The geometry of an `integrate_rgb` is compared bit for bit with a plain `integrate` of the same inputs on a second volume.  Which voxels
are coloured is exact against the float64 restatement outside the excluded set fixed on the CPU (test_tsdf_color_abi.py: at most 1 % of
a step, numpy's float32 agreeing with float64 on the rest); every step starts from the float32 restatement's states of that frame.
Values -- C_k, Wc, the shaded image, the surface colours -- lie within the project's 2e-5 * max(|want|, 1e-3) of the float32
restatement, with NaN at exactly the same places.  Behaviour: two runs give identical bits, a captured chain replays bit for bit, the
PLY round-trips, the tracker equals the raw calls."""
import numpy as np
import pytest
import torch

import icp_ref as I
import tsdf_color_ref as C
import tsdf_ref as S
import tsdf_surface_ref as S2

pytestmark = pytest.mark.gpu

from cfpnet_amd import pointcloud, tracking as TR, tsdf as TS  # noqa: E402

DEV = "cuda:0"
NVOX = S.DIMS[0] * S.DIMS[1] * S.DIMS[2]


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)             # a copy: the shared inputs are read-only


def bits(t):
    return t.cpu().numpy().tobytes()


def pose_dev(T):
    return dev(np.asarray(T, np.float32).reshape(-1, 3, 4))


def frame_dev(name, f):
    """(pred, rgb, std, pose): the arguments of integrate_rgb."""
    pred, std, T = S.frames(name)[f]
    return dev(pred), dev(C.images()[f]), (None if std is None else dev(std)), pose_dev(T)


def plain(frame):
    pred, _, std, T = frame
    return pred, std, T


def make_volume(name, state=None, color=None, case=None):
    """A TsdfVolume of the case with both volumes allocated (by a first integrate_rgb), emptied, and `state` / `color` uploaded."""
    c = S.TSDF_CASES[case or name]
    v = TS.TsdfVolume(S.DIMS, S.VOXEL, c["origin"], dev(np.array(S.K_GRID, np.float32)), size=S.GRID, trunc=S.TRUNC, w_max=c["w_max"])
    assert v.color is None and v.color_counts is None
    v.integrate_rgb(*frame_dev(name, 0), C.MEAN, C.CSTD)
    v.reset()
    assert v.color.shape == (S.B, S.DIMS[2], S.DIMS[1], S.DIMS[0], 4) and not v.color.any() and v.color.data_ptr() % 16 == 0
    if state is not None:
        v.volume.copy_(dev(state))
    if color is not None:
        v.color.copy_(dev(color))
    return v


def final_volume(name):
    return make_volume(name, S.states(name)[-1], C.color_states(name)[-1])


@pytest.mark.parametrize("name", ["blend_24x32", "direct_48x64", "no_std", "w_max_binds"])
def test_integrate_rgb_against_the_restatement(name):
    v, p = make_volume(name), make_volume(name)
    for f in range(len(S.POSES)):
        before, cbefore = S.states(name)[f], C.color_states(name)[f]
        for vol in (v, p):
            vol.volume.copy_(dev(before))
        v.color.copy_(dev(cbefore))
        kept = bits(v.counts)
        frame = frame_dev(name, f)
        counts = v.integrate_rgb(*frame, C.MEAN, C.CSTD)
        c3 = p.integrate(*plain(frame))
        assert counts is v.color_counts and counts.shape == (S.B, 4) and counts.dtype == torch.int32 and bits(v.counts) == kept
        assert bits(v.volume) == bits(p.volume) and bits(counts[:, :3].contiguous()) == bits(c3), (name, f)      # the geometry, bit for bit
        got, n = v.color.cpu().numpy(), counts.cpu().numpy()
        for b in range(S.B):
            a, d, ex = C.step_reference(name, f, b), C.step_reference(name, f, b, np.float64), C.step_excluded(name, f, b)
            keep = ~ex
            changed = (got[b] != cbefore[b]).any(-1)
            visible = (a["col"] != cbefore[b]).any(-1)                                 # under a binding w_max a colour may leave all four numbers as they were
            assert np.array_equal(changed[keep], (d["coloured"] & visible)[keep]), (name, f, b)
            assert not (changed & ~d["updated"] & keep).any()
            low, room = C.counts_of(d, keep)[3], int(ex.sum())
            print(f"{name} frame {f} image {b}: counts {n[b].tolist()}, coloured in float64 outside the excluded set {low}, {room} voxels excluded")
            assert low <= int(n[b][3]) <= low + room and n[b][3] <= n[b][1]
            for k, what in enumerate(("R", "G", "B", "Wc")):
                C.close(got[b][..., k], a["col"][..., k], f"{name} frame {f} image {b} {what}", keep)
    if name == "w_max_binds":
        assert (got[..., 3] == 900.0).sum() > 500 and got[..., 3].max() == 900.0


def test_integrate_rgb_reads_the_pixel_the_float64_restatement_names_and_skips_a_nan_channel():
    """On an empty volume with mean 0 and std 1 a coloured voxel holds the image itself (c * w / w), so the (pix + 1) / (H W) channel
    shows which pixel it read.  Then the case's own frame 0: where image 2 reads its NaN patch nothing is coloured and the geometry
    still updates."""
    name = "blend_24x32"
    v = make_volume(name)
    pred, _, std, T = frame_dev(name, 0)
    v.integrate_rgb(pred, dev(C.pix_image()), std, T, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    col = v.color.cpu().numpy()
    for b in range(S.B):
        d, ex = C.step_reference(name, 0, b, np.float64), C.step_excluded(name, 0, b)
        keep = ~ex
        assert np.array_equal((col[b][..., 3] > 0)[keep], d["band"][keep])            # the image has no NaN: every voxel of the band
        sel = d["band"] & keep
        pix = C.pix_of(col[b][..., 0][sel])
        assert np.array_equal(pix, d["pix"][sel]) and np.abs(col[b][..., 1][sel] - 0.25).max() < 1e-6
        print(f"image {b}: {int(sel.sum())} coloured voxels read {np.unique(pix).size} different pixels, all the float64 restatement's")
    v.reset()
    v.integrate_rgb(*frame_dev(name, 0), C.MEAN, C.CSTD)
    b, k, rows, cols = C.NAN_PATCH
    d, ex = C.step_reference(name, 0, b, np.float64), C.step_excluded(name, 0, b)
    patch = np.zeros(S.GRID, bool)
    patch[rows, cols] = True
    reads = (d["pix"] >= 0) & patch.ravel()[np.maximum(d["pix"], 0)] & ~ex
    col, vol = v.color[b].cpu().numpy(), v.volume[b].cpu().numpy()
    assert (reads & d["band"]).sum() > 50 and not col[reads].any()                    # neither read nor written
    assert (vol[reads & d["updated"]][:, 1] > 0).all() and (reads & d["updated"]).sum() > 50
    assert (col[d["coloured"] & ~ex][:, 3] > 0).all()


def test_a_volume_outside_the_view_is_not_touched():
    name = "outside_the_view"
    state, cstate = S.states("blend_24x32")[-1], C.color_states("blend_24x32")[-1]   # something worth keeping
    v = make_volume("blend_24x32", state, cstate, case=name)
    for f in range(len(S.POSES)):
        counts = v.integrate_rgb(*frame_dev(name, f), C.MEAN, C.CSTD)
        assert counts.cpu().tolist() == [[0, 0, 0, 0]] * S.B and bits(v.volume) == state.tobytes() and bits(v.color) == cstate.tobytes()


def test_frames_with_and_without_an_image_mix_and_two_runs_give_identical_bits():
    name = "blend_24x32"
    fr = [frame_dev(name, f) for f in range(3)]
    p = make_volume(name)
    for f in range(3):
        p.integrate(*plain(fr[f]))
        if f == 0:
            after0 = p.volume.clone()
    res = []
    for _ in range(2):
        v = make_volume(name)
        v.integrate(*plain(fr[0]))
        n = v.integrate_rgb(*fr[1], C.MEAN, C.CSTD)
        v.integrate(*plain(fr[2]))
        res.append((bits(v.volume), bits(v.color), bits(n)))
    assert res[0] == res[1] and res[0][0] == bits(p.volume)                           # the geometry of three plain integrates
    alone = make_volume(name, after0.cpu().numpy())
    alone.integrate_rgb(*fr[1], C.MEAN, C.CSTD)
    assert res[0][1] == bits(alone.color) and alone.color[..., 3].max() > 0           # the colour of the middle frame alone
    # the checks of integrate_rgb's own
    with pytest.raises(ValueError, match=r"rgb must be \[B,3,H,W\]"):
        v.integrate_rgb(fr[1][0], fr[1][1][:, :, :-1], fr[1][2], fr[1][3])
    with pytest.raises(ValueError, match=r"rgb must be \[B,3,H,W\]"):
        v.integrate_rgb(fr[1][0], fr[1][1][:2], fr[1][2], fr[1][3])
    with pytest.raises(ValueError, match=r"rgb must be \[B,3,H,W\]"):
        v.integrate_rgb(fr[1][0], fr[1][1][:, :2], fr[1][2], fr[1][3])
    with pytest.raises(ValueError, match="float32 device tensor"):
        v.integrate_rgb(fr[1][0], fr[1][1].double(), fr[1][2], fr[1][3])
    with pytest.raises(ValueError, match="3 finite numbers"):
        v.integrate_rgb(*fr[1], (0.0, float("nan"), 0.0), C.CSTD)
    assert bits(v.volume) == res[0][0] and bits(v.color) == res[0][1]                 # a refused call changes nothing
    v.reset()
    assert not v.color.any() and bits(v.volume) == np.stack([S.empty_volume(S.DIMS)] * S.B).tobytes()


@pytest.mark.parametrize("name", list(S.RAYCAST_CASES))
def test_shade_against_the_restatement(name):
    c = S.RAYCAST_CASES[name]
    v = final_volume(c["case"])
    K, T = dev(np.array(c["K"], np.float32)), pose_dev(c["T"])
    depth, _, _ = v.raycast(T, K, (c["Hd"], c["Wd"]), c["t_range"], c["step"])
    rgb = v.shade(depth, T, K)
    assert rgb.shape == depth.shape + (3,) and rgb.dtype == torch.float32
    first = bits(rgb)
    assert v.shade(depth, T, K) is rgb and bits(rgb) == first                         # the cached buffer, the same bits
    gd, got = depth.cpu().numpy(), rgb.cpu().numpy()
    origin = S.TSDF_CASES[c["case"]]["origin"]
    for b in range(S.B):
        want = C.shade(C.color_states(c["case"])[-1][b], c["K"][b], c["T"][b], gd[b], origin, S.VOXEL)      # on the GPU's own depth
        C.close(got[b], want, f"{name} image {b} shade")                              # and NaN at exactly the same places
        nan = np.isnan(got[b]).any(-1)
        hit = ~np.isnan(gd[b])
        assert np.array_equal(nan, np.isnan(got[b]).all(-1)) and nan[~hit].all() and (~hit).any() and (~nan).sum() > 0.9 * hit.sum()
        print(f"{name} image {b}: {int(hit.sum())} hits, {int((~nan).sum())} with a colour")
    other = torch.full_like(rgb, -7.0)
    assert v.shade(depth, T, K, out=other) is other and bits(other) == first
    # any metric depth on that grid: a NaN, an infinite and a far depth give NaN, the rest is unchanged
    d2 = depth.clone()
    d2[:, 3, 5], d2[:, 4, 6], d2[:, 5, 7] = float("nan"), float("inf"), 9.0
    r2 = v.shade(d2, T, K, out=torch.empty_like(rgb)).cpu().numpy()
    assert np.isnan(r2[:, 3, 5]).all() and np.isnan(r2[:, 4, 6]).all() and np.isnan(r2[:, 5, 7]).all()
    r2[:, 3, 5], r2[:, 4, 6], r2[:, 5, 7] = got[:, 3, 5], got[:, 4, 6], got[:, 5, 7]
    assert r2.tobytes() == first
    with pytest.raises(ValueError, match="depth must be"):
        v.shade(depth[:2], T, K)
    with pytest.raises(ValueError, match="out must be"):
        v.shade(depth, T, K, out=other[:, :-1])


def _colors_sentinel(B, cap):
    return torch.full((B, cap, 3), -7.0, device=DEV)


@pytest.mark.parametrize("name", list(S2.STATE_CASES))
def test_surface_colors_against_the_restatement(name):
    v = final_volume(name)
    for mj in (None, S2.JUMP):
        sp = v.surface_points(max_jump=mj)
        assert sp.colors is None and sp.split()[0]["colors"] is None
        colors = v.surface_colors(sp)
        assert colors is sp.colors and colors.shape == (S.B, sp.capacity, 3)
        first = bits(colors)
        assert v.surface_colors(sp) is colors and bits(colors) == first               # sp.colors is reused; the same bits
        parts = sp.split()
        for b in range(S.B):
            ref = C.surface_reference(name, b, 0.0, np.inf if mj is None else mj)
            got = parts[b]["colors"].cpu().numpy()
            assert np.array_equal(parts[b]["index"].cpu().numpy(), S2.reference(name, b, 0.0, np.inf if mj is None else mj)["index"])
            C.close(got, ref["colors"], f"{name} max_jump {mj} image {b} surface colours")
            assert not np.isnan(got).any() and (ref["ends"] >= 1).all()               # every point has a colour
            assert mj is not None or (ref["ends"] == 1).any()                         # and without the jump filter both branches are taken
    # rows beyond the count are untouched; a capacity below the count colours the first rows only
    full = v.surface_points()
    v.surface_colors(full)
    counts = full.counts.cpu().tolist()
    cap = max(counts) + 6
    big = v.surface_points(capacity=cap)
    big.index[:] = torch.where(torch.arange(cap, device=DEV)[None, :] < full.counts[:, None], big.index,
                               torch.where(torch.arange(cap, device=DEV)[None, :] % 2 == 0, -7, 2 ** 31 - 1).to(torch.int32))
    out = v.surface_colors(big, out=_colors_sentinel(S.B, cap))
    for b, n in enumerate(counts):
        assert (out[b, n:] == -7).all() and bits(out[b, :n]) == bits(full.colors[b, :n])      # what lies beyond the rows is never read
    small = min(counts) - 7
    few = v.surface_points(capacity=small)
    got = v.surface_colors(few, out=_colors_sentinel(S.B, small))
    assert few.counts.cpu().tolist() == counts and bits(got) == bits(full.colors[:, :small].contiguous())
    # an index that names no edge of the lattice, inside the rows: NaN there, the other rows as before -- the guarded path, by value
    bad = v.surface_points(capacity=cap)
    for row, e in ((2, 3 * NVOX), (4, -1), (6, 2 ** 31 - 1), (8, 3 * (S.DIMS[0] - 1)), (9, 3 * (NVOX - 1) + 2), (11, 3 * (NVOX - S.DIMS[0]) + 1)):
        bad.index[:, row] = e
    got = v.surface_colors(bad, out=_colors_sentinel(S.B, cap)).cpu().numpy()
    rows = [2, 4, 6, 8, 9, 11]
    assert np.isnan(got[:, rows]).all()
    want = out.cpu().numpy().copy()
    want[:, rows] = got[:, rows]
    assert got.tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="out must be"):
        v.surface_colors(full, out=_colors_sentinel(S.B, cap))
    with pytest.raises(ValueError, match="sp must be"):
        v.surface_colors(full.points)


def test_the_whole_chain_under_graph_capture():
    """One captured integrate_rgb + raycast + shade + surface_points(capacity, out) + surface_colors(out), replayed on new inputs and a
    new pose, equals the eager calls bit for bit."""
    name, rc, cap = "blend_24x32", S.RAYCAST_CASES["blend_to_37x53"], 2048
    K = dev(np.array(rc["K"], np.float32))
    size = (rc["Hd"], rc["Wd"])
    views = [pose_dev(S.POSE_VIEW), pose_dev(S.POSES[1]), pose_dev(S.POSES[0])]

    def run(v, frame, view, out):
        v.integrate_rgb(*frame, C.MEAN, C.CSTD)
        rays = v.raycast(view, K, size, rc["t_range"], rc["step"])
        rgb = v.shade(rays[0], view, K)
        sp = v.surface_points(capacity=cap, out=out)
        v.surface_colors(sp)
        return rays, rgb, sp

    def snapshot(v, rays, rgb, sp):
        n = sp.counts.cpu().tolist()
        assert max(n) <= cap
        return (bits(v.volume), bits(v.color), bits(v.color_counts), bits(rgb), bits(sp.counts)) + tuple(bits(t) for t in rays) + \
            tuple(bits(t[b, :m]) for b, m in enumerate(n) for t in (sp.points, sp.index, sp.colors))

    eager = make_volume(name)
    want, eo = [], None
    for f in range(len(S.POSES)):
        res = run(eager, frame_dev(name, f), views[f], eo)
        eo = res[2]
        want.append(snapshot(eager, *res))
    assert want[0] != want[1] != want[2]
    g = make_volume(name)
    frame = tuple(t.clone() for t in frame_dev(name, 0))
    sV = views[0].clone()
    res = run(g, frame, sV, None)                             # the first frame eagerly: every buffer exists afterwards
    assert snapshot(g, *res) == want[0]
    state, cstate = g.volume.clone(), g.color.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                             # warm-up on the side stream, as capture asks for
        run(g, frame, sV, res[2])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(g, frame, sV, res[2])
    g.volume.copy_(state)                                     # the warm-up and the capture's eager run advanced the map: put the first frame's back
    g.color.copy_(cstate)
    for f in range(1, len(S.POSES)):
        for dst, src in zip(frame, frame_dev(name, f)):
            dst.copy_(src)
        sV.copy_(views[f])
        graph.replay()
        torch.cuda.synchronize()
        assert snapshot(g, *out) == want[f], f


def test_write_ply_round_trips_the_colours_and_the_default_is_unchanged(tmp_path):
    name = "direct_48x64"
    v = final_volume(name)
    sp = v.surface_points(max_jump=S2.JUMP)
    v.surface_colors(sp)
    parts = sp.split()
    counts = v.write_ply(str(tmp_path / "rgb_{}.ply"), colors=True, max_jump=S2.JUMP)
    assert counts == [p["points"].shape[0] for p in parts]
    for b in range(S.B):
        raw = (tmp_path / f"rgb_{b}.ply").read_bytes()
        head, body = raw.split(b"end_header\n", 1)
        assert f"element vertex {counts[b]}".encode() in head and b"property float nz" in head and b"property uchar blue" in head
        rec = np.frombuffer(body, np.dtype([("xyz", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)]))
        assert rec.size == counts[b] and rec["xyz"].tobytes() == parts[b]["points"].cpu().numpy().tobytes()
        want = np.clip(np.rint(np.nan_to_num(parts[b]["colors"].cpu().numpy().astype(np.float64), nan=0.0) * 255.0), 0, 255).astype(np.uint8)
        assert np.array_equal(rec["rgb"], want) and want.std() > 10 and rec["rgb"].min() >= 20      # the texture spans 0.1 .. 0.9
    # the default call: what it always wrote, byte for byte
    v.write_ply(str(tmp_path / "plain_{}.ply"), max_jump=S2.JUMP)
    v.write_ply(str(tmp_path / "off_{}.ply"), colors=False, max_jump=S2.JUMP)
    for b in range(S.B):
        pointcloud.write_ply(str(tmp_path / "want.ply"), parts[b]["points"], parts[b]["normals"])
        assert (tmp_path / f"plain_{b}.ply").read_bytes() == (tmp_path / "want.ply").read_bytes() == (tmp_path / f"off_{b}.ply").read_bytes()
    # a point without a colour is written black
    v.color.zero_()
    v.write_ply(str(tmp_path / "black_{}.ply"), colors=True, max_jump=S2.JUMP)
    body = (tmp_path / "black_0.ply").read_bytes().split(b"end_header\n", 1)[1]
    assert not np.frombuffer(body, np.dtype([("xyz", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)]))["rgb"].any()
    plain = TS.TsdfVolume(S.DIMS, S.VOXEL, S.ORIGIN, dev(np.array(S.K_GRID, np.float32)), size=S.GRID, trunc=S.TRUNC)
    plain.integrate(*plain_frame(name))
    with pytest.raises(ValueError, match="nothing was coloured yet"):
        plain.write_ply(str(tmp_path / "none_{}.ply"), colors=True)
    with pytest.raises(ValueError, match="nothing was coloured yet"):
        plain.shade(torch.ones(S.B, 4, 4, device=DEV))


def plain_frame(name):
    return plain(frame_dev(name, 0))


def test_tracker_update_rgb_equals_the_raw_calls_and_update_gives_the_same_poses():
    fr = I.track_frames()
    H, W = I.GRID
    rng = np.random.default_rng(4100)
    imgs = [dev(rng.normal(0.0, 1.0, (I.B, 3, H, W)).astype(np.float32)) for _ in fr]

    def volume():
        return TS.TsdfVolume(I.TRACK_DIMS, I.TRACK_VOXEL, I.TRACK_ORIGIN, dev(np.array(I.K_GRID, np.float32)), size=I.GRID, trunc=I.TRACK_TRUNC,
                             hi=I.TRACK_HI)

    t = TR.Tracker(volume(), pose_dev(fr[0][2]), iters=I.TRACK_ITERS)
    u = TR.Tracker(volume(), pose_dev(fr[0][2]), iters=I.TRACK_ITERS)
    poses, stats = [], []
    for f, (pred, std, _) in enumerate(fr):
        p, s = t.update_rgb(dev(pred), imgs[f], dev(std), mean=C.MEAN, std=C.CSTD)
        q, _ = u.update(dev(pred), dev(std))
        assert bits(p) == bits(q), f                                                  # tracking does not look at the image
        poses.append(p.clone())
        stats.append(None if s is None else s.clone())
    assert stats[0] is None and bits(t.volume.volume) == bits(u.volume.volume) and u.volume.color is None
    assert t.volume.color_counts.cpu().numpy()[:, 3].min() > 1000
    v = volume()
    last = pose_dev(fr[0][2])
    v.integrate_rgb(dev(fr[0][0]), imgs[0], dev(fr[0][1]), last, C.MEAN, C.CSTD)
    for f in range(1, I.TRACK_FRAMES):
        pred, std = dev(fr[f][0]), dev(fr[f][1])
        d, s, n = v.raycast(last, normals=True)
        r = TR.icp(pred, v.camera, d, n, None, std, s, None, v.grid_size, iters=I.TRACK_ITERS, lo=v.lo, hi=v.hi, std_floor=v.std_floor,
                   z_near=v.z_near, ref_pose=last)
        last = r.world.clone()
        v.integrate_rgb(pred, imgs[f], std, last, C.MEAN, C.CSTD)
        assert bits(last) == bits(poses[f]) and bits(r.stats) == bits(stats[f]), f
    assert bits(v.volume) == bits(t.volume.volume) and bits(v.color) == bits(t.volume.color) and bits(v.color_counts) == bits(t.volume.color_counts)
    # integrate=False tracks and leaves both volumes; a bad image is refused before the frame is tracked
    before = (bits(t.volume.volume), bits(t.volume.color), bits(t.pose))
    t.update_rgb(dev(fr[1][0]), imgs[1], dev(fr[1][1]), integrate=False, mean=C.MEAN, std=C.CSTD)
    assert (bits(t.volume.volume), bits(t.volume.color)) == before[:2]
    pose = bits(t.pose)
    with pytest.raises(ValueError, match="rgb must be"):
        t.update_rgb(dev(fr[2][0]), imgs[2][:, :2], dev(fr[2][1]))
    assert bits(t.pose) == pose
