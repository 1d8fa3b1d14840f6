"""`cfp_tsdf_integrate` / `cfp_tsdf_raycast` through `tsdf.TsdfVolume` on the GPU against the numpy restatement (`tsdf_ref.py`).

Discrete results -- which voxels an integration updates, which pixel each reads, at which step a ray hits -- are exact against the
float64 restatement outside the excluded set fixed on the CPU (test_tsdf_abi.py: at most 1 % of a case, and numpy's float32 agrees with
float64 on everything else).  Every integration step starts from the float32 restatement's state for that frame, so nothing carries
over.  Values against the float32 restatement: Wt, depth and std within the project's 2e-5 * max(|want|, 1e-3); F, a normalised
quantity in [-1, 1] with cancellation around 0, within 2e-5 absolute; normals within twice the worst float32-vs-float64 angle of the
restatement over these cases (measured here, recorded in tsdf_ref.py), against the float64 normal.  Behaviour: two runs give identical
bits, a captured integrate + raycast replays bit for bit, and the raycast depth goes straight into `pointcloud.point_cloud`."""
import numpy as np
import pytest
import torch

import pointcloud_ref as P
import tsdf_ref as S

pytestmark = pytest.mark.gpu

from cfpnet_amd import pointcloud, tsdf as TS  # noqa: E402

DEV = "cuda:0"
INF = float("inf")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)             # a copy: the shared inputs are read-only


def bits(t):
    return t.cpu().numpy().tobytes()


def pose_dev(T):
    return dev(np.asarray(T, np.float32).reshape(-1, 3, 4))


def frame_dev(name, f):
    pred, std, T = S.frames(name)[f]
    return dev(pred), (None if std is None else dev(std)), pose_dev(T)


def make_volume(name, state=None):
    """A TsdfVolume of the case with its buffers allocated (by a first integrate) and `state` (all empty by default) uploaded."""
    c = S.TSDF_CASES[name]
    v = TS.TsdfVolume(S.DIMS, S.VOXEL, c["origin"], dev(np.array(S.K_GRID, np.float32)), size=S.GRID, trunc=S.TRUNC, w_max=c["w_max"])
    v.integrate(*frame_dev(name, 0))
    if state is None:
        v.reset()
    else:
        v.volume.copy_(dev(state))
    return v


@pytest.mark.parametrize("name", ["blend_24x32", "direct_48x64", "no_std", "w_max_binds"])
def test_integrate_against_the_restatement(name):
    v = make_volume(name)
    assert v.volume.shape == (S.B, S.DIMS[2], S.DIMS[1], S.DIMS[0], 2) and bits(v.volume) == np.stack([S.empty_volume(S.DIMS)] * S.B).tobytes()
    for f in range(len(S.POSES)):
        before = S.states(name)[f]
        v.volume.copy_(dev(before))
        counts = v.integrate(*frame_dev(name, f))
        got, n = v.volume.cpu().numpy(), counts.cpu().numpy()
        assert counts.shape == (S.B, 3) and counts.dtype == torch.int32
        for b in range(S.B):
            a, d, ex = S.step_reference(name, f, b), S.step_reference(name, f, b, np.float64), S.step_excluded(name, f, b)
            keep = ~ex
            changed = (got[b] != before[b]).any(-1)
            visible = (a["vol"] != before[b]).any(-1)                                  # an update that leaves both numbers as they were cannot be seen
            assert np.array_equal(changed[keep], (d["updated"] & visible)[keep]), (name, f, b)
            assert not (changed & ~d["seen"] & keep).any()                            # a skipped voxel is not written
            low, room = S.counts_of(d, keep), int(ex.sum())
            print(f"{name} frame {f} image {b}: counts {n[b].tolist()}, float64 outside the excluded set {low}, {room} voxels excluded")
            assert all(lo <= int(g) <= lo + room for g, lo in zip(n[b], low)), (n[b], low, room)
            assert n[b][0] == n[b][1] + n[b][2]
            S.close(got[b][..., 1], a["vol"][..., 1], f"{name} frame {f} image {b} Wt", keep)
            S.close_abs(got[b][..., 0], a["vol"][..., 0], S.F_ATOL, f"{name} frame {f} image {b} F", keep)
    if name == "w_max_binds":
        assert (got[..., 1] == 900.0).sum() > 1000 and got[..., 1].max() == 900.0


def test_integrate_reads_the_pixel_the_float64_restatement_names():
    """A std plane on the grid itself whose value at pixel p is 1 / sqrt(p + 1) makes the weight of a voxel of an empty volume p + 1,
    to a part in a million: the pixel each voxel reads, observed."""
    name, H, W = "blend_24x32", *S.GRID
    v = make_volume(name)
    pred, _, T = frame_dev(name, 0)
    ids = (1.0 / np.sqrt(np.arange(H * W, dtype=np.float64) + 1.0)).astype(np.float32).reshape(1, H, W)
    v.integrate(pred, dev(np.repeat(ids, S.B, 0)), T)
    wt = v.volume[..., 1].cpu().numpy().astype(np.float64)
    for b in range(S.B):
        d, ex = S.step_reference(name, 0, b, np.float64), S.step_excluded(name, 0, b)
        keep = ~ex                                                                    # the std does not enter the exclusion: u, v and sdf only
        assert np.array_equal((wt[b] > 0)[keep], d["updated"][keep])
        sel = d["updated"] & keep
        pix = np.rint(wt[b][sel]) - 1
        assert np.abs(wt[b][sel] - np.rint(wt[b][sel])).max() < 0.01 and np.array_equal(pix.astype(np.int64), d["pix"][sel])
        print(f"image {b}: {int(sel.sum())} voxels read {np.unique(pix).size} different pixels, all the float64 restatement's")


def test_a_volume_outside_the_view_is_not_touched():
    name = "outside_the_view"
    state = S.states("blend_24x32")[-1]                                               # something worth keeping
    v = make_volume(name, state)
    for f in range(len(S.POSES)):
        counts = v.integrate(*frame_dev(name, f))
        assert counts.cpu().tolist() == [[0, 0, 0]] * S.B and bits(v.volume) == state.tobytes()


@pytest.mark.parametrize("name", list(S.RAYCAST_CASES))
def test_raycast_against_the_restatement(name):
    c = S.RAYCAST_CASES[name]
    v = make_volume(c["case"], S.states(c["case"])[-1])
    K = dev(np.array(c["K"], np.float32))
    depth, std, normal = v.raycast(pose_dev(c["T"]), K, (c["Hd"], c["Wd"]), c["t_range"], c["step"])
    assert depth.shape == (S.B, c["Hd"], c["Wd"]) and std.shape == depth.shape and normal.shape == depth.shape + (3,)
    first = (bits(depth), bits(std), bits(normal))
    depth_only, std_only = v.raycast(pose_dev(c["T"]), K, (c["Hd"], c["Wd"]), c["t_range"], c["step"], normals=False)
    again = v.raycast(pose_dev(c["T"]), K, (c["Hd"], c["Wd"]), c["t_range"], c["step"])
    assert tuple(bits(t) for t in again) == first and (bits(depth_only), bits(std_only)) == first[:2]      # two runs, with and without normals
    gd, gs, gn = depth.cpu().numpy(), std.cpu().numpy(), normal.cpu().numpy()
    tol = 2.0 * S.normal_angle_measured()
    for b in range(S.B):
        a, d, ex = S.raycast_reference(name, b), S.raycast_reference(name, b, np.float64), S.raycast_excluded(name, b)
        keep = ~ex
        assert np.array_equal(S.hit_step_of(gd[b], c["t_range"][0], c["step"])[keep], d["hit"][keep]), (name, b)
        S.close(gd[b], a["depth"], f"{name} image {b} depth", keep)
        S.close(gs[b], a["std"], f"{name} image {b} std", keep)
        nan = np.isnan(gn[b]).any(-1)
        assert np.array_equal(nan[keep], np.isnan(a["normal"]).any(-1)[keep]) and np.array_equal(nan, np.isnan(gn[b]).all(-1))
        ok = ~nan & ~np.isnan(d["normal"]).any(-1) & keep
        worst = float(P.angle(gn[b][ok], d["normal"][ok]).max())
        length = float(np.abs(np.linalg.norm(gn[b][ok].astype(np.float64), axis=-1) - 1.0).max())
        print(f"{name} image {b}: {int(ok.sum())} normals, worst angle to the float64 restatement {worst:.3e} rad (tolerance {tol:.3e}), "
              f"worst | |n| - 1 | = {length:.3e}")
        assert ok.sum() > 50 and worst <= tol and length <= 4 * 2.0 ** -23
    # `out`: the tuple of an earlier call
    other = tuple(torch.empty_like(t) for t in again)
    res = v.raycast(pose_dev(c["T"]), K, (c["Hd"], c["Wd"]), c["t_range"], c["step"], out=other)
    assert res[0].data_ptr() == other[0].data_ptr() and tuple(bits(t) for t in other) == first
    with pytest.raises(ValueError, match="out depth"):
        v.raycast(size=(c["Hd"], c["Wd"]), out=(other[1][:, :-1], other[1], other[2]))


def test_two_integrations_give_identical_bits():
    name = "blend_24x32"
    res = []
    for _ in range(2):
        v = make_volume(name, S.states(name)[1])
        counts = v.integrate(*frame_dev(name, 1))
        res.append((bits(v.volume), bits(counts)))
    assert res[0] == res[1]


def test_raycast_depth_goes_straight_into_point_cloud():
    c = S.RAYCAST_CASES["blend_to_37x53"]
    v = make_volume(c["case"], S.states(c["case"])[-1])
    K = dev(np.array(c["K"], np.float32))
    Hd, Wd = c["Hd"], c["Wd"]
    depth, _, _ = v.raycast(pose_dev(c["T"]), K, (Hd, Wd), c["t_range"], c["step"])
    pc = pointcloud.point_cloud(depth, K, size=(Hd, Wd), lo=-INF, hi=INF)
    gd = depth.cpu().numpy()
    for b, part in enumerate(pc.split()):
        hits = np.flatnonzero(~np.isnan(gd[b].ravel()))
        assert np.array_equal(part["index"].cpu().numpy(), hits) and hits.size > 100                  # every hit and nothing else, in pixel order
        assert part["points"][:, 2].cpu().numpy().tobytes() == gd[b].ravel()[hits].tobytes()          # z is the raycast depth, bit for bit


def test_integrate_and_raycast_under_graph_capture():
    """One captured integrate + raycast replayed on new inputs, a new camera pose and a new view equals the eager calls bit for bit."""
    name, rc = "blend_24x32", S.RAYCAST_CASES["blend_to_37x53"]
    K = dev(np.array(rc["K"], np.float32))
    size = (rc["Hd"], rc["Wd"])
    views = [pose_dev(S.POSE_VIEW), pose_dev(S.POSES[1]), pose_dev(S.POSES[0])]

    def snapshot(v, out):
        return (bits(v.volume), bits(v.counts)) + tuple(bits(t) for t in out)

    eager = make_volume(name)
    want = []
    for f in range(len(S.POSES)):
        eager.integrate(*frame_dev(name, f))
        want.append(snapshot(eager, eager.raycast(views[f], K, size, rc["t_range"], rc["step"])))
    g = make_volume(name)
    sp, su, sT = (t.clone() for t in frame_dev(name, 0))
    sV = views[0].clone()

    def step():
        g.integrate(sp, su, sT)
        return g.raycast(sV, K, size, rc["t_range"], rc["step"])

    assert snapshot(g, step()) == want[0]                     # the first frame eagerly: every buffer exists afterwards
    state = g.volume.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                             # warm-up on the side stream, as capture asks for
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    g.volume.copy_(state)                                     # the warm-up advanced the volume: put the first frame's back
    for f in range(1, len(S.POSES)):
        pred, std, T = frame_dev(name, f)
        sp.copy_(pred); su.copy_(std); sT.copy_(T); sV.copy_(views[f])
        graph.replay()
        torch.cuda.synchronize()
        assert snapshot(g, out) == want[f], f
