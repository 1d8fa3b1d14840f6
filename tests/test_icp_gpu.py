"""`cfp_icp_step` through `tracking.icp` / `tracking.Tracker` on the GPU against the numpy restatement (`icp_ref.py`).

The pairing is exact against the float64 restatement outside the excluded set fixed on the CPU (test_icp_abi.py: at most 1 % of the
stride grid per case and image, and numpy's float32 agrees with float64 on everything else).  The sums are compared with the float32
restatement evaluated on the GPU's own pairing, each within the project's 2e-5 of the sum of the absolute values of its terms (the
float32-vs-float64 gap of the restatement is below half of that: test_icp_abi.py); the count is exact.  One step's pose and world pose
against the restatement's step from the same pose and the GPU's sums, within 1e-6 per entry (twice the gap measured on the CPU is
below that).  Behaviour: two calls give identical bits, a captured `icp` and a captured `Tracker.update` replay bit for bit, a scene that
does not constrain the pose is refused, and the poses converge like the float64 restatement's."""
import numpy as np
import pytest
import torch

import icp_ref as I
import pointcloud_ref as P

pytestmark = pytest.mark.gpu

from cfpnet_amd import tracking as TR, tsdf as TS  # noqa: E402

DEV = "cuda:0"
ROT_MARGIN, TRANS_MARGIN = 0.02, 2e-4                 # degrees, metres: what the convergence bounds add to twice the restatement's error


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)      # a copy: the shared inputs are read-only


def bits(t):
    return None if t is None else t.cpu().numpy().tobytes()


def pose_dev(T):
    return dev(np.asarray(T, np.float32).reshape(-1, 3, 4))


def all_bits(r):
    return tuple(bits(t) for t in r[:5])


def case_call(name, iters=1, index=True, ref=True, out=None, T=None, **over):
    """`icp` on the inputs of the case from its start pose."""
    c, x = I.ICP_CASES[name], I.inputs(name)
    kw = dict(I.case_kw(name))
    kw.update(over)
    return TR.icp(dev(x["pred"]), dev(x["K"]), dev(x["md"]), dev(x["mn"]), pose_dev(x["T"] if T is None else T), dev(x["std"]), dev(x["ms"]),
                  dev(x["Km"]), I.GRID, dev(x["nsrc"]), iters=iters, ref_pose=pose_dev(np.stack([I.T_REF] * I.B)) if ref else None,
                  index=index, out=out, **kw)


@pytest.fixture(scope="module")
def single_steps():
    """One step of every case, computed once and shared -- read-only."""
    out = {}
    for name in I.ICP_CASES:
        r = case_call(name)
        out[name] = {k: (None if t is None else t.cpu().numpy()) for k, t in r._asdict().items() if k != "ws"}
    return out


@pytest.mark.parametrize("name", list(I.ICP_CASES))
def test_association_against_the_float64_restatement(single_steps, name):
    got = single_steps[name]["index"]
    assert got.shape == (I.B,) + I.GRID and got.dtype == np.int32
    for b in range(I.B):
        d, ex = I.case_pairs(name, b, np.float64), I.case_excluded(name, b)
        differ = got[b] != d["index"]
        print(f"{name} image {b}: {int((got[b] >= 0).sum())} pairs, {int(differ.sum())} differ from the float64 restatement, "
              f"{int((differ & ~ex).sum())} outside the {int(ex.sum())} excluded pixels")
        assert not (differ & ~ex).any()
        assert (got[b][~d["on"]] == -1).all()                                         # off the stride grid: written, and -1


@pytest.mark.parametrize("name", list(I.ICP_CASES))
def test_sums_against_the_float32_restatement_on_the_gpus_own_pairs(single_steps, name):
    got = single_steps[name]
    assert got["sums"].shape == (I.B, 32) and got["sums"].dtype == np.float64 and (got["sums"][:, 30:] == 0).all()
    for b in range(I.B):
        want, scale = I.sums(I.pairs(*I.case_maps(name, b, np.float32), I.inputs(name)["T"][b], index=got["index"][b].astype(np.int64),
                                     **I.case_kw(name)))
        worst = float((np.abs(got["sums"][b, :30] - want) / np.maximum(scale, 1e-300)).max())
        print(f"{name} image {b}: {int(want[29])} pairs, worst |got - want| / (sum of |terms|) = {worst:.3e} (bound {I.RTOL:.1e})")
        assert got["sums"][b, 29] == want[29] == (got["index"][b] >= 0).sum()         # the count is exact
        assert (np.abs(got["sums"][b, :30] - want) <= I.RTOL * scale).all()
        st = got["stats"][0, b]
        assert st[0] == want[29] and abs(st[1] - want[28]) <= 1e-6 * want[28] and abs(st[2] - np.sqrt(want[27] / want[28])) <= 1e-5 * st[2]


@pytest.mark.parametrize("name", list(I.ICP_CASES))
def test_one_step_against_the_restatement(single_steps, name):
    got = single_steps[name]
    tol = 1e-6                                                                        # max(2 x the gap measured on the CPU (<= 5e-7 asserted there), 1e-6)
    for b in range(I.B):
        T0 = I.inputs(name)["T"][b]
        want, ok, xi = I.step(got["sums"][b, :30], T0)
        assert ok and got["stats"][0, b, 5] == 1.0
        T = got["pose"][b].ravel()
        worst = float(np.abs(T.astype(np.float64) - want).max())
        ww = float(np.abs(got["world"][b].ravel().astype(np.float64) - I.world(T, I.T_REF)).max())
        Rm = T.reshape(3, 4)[:, :3].astype(np.float64)
        print(f"{name} image {b}: worst |T' - want| = {worst:.3e}, |T_world - want| = {ww:.3e} (bound {tol:.1e}), |omega| {got['stats'][0, b, 3]:.4f}")
        assert worst <= tol and ww <= tol and np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-6
        assert abs(got["stats"][0, b, 3] - np.linalg.norm(xi[:3])) <= 1e-6 and abs(got["stats"][0, b, 4] - np.linalg.norm(xi[3:])) <= 1e-6
        assert not np.array_equal(T, T0)


def test_two_calls_give_identical_bits_and_out_is_written_in_place():
    name = "stride1_normals_std"
    a, b = case_call(name, iters=3), case_call(name, iters=3)
    assert all_bits(a) == all_bits(b) and a.stats.shape == (3, I.B, 6)
    c = case_call(name, iters=3, out=b)
    assert c.pose.data_ptr() == b.pose.data_ptr() and all_bits(c) == all_bits(a)
    with pytest.raises(ValueError, match="out stats"):
        case_call(name, iters=2, out=b)
    with pytest.raises(ValueError, match="out index"):
        case_call(name, iters=3, index=False, out=b)
    with pytest.raises(ValueError, match="IcpResult"):
        case_call(name, iters=3, out=tuple(b))


def test_icp_under_graph_capture():
    """A captured `icp` (10 iterations) replayed on a new frame and a new start pose equals the eager call bit for bit."""
    name, other = "stride1_normals_std", "stride2_std"
    x, y = I.inputs(name), I.inputs(other)
    kw = dict(I.case_kw(name), iters=10, index=True)
    K, md, mn, ms, ref = dev(x["K"]), dev(x["md"]), dev(x["mn"]), dev(x["ms"]), pose_dev(np.stack([I.T_REF] * I.B))
    nsrc_y = np.stack([P.normals(P.depth(y["pred"][b], *I.GRID, 0), I.K_GRID[b]) for b in range(I.B)])

    def eager(pred, std, nsrc, T):
        return all_bits(TR.icp(dev(pred), K, md, mn, pose_dev(T), dev(std), ms, None, I.GRID, dev(nsrc), ref_pose=ref, **kw))

    want = [eager(x["pred"], x["std"], x["nsrc"], x["T"]), eager(y["pred"], y["std"], nsrc_y, I.ID12.reshape(1, 12).repeat(I.B, 0))]
    assert want[0] != want[1]
    sp, su, sn, sT = dev(x["pred"]), dev(x["std"]), dev(x["nsrc"]), pose_dev(x["T"])

    def run(out=None):
        return TR.icp(sp, K, md, mn, sT, su, ms, None, I.GRID, sn, ref_pose=ref, out=out, **kw)

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
    for k, (pred, std, nsrc, T) in enumerate(((x["pred"], x["std"], x["nsrc"], x["T"]),
                                              (y["pred"], y["std"], nsrc_y, I.ID12.reshape(1, 12).repeat(I.B, 0)))):
        sp.copy_(dev(pred)); su.copy_(dev(std)); sn.copy_(dev(nsrc)); sT.copy_(pose_dev(T))
        graph.replay()
        torch.cuda.synchronize()
        assert all_bits(out) == want[k], k
    assert bits(sT) == pose_dev(I.ID12.reshape(1, 12).repeat(I.B, 0)).cpu().numpy().tobytes()      # the caller's start pose is not touched


def test_refusals():
    H, W = I.GRID
    x = I.inputs("stride1_plain")
    K, ref = dev(x["K"]), pose_dev(np.stack([I.T_REF] * I.B))
    # a fronto-parallel wall given directly as model maps: zero pivots
    wall_d = torch.full((I.B, H, W), 2.0, device=DEV)
    wall_n = torch.zeros(I.B, H, W, 3, device=DEV)
    wall_n[..., 2] = -1.0
    T0 = I.rot(0.01, -0.02, 0.005, (0.01, 0.02, -0.03)).astype(np.float32)
    r = TR.icp(torch.full((I.B, H, W), 2.05, device=DEV), K, wall_d, wall_n, pose_dev(np.stack([T0] * I.B)), size=I.GRID, iters=2, ref_pose=ref)
    st = r.stats.cpu().numpy()
    print("wall:", st[:, 0])
    assert (st[..., 5] == 0).all() and (st[..., 0] > 2000).all() and (st[..., 3:5] == 0).all() and np.isfinite(st[..., 2]).all()
    assert bits(r.pose) == np.stack([T0] * I.B).tobytes()                             # bitwise unchanged
    want = np.stack([I.world(T0, I.T_REF)] * I.B)
    assert np.abs(r.world.cpu().numpy().reshape(I.B, 12) - want).max() <= 1e-6        # T_world is still written
    # an image without a pair: the others still step
    md = dev(x["md"])
    md[1] = float("nan")
    r = TR.icp(dev(x["pred"]), K, md, dev(x["mn"]), pose_dev(x["T"]), size=I.GRID, iters=1)
    st, T = r.stats.cpu().numpy()[0], r.pose.cpu().numpy().reshape(I.B, 12)
    assert st[1, 0] == 0 and st[1, 5] == 0 and np.isnan(st[1, 2]) and T[1].tobytes() == x["T"][1].tobytes() and r.world is None
    assert (st[[0, 2], 5] == 1).all() and all(T[b].tobytes() != x["T"][b].tobytes() for b in (0, 2))
    assert (r.sums.cpu().numpy()[1] == 0).all()
    # min_pairs above the count
    r = TR.icp(dev(x["pred"]), K, dev(x["md"]), dev(x["mn"]), pose_dev(x["T"]), size=I.GRID, iters=1, min_pairs=H * W + 1)
    assert (r.stats.cpu().numpy()[0, :, 5] == 0).all() and bits(r.pose) == x["T"].tobytes()


@pytest.mark.parametrize("m", range(3))
def test_convergence_from_the_identity(m):
    x = I.converge_inputs(m)
    for stride in (1, 2):
        r = TR.icp(dev(x["pred"]), dev(x["K"]), dev(x["md"]), dev(x["mn"]), None, size=I.GRID, iters=12, stride=stride)
        T, st = r.pose.cpu().numpy().reshape(I.B, 12), r.stats.cpu().numpy()
        for b, (_, _, (deg0, tr0)) in enumerate(I.converge_reference(m, stride, 12)):
            deg, tr = I.pose_error(T[b], x["T_true"][b])
            print(f"motion {m} stride {stride} image {b}: error {deg:.4f} deg / {1e3 * tr:.3f} mm (float64 restatement {deg0:.4f} / "
                  f"{1e3 * tr0:.3f}), rms {st[0, b, 2]:.4f} -> {st[-1, b, 2]:.5f}")
            assert deg <= 2 * deg0 + ROT_MARGIN and tr <= 2 * tr0 + TRANS_MARGIN
            assert st[-1, b, 2] < st[0, b, 2] and st[:, b, 5].all()


# ---- Tracker -------------------------------------------------------------------------------------------------------------------------------

def make_tracker():
    v = TS.TsdfVolume(I.TRACK_DIMS, I.TRACK_VOXEL, I.TRACK_ORIGIN, dev(np.array(I.K_GRID, np.float32)), size=I.GRID, trunc=I.TRACK_TRUNC,
                      hi=I.TRACK_HI)
    return TR.Tracker(v, pose_dev(I.track_frames()[0][2]), iters=I.TRACK_ITERS)


def test_tracker_against_raw_calls_the_cpu_chain_and_capture():
    fr = I.track_frames()
    ref = I.track_reference()
    depth, normal, which = ref["first"]
    assert all((~np.isnan(normal).any(-1) & (which == k)).sum() > 100 for k in range(4))      # all three planes and the sphere in the model
    bound = 2 * ref["errors"] + np.array([ROT_MARGIN, TRANS_MARGIN])
    assert (bound[..., 0] < 0.5).all() and (bound[..., 1] < 0.5 * I.TRACK_VOXEL).all()        # or the comparison shows nothing
    # the Tracker
    t = make_tracker()
    poses, stats = [], []
    for f, (pred, std, _) in enumerate(fr):
        p, s = t.update(dev(pred), dev(std))
        poses.append(p.clone())
        stats.append(None if s is None else s.clone())
    assert stats[0] is None and bits(poses[0]) == fr[0][2].tobytes() and all(s.shape == (I.TRACK_ITERS, I.B, 6) for s in stats[1:])
    volume = bits(t.volume.volume)
    # the same sequence of raw calls by hand
    v = TS.TsdfVolume(I.TRACK_DIMS, I.TRACK_VOXEL, I.TRACK_ORIGIN, dev(np.array(I.K_GRID, np.float32)), size=I.GRID, trunc=I.TRACK_TRUNC,
                      hi=I.TRACK_HI)
    last = pose_dev(fr[0][2])
    v.integrate(dev(fr[0][0]), dev(fr[0][1]), last)
    for f in range(1, I.TRACK_FRAMES):
        pred, std = dev(fr[f][0]), dev(fr[f][1])
        d, s, n = v.raycast(last, normals=True)
        r = TR.icp(pred, v.camera, d, n, None, std, s, None, v.grid_size, iters=I.TRACK_ITERS, lo=v.lo, hi=v.hi, std_floor=v.std_floor,
                   z_near=v.z_near, ref_pose=last)
        last = r.world.clone()
        v.integrate(pred, std, last)
        assert bits(last) == bits(poses[f]) and bits(r.stats) == bits(stats[f]), f
    assert bits(v.volume) == volume
    # against the CPU chain
    for f in range(1, I.TRACK_FRAMES):
        got = poses[f].cpu().numpy().reshape(I.B, 12)
        for b in range(I.B):
            deg, tr = I.pose_error(got[b], I.track_pose(f, b))
            print(f"frame {f} image {b}: error {deg:.4f} deg / {1e3 * tr:.3f} mm (CPU chain {ref['errors'][f, b, 0]:.4f} / "
                  f"{1e3 * ref['errors'][f, b, 1]:.3f}; bound {bound[f, b, 0]:.4f} / {1e3 * bound[f, b, 1]:.3f})")
            assert deg <= bound[f, b, 0] and tr <= bound[f, b, 1]
        assert stats[f].cpu().numpy()[-1, :, 5].all()
    # track stores nothing; integrate=False leaves the volume
    g = make_tracker()
    sp, su = dev(fr[0][0]), dev(fr[0][1])
    g.update(sp, su)
    sp.copy_(dev(fr[1][0])); su.copy_(dev(fr[1][1]))
    before = (bits(g.pose), bits(g.volume.volume))
    assert bits(g.track(sp, su)) == bits(poses[1]) and (bits(g.pose), bits(g.volume.volume)) == before
    p, _ = g.update(sp, su, integrate=False)
    assert bits(p) == bits(poses[1]) and bits(g.volume.volume) == before[1]
    g.pose.copy_(pose_dev(fr[0][2]))
    # a captured update replayed on the frames equals the eager calls
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    state = g.volume.volume.clone()
    with torch.cuda.stream(side):                             # warm-up on the side stream, as capture asks for
        g.update(sp, su)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = g.update(sp, su)
    g.volume.volume.copy_(state)                              # the warm-up advanced the volume and the pose: put the first frame's back
    g.pose.copy_(pose_dev(fr[0][2]))
    for f in range(1, I.TRACK_FRAMES):
        sp.copy_(dev(fr[f][0])); su.copy_(dev(fr[f][1]))
        graph.replay()
        torch.cuda.synchronize()
        assert bits(out[0]) == bits(poses[f]) and bits(out[1]) == bits(stats[f]), f
    assert bits(g.volume.volume) == volume
