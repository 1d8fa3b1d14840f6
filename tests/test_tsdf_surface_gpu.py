"""`cfp_tsdf_surface` through `tsdf.TsdfVolume.surface_points` on the GPU against the numpy restatement (`tsdf_surface_ref.py`).

Nothing is excluded: counts and index lists are `torch.equal` to the float32 restatement, the NaN-normal rows are identical, points and
std lie within the project's 2e-5 * max(|want|, 1e-3) of the float32 restatement and normals within 2e-5 rad -- that relative bound
applied to a unit vector -- of the float64 one (the restatement alone stays more than 20 x inside it on these inputs,
test_tsdf_surface_abi.py; a wrong neighbour moves a normal by degrees).  Behaviour: a capacity below the count keeps the first rows bit
for bit and leaves the others alone, two runs give identical bits, a captured integrate + surface_points replays bit for bit, the
normals agree in orientation with the raycast's, and `write_ply` hands the vertices over."""
import numpy as np
import pytest
import torch

import tsdf_ref as S
import tsdf_surface_ref as Q

pytestmark = pytest.mark.gpu

from cfpnet_amd import tsdf as TS  # noqa: E402
from test_tsdf_gpu import DEV, bits, dev, frame_dev, make_volume, pose_dev  # noqa: E402

INF = float("inf")


def random_volume_dev(dims):
    """A TsdfVolume of `dims` with its buffers allocated (by a first integrate of a tiny frame) and the random volume uploaded."""
    vol = Q.random_volume(dims)
    B = vol.shape[0]
    v = TS.TsdfVolume(dims, Q.RANDOM_VOXEL, Q.RANDOM_ORIGIN, (4.0, 4.0, 2.0, 2.0), size=(4, 4))
    v.integrate(torch.ones(B, 4, 4, device=DEV))
    v.volume.copy_(dev(vol))
    return v


def volume_of(name):
    if name in Q.STATE_CASES:
        return make_volume(name, S.states(name)[-1])
    return random_volume_dev(tuple(int(d) for d in name.split("_")[1].split("x")))


def check(res, name, w_min=0.0, max_jump=INF, normals=True):
    """Everything `res` holds against the restatement with the same options; returns the per-image counts."""
    vol = Q.inputs()[name][0]
    B = vol.shape[0]
    want = [Q.reference(name, b, w_min, max_jump) for b in range(B)]
    n = [int(r["index"].size) for r in want]
    assert res.counts.dtype == torch.int32 and res.index.dtype == torch.int32
    assert torch.equal(res.counts.cpu(), torch.tensor(n, dtype=torch.int32)), (name, res.counts.tolist(), n)
    assert res.capacity >= max(n) and res.points.shape == (B, res.capacity, 3) and res.std.shape == (B, res.capacity)
    assert (res.normals is not None) == normals
    for b, part in enumerate(res.split()):
        a, d = want[b], Q.reference(name, b, w_min, max_jump, np.float64)
        assert torch.equal(part["index"].cpu(), torch.from_numpy(a["index"].astype(np.int32))), (name, b)
        what = f"{name} image {b} ({n[b]} points)"
        Q.close(part["points"].cpu().numpy(), a["points"], what + " points")
        Q.close(part["std"].cpu().numpy(), a["std"], what + " std")
        if normals:
            gn = part["normals"].cpu().numpy()
            nan = np.isnan(gn).any(-1)
            assert np.array_equal(nan, np.isnan(a["normals"]).any(-1)) and np.array_equal(nan, np.isnan(gn).all(-1)), (name, b)
            if (~nan).any():
                worst = float(Q.angle(gn[~nan], d["normals"][~nan]).max())
                length = float(np.abs(np.linalg.norm(gn[~nan].astype(np.float64), axis=-1) - 1.0).max())
                print(f"{what}: {int((~nan).sum())} normals, worst angle to the float64 restatement {worst:.3e} rad (bound {Q.ANGLE_TOL:.1e}), "
                      f"worst | |n| - 1 | = {length:.3e}")
                assert worst <= Q.ANGLE_TOL and length <= 4 * 2.0 ** -23
    return n


@pytest.mark.parametrize("name", list(Q.inputs()))
def test_surface_against_the_restatement(name):
    v = volume_of(name)
    res = v.surface_points()
    n = check(res, name)
    assert res.capacity == max(max(n), 1)                                             # capacity=None allocates exactly the largest count
    assert torch.equal(v.surface_count(), res.counts)
    again = v.surface_points()                                                        # two runs: identical bits
    plain = v.surface_points(normals=False)
    assert plain.normals is None
    for b, (p0, p1, p2) in enumerate(zip(res.split(), again.split(), plain.split())):
        for key in ("points", "std", "index"):
            assert bits(p0[key]) == bits(p1[key]) == bits(p2[key]), (name, b, key)
        assert bits(p0["normals"]) == bits(p1["normals"])


@pytest.mark.parametrize("name", ["random_130x5x3", "random_67x33x31"])
def test_w_min_that_binds(name):
    v = volume_of(name)
    n = check(v.surface_points(w_min=Q.W_MIN_BINDS), name, Q.W_MIN_BINDS)
    assert torch.equal(v.surface_count(w_min=Q.W_MIN_BINDS).cpu(), torch.tensor(n, dtype=torch.int32))
    both = check(v.surface_points(w_min=Q.W_MIN_BINDS, max_jump=0.5), name, Q.W_MIN_BINDS, 0.5)
    assert all(0 < b < a for a, b in zip(n, both))


@pytest.mark.parametrize("name", list(Q.STATE_CASES))
def test_max_jump_that_binds(name):
    v = volume_of(name)
    n = check(v.surface_points(max_jump=Q.JUMP), name, 0.0, Q.JUMP)
    assert torch.equal(v.surface_count(max_jump=Q.JUMP).cpu(), torch.tensor(n, dtype=torch.int32))


def _sentinel(B, cap, normals=True):
    return TS.SurfacePoints(torch.full((B, cap, 3), -7.0, device=DEV), torch.full((B, cap, 3), -7.0, device=DEV) if normals else None,
                            torch.full((B, cap), -7.0, device=DEV), torch.full((B, cap), -7, dtype=torch.int32, device=DEV),
                            torch.full((B,), -7, dtype=torch.int32, device=DEV), cap)


@pytest.mark.parametrize("name", ["direct_48x64", "random_67x33x31"])
def test_a_capacity_below_the_count(name):
    v = volume_of(name)
    full = v.surface_points()
    counts = full.counts.cpu().tolist()
    B = len(counts)
    for cap in (min(counts) - 7, 1):
        out = _sentinel(B, cap)
        res = v.surface_points(capacity=cap, out=out)
        assert res is out and res.counts.cpu().tolist() == counts                     # the true totals
        for key in ("points", "normals", "std", "index"):
            assert bits(getattr(res, key)) == bits(getattr(full, key)[:, :cap]), (name, cap, key)      # the first rows, bit for bit
        with pytest.raises(RuntimeError, match=r"overflow: \(image, kept\)"):
            res.split()
    # rows beyond the count are not written: a capacity above it, pre-filled with a sentinel
    cap = max(counts) + 5
    out = _sentinel(B, cap)
    res = v.surface_points(capacity=cap, out=out)
    for b, n in enumerate(counts):
        assert (res.points[b, n:] == -7).all() and (res.normals[b, n:] == -7).all() and (res.std[b, n:] == -7).all() and (res.index[b, n:] == -7).all()
        assert bits(res.points[b, :n]) == bits(full.points[b, :n]) and bits(res.index[b, :n]) == bits(full.index[b, :n])
    with pytest.raises(ValueError, match="out must be"):
        v.surface_points(capacity=cap + 1, out=out)
    with pytest.raises(ValueError, match="out must be"):
        v.surface_points(normals=False, out=out)
    with pytest.raises(ValueError, match="capacity must be at least 1"):
        v.surface_points(capacity=0)


def test_an_empty_volume_gives_nothing_and_writes_nothing():
    v = make_volume("direct_48x64")                                                   # reset: F = 1, Wt = 0
    assert v.surface_count().cpu().tolist() == [0] * S.B
    res = v.surface_points()
    assert res.capacity == 1 and res.counts.cpu().tolist() == [0] * S.B and all(p["points"].shape == (0, 3) for p in res.split())
    out = _sentinel(S.B, 5)
    v.surface_points(out=out)
    assert out.counts.cpu().tolist() == [0] * S.B
    for t in (out.points, out.normals, out.std, out.index):
        assert (t == -7).all()
    for bad in (dict(w_min=-1.0), dict(w_min=float("nan")), dict(max_jump=-0.5)):
        with pytest.raises(ValueError, match="must not be negative"):
            v.surface_points(**bad)


def test_integrate_and_surface_points_under_graph_capture():
    """One captured integrate + surface_points(capacity=..., out=...) replayed on new frames equals the eager calls bit for bit."""
    name, cap = "blend_24x32", 2048

    def snapshot(v, r):
        return (bits(v.volume), bits(r.counts)) + tuple(bits(t[b, :n]) for b, n in enumerate(r.counts.cpu().tolist())
                                                        for t in (r.points, r.normals, r.std, r.index))

    eager = make_volume(name)
    want = []
    for f in range(len(S.POSES)):
        eager.integrate(*frame_dev(name, f))
        want.append(snapshot(eager, eager.surface_points(capacity=cap)))
    assert want[0] != want[1] != want[2]
    g = make_volume(name)
    sp, su, sT = (t.clone() for t in frame_dev(name, 0))
    out = g.surface_points(capacity=cap)                                              # every buffer exists before the capture

    def step():
        g.integrate(sp, su, sT)
        return g.surface_points(capacity=cap, out=out)

    assert step() is out and snapshot(g, out) == want[0]
    state = g.volume.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                             # warm-up on the side stream, as capture asks for
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    g.volume.copy_(state)                                     # the warm-up advanced the volume: put the first frame's back
    for f in range(1, len(S.POSES)):
        pred, std, T = frame_dev(name, f)
        sp.copy_(pred); su.copy_(std); sT.copy_(T)
        graph.replay()
        torch.cuda.synchronize()
        assert snapshot(g, out) == want[f], f


def test_normals_are_oriented_like_the_raycast():
    """R times an extracted normal is what the raycast writes at the same place: for every raycast hit with a normal, the nearest
    extracted point within a voxel that has one -- the cosine of the two stays above 0.9.  The convention, not a value."""
    c = S.RAYCAST_CASES["direct_to_37x53"]
    v = make_volume(c["case"], S.states(c["case"])[-1])
    K = dev(np.array(c["K"], np.float32))
    depth, _, normal = v.raycast(pose_dev(c["T"]), K, (c["Hd"], c["Wd"]), c["t_range"], c["step"])
    parts = v.surface_points().split()
    for b in range(S.B):
        cos, n = matched_cosines(depth[b].cpu().numpy(), normal[b].cpu().numpy(), c["K"][b], c["T"][b], parts[b]["points"].cpu().numpy(),
                                 parts[b]["normals"].cpu().numpy())
        print(f"image {b}: {n} raycast hits matched to an extracted point within a voxel, cosines {cos.min():.4f} .. {cos.max():.4f}")
        assert n > 300 and cos.min() > 0.9


def matched_cosines(depth, normal, K, T, pts, nrm):
    fx, fy, cx, cy = K
    M = np.asarray(T, np.float64).reshape(3, 4)
    Rm, t = M[:, :3], M[:, 3]
    ys, xs = np.nonzero(~np.isnan(depth) & ~np.isnan(normal).any(-1))
    z = depth[ys, xs].astype(np.float64)
    pc = np.stack([(xs - cx) / fx * z, (ys - cy) / fy * z, z], -1)
    pw = (pc - t) @ Rm                                                                # R^T (Pc - t)
    have = ~np.isnan(nrm).any(-1)
    d = np.linalg.norm(pw[:, None, :] - pts[have][None, :, :].astype(np.float64), axis=-1)
    near = d.argmin(1)
    ok = d[np.arange(d.shape[0]), near] < S.VOXEL
    rotated = nrm[have][near[ok]].astype(np.float64) @ Rm.T                           # R n_w
    return (rotated * normal[ys, xs][ok]).sum(-1), int(ok.sum())


def test_write_ply_hands_the_vertices_over(tmp_path):
    v = make_volume("direct_48x64", S.states("direct_48x64")[-1])
    counts = v.write_ply(str(tmp_path / "map_{}.ply"), max_jump=Q.JUMP)
    want = [Q.reference("direct_48x64", b, 0.0, Q.JUMP)["index"].size for b in range(S.B)]
    assert counts == want
    raw = (tmp_path / "map_1.ply").read_bytes()
    head, body = raw.split(b"end_header\n", 1)
    assert f"element vertex {want[1]}".encode() in head and b"property float nz" in head and len(body) == want[1] * 24
    xyz = np.frombuffer(body, "<f4").reshape(-1, 6)[:, :3]
    assert xyz.tobytes() == v.surface_points(max_jump=Q.JUMP).split()[1]["points"].cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="same file"):
        v.write_ply(str(tmp_path / "map.ply"))
