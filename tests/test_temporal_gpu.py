"""`temporal.TemporalFilter` on the GPU -- the first frame, the closed-form variance recursion of a constant scene, a step change beyond
the gate, an `update` captured in a graph and replayed on new inputs -- and the `--robust_frames` switch of evaluate_all.py.

Tolerances: the variance recursion is compared in float64 with the closed form, every step of the float32 kernel adding at most a few
units of 2^-24 relative (four roundings per step: the sum, the product, the quotient, the process term): 8 * steps * 2^-24.  Everything
else is bitwise."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import pointcloud_ref as P
import reproject_ref as R

pytestmark = pytest.mark.gpu

from cfpnet_amd import hip, metrics, temporal as TP  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = (40.0, 41.5, 25.3, 17.9)
h, w, H, W = 19, 27, 37, 53


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)             # a copy: the shared inputs are read-only


def frames(n, B=2, seed=11, sigma=0.01):
    """n frames of one scene: (pred [B,h,w], unc [B,3,h,w]) float32, the scene times a little noise; plane 0 of unc is the std."""
    pred0 = np.clip(np.nan_to_num(R.reproject_inputs("odd_19x27_to_37x53")[0][:B], nan=1.5, posinf=R.HI, neginf=R.LO), 0.5, 5.0)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        pred = (pred0 * (1 + rng.normal(0, sigma, pred0.shape))).astype(np.float32)
        unc = np.stack([(0.03 + 0.04 * rng.random(pred0.shape)), rng.random(pred0.shape), rng.random(pred0.shape)], 1).astype(np.float32)
        out.append((pred, unc))
    return out


def bits(t):
    return t.cpu().numpy().tobytes()


def test_first_call_adopts_the_frame():
    (pred, unc), = frames(1)
    pred[1, 3:5, 4:7] = np.nan
    f = TP.TemporalFilter(K, size=(H, W))
    depth, std = f.update(dev(pred), dev(unc))
    assert depth.shape == (2, H, W) and std.shape == (2, H, W) and depth.data_ptr() == f.depth.data_ptr()
    for b in range(2):
        want_d = P.depth(pred[b], H, W, 1)
        want_s = np.maximum(P.plane_to_grid(unc[b, 0], H, W), np.float32(1e-3))
        R.close(depth[b].cpu().numpy(), want_d, f"first frame depth {b}")
        hole = np.isnan(want_d)
        assert (hole.sum() > 0) == (b == 1) and np.isinf(std[b].cpu().numpy()[hole]).all()      # nothing known: (NaN, +inf)
        R.close(std[b].cpu().numpy(), np.where(hole, np.float32(np.inf), want_s), f"first frame std {b}")
    assert f.counts.cpu().tolist() == [[0, 0, 0, 0]] * 2 and f.stats.cpu().tolist() == [[0.0, 0.0]] * 2
    # the same through the model's half-resolution prediction given as [B,1,h,w] and a plain std map
    g = TP.TemporalFilter(K, size=(H, W))
    d2, s2 = g.update(dev(pred)[:, None], dev(unc[:, 0]))
    assert bits(d2) == bits(depth) and bits(s2) == bits(std)
    # reset: the next frame is adopted again, the buffers stay
    ptr = f.depth.data_ptr()
    f.reset()
    d3, _ = f.update(dev(pred), dev(unc))
    assert d3.data_ptr() == ptr and bits(d3) == bits(d2) and f.counts.cpu().tolist() == [[0, 0, 0, 0]] * 2


@pytest.mark.parametrize("splat", [1, 2])
def test_constant_scene_follows_the_closed_form_recursion(splat):
    """Identity pose, the same frame every time: nothing is rejected, the depth stays, and 1 / var_n = 1 / (var_{n-1} + q) + 1 / vc."""
    (pred, unc), = frames(1)
    q, steps = 0.02, 6
    f = TP.TemporalFilter(K, size=(H, W), process_sigma=q, splat=splat)
    p, u = dev(pred), dev(unc)
    depth0 = f.update(p, u)[0].clone()
    vc = f.var.cpu().numpy().astype(np.float64)
    var = vc.copy()
    for n in range(1, steps + 1):
        # no pose: the state is the prior.  An identity pose goes through the warp, which is the identity map for splat 1 only (with
        # splat 2 a pixel is also offered its neighbours' depths and the nearest wins)
        depth, std = f.update(p, u, pose=np.eye(4)[:3] if splat == 1 and n % 2 == 0 else None)
        var = 1.0 / (1.0 / (var + np.float64(np.float32(q * q))) + 1.0 / vc)
        got = f.var.cpu().numpy().astype(np.float64)
        rel = np.abs(got - var) / var
        print(f"splat {splat} step {n}: worst relative distance of var from the closed form {rel.max():.3e} (bound {8 * n * 2.0 ** -24:.3e})")
        assert rel.max() <= 8 * n * 2.0 ** -24
        assert f.counts.cpu().tolist() == [[H * W, H * W, 0, 0]] * 2                 # every pixel has a prior and fuses
        assert f.stats.cpu().tolist() == [[0.0, 0.0]] * 2                             # identity pose: the prior is the state, bit for bit
        assert bits(depth) == bits(depth0)                                            # c + w * 0
        assert bits(std) == bits(torch.sqrt(f.var))


def test_a_step_change_beyond_the_gate_is_rejected_everywhere():
    (pred, unc), = frames(1)
    f = TP.TemporalFilter(K, size=(H, W))
    f.update(dev(pred), dev(unc))
    moved = (pred + np.float32(1.5)).astype(np.float32)                               # the gate is 3 * sqrt(2 * 0.07^2 + 4e-4) + 0.05 < 0.36 m
    fresh = TP.TemporalFilter(K, size=(H, W))
    want_d, want_s = fresh.update(dev(moved), dev(unc))
    depth, std = f.update(dev(moved), dev(unc))
    assert f.counts.cpu().tolist() == [[H * W, 0, H * W, 0]] * 2
    assert bits(depth) == bits(want_d) and bits(std) == bits(want_s)                  # the output is the new frame
    stats = f.stats.cpu().numpy()
    assert (np.abs(stats[:, 0] / (H * W) - 1.5) < 1e-2).all() and (np.abs(np.sqrt(stats[:, 1] / (H * W)) - 1.5) < 1e-2).all()


def test_update_moves_with_the_camera():
    """A sideways translation of the camera: the state follows (reproject), pixels the warp leaves uncovered are adopted, not fused."""
    (pred, unc), = frames(1)
    f = TP.TemporalFilter(K, size=(H, W), splat=2)
    f.update(dev(pred), dev(unc))
    T = dev(np.array([[1, 0, 0, 0.2, 0, 1, 0, 0, 0, 0, 1, 0]] * 2, np.float32).reshape(2, 3, 4))
    warped, _, wvar = TP.reproject(f.depth.clone(), K, T, size=(H, W), lo=-np.inf, hi=np.inf, splat=2, plane=f.var.clone())
    want = TP.fuse(dev(pred), dev(unc), warped, wvar, lo=R.LO, hi=R.HI)
    depth, std = f.update(dev(pred), dev(unc), pose=T)
    assert bits(depth) == bits(want[0]) and bits(f.var) == bits(want[1]) and bits(f.counts) == bits(want[2]) and bits(f.stats) == bits(want[3])
    counts = f.counts.cpu().numpy()
    assert (counts[:, 0] < H * W).all() and (counts[:, 0] > 0.5 * H * W).all() and (counts[:, 3] == 0).all()
    assert not torch.isnan(depth).any()


def test_update_under_graph_capture():
    """One captured `update` replayed on new inputs and a new pose equals the eager calls bit for bit."""
    seq = frames(4, seed=21)
    poses = [np.array([[1, 0, 0, 0.01 * k, 0, 1, 0, -0.005 * k, 0, 0, 1, 0.002 * k]] * 2, np.float32).reshape(2, 3, 4) for k in range(4)]
    eager = TP.TemporalFilter(K, size=(H, W))
    want = []
    for (pred, unc), T in zip(seq, poses):
        d, s = eager.update(dev(pred), dev(unc), pose=dev(T))
        want.append((bits(d), bits(s), bits(eager.counts), bits(eager.stats)))
    g = TP.TemporalFilter(K, size=(H, W))
    sp, su, sT = dev(seq[0][0]).clone(), dev(seq[0][1]).clone(), dev(poses[0]).clone()
    d, s = g.update(sp, su, pose=sT)                      # the first frame eagerly: it allocates and adopts
    assert (bits(d), bits(s)) == want[0][:2]
    state = (g.depth.clone(), g.var.clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # warm-up on the side stream, as capture asks for
        g.update(sp, su, pose=sT)
    torch.cuda.current_stream().wait_stream(side)
    g.depth.copy_(state[0]); g.var.copy_(state[1])        # the warm-up advanced the state: put the first frame's back
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gd, gs = g.update(sp, su, pose=sT)
    g.depth.copy_(state[0]); g.var.copy_(state[1])
    for k in range(1, 4):
        sp.copy_(dev(seq[k][0])); su.copy_(dev(seq[k][1])); sT.copy_(dev(poses[k]))
        graph.replay()
        torch.cuda.synchronize()
        assert (bits(gd), bits(gs), bits(g.counts), bits(g.stats)) == want[k], k


# ---- the command line ----------------------------------------------------------------------------------------------------------------------

BASE = ["@configs/cfpnet_combine1.txt", "--selected_epoch", "best", "--synthetic", "2", "--batch", "2"]


def _cli(argv):
    import evaluate_all
    out, err = io.StringIO(), io.StringIO()
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
            res = evaluate_all.main(list(argv))
    finally:
        os.chdir(cwd)
    return res, out.getvalue().splitlines(), err.getvalue().splitlines()


def test_cli_robust_frames(tmp_path, monkeypatch):
    plain, lines0, _ = _cli(BASE + ["--robust_sigma", "0.05", "--save_dir", str(tmp_path / "a")])
    updates, evals = [], []
    real_filter, real_eval = TP.TemporalFilter, metrics.eval_metrics

    class Recording(real_filter):
        def update(self, pred, unc, pose=None):
            updates.append((pred.clone(), unc.clone(), pose))
            return super().update(pred, unc, pose)

    def recording_eval(pred, gt, *a, **kw):
        evals.append((pred.clone(), gt.clone(), a, kw))
        return real_eval(pred, gt, *a, **kw)

    monkeypatch.setattr(TP, "TemporalFilter", Recording)
    monkeypatch.setattr(metrics, "eval_metrics", recording_eval)
    res, lines, _ = _cli(BASE + ["--robust_sigma", "0.05", "--robust_frames", "3", "--save_dir", str(tmp_path / "b")])
    monkeypatch.undo()
    assert res == plain and lines[:2] == lines0[:2] and len(lines) == len(lines0) == 3          # the Metrics lines do not change
    assert lines0[2].startswith("Robustness: ") and lines[2].startswith("Robustness: ")
    r0, r1 = json.loads(lines0[2][len("Robustness: "):]), json.loads(lines[2][len("Robustness: "):])
    assert "fused" not in r0 and r1["drop"] == r0["drop"] == {} and r1["sigma"] == r0["sigma"] and list(r1) == ["drop", "sigma", "fused"]
    fused = r1["fused"]
    assert fused["frames"] == 3 and fused["drop"] == {} and list(fused["sigma"]) == ["0.05"] and list(fused["sigma"]["0.05"]) == list(metrics.KEYS)
    full = json.load(open(os.path.join(str(tmp_path / "b"), "robustness.json")))
    assert full["fused"] == fused and "fused" not in json.load(open(os.path.join(str(tmp_path / "a"), "robustness.json")))
    # what TemporalFilter gives when called directly on the recorded model outputs
    assert len(updates) == 3 and all(p.shape == (2, 1, 240, 320) or p.shape == (2, 240, 320) for p, _, _ in updates)
    assert all(u.shape == (2, 3, 240, 320) and pose is None for _, u, pose in updates)
    assert bits(updates[0][0]) != bits(updates[1][0]) != bits(updates[2][0])                    # three draws of the degradation
    full_res = [(p, g) for p, g, _, _ in evals if p.shape[-2:] == (480, 640)]
    assert len(full_res) == 1 and len(evals) == 3                                               # plain, degraded, fused
    assert bits(evals[1][0]) == bits(updates[0][0])                                             # frame 0 is the draw of the Robustness entry
    f = real_filter(P.ZJUL5, size=(480, 640), lo=1e-3, hi=10.0)
    for p, u, _ in updates:
        depth, _ = f.update(p, u)
    assert bits(depth) == bits(full_res[0][0])
    avg = metrics.RunningAverageDict()
    avg.update(real_eval(depth, full_res[0][1], 1e-3, 10.0, mode=metrics.EVALUATE_ALL))
    assert {k: round(v, 3) for k, v in avg.get_value().items()} == fused["sigma"]["0.05"]
    print(f"sigma 0.05: one frame {r1['sigma']['0.05']}, three fused {fused['sigma']['0.05']}")
