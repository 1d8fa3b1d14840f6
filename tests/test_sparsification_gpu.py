"""`cfp_unc_sparsification` on the GPU against the numpy restatement of its definition (`sparsification_ref.py`, itself checked in
test_sparsification_abi.py).

Tolerances
  exact cases (nothing interpolated): 1e-9 relative.  The kernel's sums are exact integer accumulations rounded once; the reference's are
      float64 sums of at most 3.1e5 terms, within ~3e-11 relative of that in any order; the rest is a handful of float64 operations.
      A curve point is compared relative to itself.  AUSE and AURG are differences of two means of curve points over e0, so they carry
      1e-9 of what is subtracted: |delta| <= 1e-9 * (mean_k a + mean_k b) / e0 for the difference mean_k (a - b) / e0 (for a score that
      equals its oracle, or a constant plane, the value itself is ~0 and no bound relative to the value could hold).
  interpolated protocol: a last-bit difference in an interpolated score or prediction can move a pixel across a boundary, so the bound is
      measured, from the reference alone, on the very inputs of each case: the largest relative difference between reference runs that
      differ only in how the bilinear blend is rounded (float32 op by op in the kernel's order / float64 rounded once / ATen's order);
      allowed is 4x that spread with a floor of 2e-5 (the RTOL of test_metrics.py).  Measured spreads, K = 20: (24,32)->(48,64)
      mode 0 1.0e-06 / mode 1 8.5e-07; (23,31)->(47,61) mode 0 7.3e-07 / mode 1 4.3e-07, so the floor is the bound in force there.
      At (240,320)->(480,640) a synthetic pair with white-noise planes gave 7.2e-05 (a pixel changes sides at one boundary: bound
      2.9e-04); the end-to-end test measures the spread of the engine's own tensors and prints it."""
import io
import contextlib
import os

import numpy as np
import pytest
import torch

import sparsification_ref as R

pytestmark = pytest.mark.gpu

from cfpnet_amd import metrics, synthetic  # noqa: E402

DEV = "cuda:0"
LO, HI = 1e-3, 10.0
RTOL_EXACT = 1e-9
RTOL_FLOOR = 2e-5
KS = (1, 7, 20, 100)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------

def make_case(B, H, W, kind, seed):
    """gt [B,H,W], pred [B,H,W], unc [B,3,H,W] float32.  Errors of at least 1 cm on every valid pixel, so e0 is well away from 0."""
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.5, 9.0, (B, H, W)).astype(np.float32)
    pred = (gt + rng.choice([-1.0, 1.0], gt.shape) * rng.uniform(0.01, 0.8, gt.shape)).astype(np.float32)
    holes = 0.3 if kind == "holes" else 0.02
    gt[rng.random(gt.shape) < holes] = 0.0
    gt[rng.random(gt.shape) < 0.01] = 11.0                                   # beyond hi: invalid too
    unc = np.stack([rng.uniform(0.0, 2.0, gt.shape), rng.uniform(0.0, 5.5, gt.shape), rng.uniform(0.0, 1.0, gt.shape)], 1).astype(np.float32)
    if kind == "tied":
        levels = np.array([0.0, 0.125, 0.25, 0.3, 0.5, 0.75, 0.9, 1.0], np.float32)
        unc = levels[rng.integers(0, 8, unc.shape)]
    elif kind == "constant":
        unc[:, 0] = np.float32(0.25)
        unc[:, 2] = np.float32(1.0)
    elif kind == "special":
        for p, vals in enumerate(([-0.0, 0.0, np.inf, np.nan], [-0.0, np.nan, -1.5, 0.0], [np.inf, -np.inf, np.nan, 1.0])):
            pick = rng.integers(0, 8, gt.shape)
            for i, v in enumerate(vals):
                unc[:, p][pick == i] = np.float32(v)
    return gt, pred, unc


def gpu(pred, unc, gt, K, mode=metrics.EVALUATE_ALL, lo=LO, hi=HI):
    r = metrics.sparsification(torch.from_numpy(pred).to(DEV), torch.from_numpy(unc).to(DEV), torch.from_numpy(gt).to(DEV), lo, hi, steps=K,
                               mode=mode)
    return {k: r[k].cpu().numpy() for k in ("curves", "ause", "aurg", "n_valid")}


def compare(got, want, b, rtol, what):
    """Image b of a batched result against one reference dict (bounds: module docstring).  Prints the largest figures before asserting."""
    c, w = got["curves"][b], want["curves"]
    assert got["n_valid"][b] == want["n_valid"], (what, got["n_valid"][b], want["n_valid"])
    assert np.array_equal(np.isnan(c), np.isnan(w)), what
    fin = ~np.isnan(w)
    worst = float((np.abs(c[fin] - w[fin]) / np.abs(w[fin])).max()) if fin.any() else 0.0
    worst_s = 0.0
    for u in range(3):
        for m in range(2):
            e0 = w[3 + m, m, 0]
            for name, scale in (("ause", (w[u, m].mean() + w[3 + m, m].mean()) / e0), ("aurg", (e0 + w[u, m].mean()) / e0)):
                g, x = got[name][b, u, m], want[name][u, m]
                assert np.isnan(g) == np.isnan(x), (what, name, u, m, g, x)
                if not np.isnan(x):
                    worst_s = max(worst_s, abs(g - x) / scale)
    print(f"{what}: curves rel {worst:.3e}, summary rel-to-operands {worst_s:.3e} (bound {rtol:.1e})")
    assert worst <= rtol and worst_s <= rtol, (what, worst, worst_s)
    return max(worst, worst_s)


# ---- 1. exact cases --------------------------------------------------------------------------------------------------------------------

SHAPES = [(1, 8, 8), (2, 37, 53), (3, 120, 160), (1, 480, 640)]
KINDS = ["continuous", "tied", "constant", "special", "holes"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_cases(shape, kind):
    B, H, W = shape
    gt, pred, unc = make_case(B, H, W, kind, seed=H * 7 + len(kind))
    for K in KS:
        got = gpu(pred, unc, gt, K)
        assert got["curves"].shape == (B, 5, 2, K) and got["ause"].shape == (B, 3, 2) and got["aurg"].shape == (B, 3, 2)
        for b in range(B):
            compare(got, R.image_equal_size(pred[b], unc[b], gt[b], LO, HI, K), b, RTOL_EXACT, f"{kind} {shape} K={K} image {b}")


# ---- 2. closed forms through the kernel ------------------------------------------------------------------------------------------------

def test_closed_forms():
    B, H, W, K = 2, 37, 53, 20
    gt, pred, unc = make_case(B, H, W, "continuous", seed=21)
    v = np.clip(pred, np.float32(LO), np.float32(HI))
    d = gt - v
    t0 = d * d
    # score 0 = the oracle score: the same curve bit for bit, AUSE exactly 0
    unc[:, 0] = t0
    unc[:, 1] = np.float32(0.7)                                               # a constant plane
    got = gpu(pred, unc, gt, K)
    assert np.array_equal(got["curves"][:, 0], got["curves"][:, 3])
    assert (got["ause"][:, 0, 0] == 0.0).all()
    e0 = got["curves"][:, 3:4, :, :1]                                         # [B,1,2,1]
    assert np.array_equal(got["curves"][:, :, :, :1], np.broadcast_to(e0, (B, 5, 2, 1)))     # k = 0 keeps all: one value in all rankings
    flat = got["curves"][:, 1]
    assert (np.abs(flat - e0[:, 0]) <= 1e-12 * e0[:, 0]).all() and (np.abs(got["aurg"][:, 1]) <= 1e-12).all()
    assert (got["ause"] >= 0).all() and (np.diff(got["curves"][:, 3, 0], axis=-1) <= 0).all()
    # the negated oracle removes the best pixels first
    unc[:, 0] = -t0
    assert (gpu(pred, unc, gt, K)["aurg"][:, 0, 0] < 0).all()
    # the same d at every pixel: every curve is flat
    gt2 = np.full((1, H, W), 2.0, np.float32)
    gt2[0, :3] = 0.0
    got = gpu(gt2 + np.float32(0.5), unc[:1], gt2, K)
    assert got["n_valid"][0] == (H - 3) * W
    assert (np.abs(got["curves"] - got["curves"][..., :1]) <= 1e-12).all()
    assert np.abs(got["curves"][0, :, 0] - 0.5).max() <= 1e-12 and np.abs(got["curves"][0, :, 1] - 0.25).max() <= 1e-12
    # no error at all: e0 == 0 -> NaN, n_valid tells
    got = gpu(gt2.copy(), unc[:1], gt2, K)
    assert np.isnan(got["curves"]).all() and np.isnan(got["ause"]).all() and np.isnan(got["aurg"]).all() and got["n_valid"][0] == (H - 3) * W


# ---- 3. batch behaviour ----------------------------------------------------------------------------------------------------------------

def test_batch_rows_empty_image_repeatability_and_masked_pixels():
    B, H, W, K = 8, 60, 80, 20
    gt, pred, unc = make_case(B, H, W, "holes", seed=33)
    gt[5] = 0.0                                                               # no valid pixel
    gt[2] = 0.0
    gt[2, 17, 43] = 3.0                                                       # a single valid pixel
    P, U, G = torch.from_numpy(pred).to(DEV), torch.from_numpy(unc).to(DEV), torch.from_numpy(gt).to(DEV)
    first = metrics.sparsification(P, U, G, LO, HI, steps=K)
    again = metrics.sparsification(P, U, G, LO, HI, steps=K)
    torch.cuda.synchronize()
    for k in ("curves", "ause", "aurg", "n_valid"):
        assert first[k].dtype == torch.float64 and first[k].is_cuda
        a, b = first[k].cpu().numpy(), again[k].cpu().numpy()
        assert np.array_equal(a, b, equal_nan=True), k
    keep = torch.tensor([b for b in range(B) if b != 5], device=DEV)
    assert torch.equal(first["curves"][keep], again["curves"][keep]) and torch.equal(first["summary"][keep], again["summary"][keep])
    got = {k: first[k].cpu().numpy() for k in ("curves", "ause", "aurg", "n_valid")}
    assert got["n_valid"][5] == 0 and np.isnan(got["curves"][5]).all() and np.isnan(got["ause"][5]).all() and np.isnan(got["aurg"][5]).all()
    assert got["n_valid"][2] == 1 and not np.isnan(got["curves"][2]).any()
    assert np.abs(got["curves"][2] - got["curves"][2][:, :, :1]).max() == 0    # one pixel: n_k = 1 at every k
    for b in range(B):                                                        # rows equal the per-image calls bit for bit
        one = metrics.sparsification(P[b:b + 1], U[b:b + 1], G[b:b + 1], LO, HI, steps=K)
        for k in ("curves", "ause", "aurg", "n_valid"):
            assert np.array_equal(one[k][0].cpu().numpy(), got[k][b], equal_nan=True), (b, k)
        compare(got, R.image_equal_size(pred[b], unc[b], gt[b], LO, HI, K), b, RTOL_EXACT, f"batch image {b}")
    # pixels outside lo < gt < hi influence nothing
    invalid = ~np.logical_and(gt > LO, gt < HI)
    pred2, unc2 = pred.copy(), unc.copy()
    pred2[invalid] = np.float32(123.0)
    pred2[invalid & (np.arange(W) % 2 == 0)] = np.nan
    unc2[np.broadcast_to(invalid[:, None], unc.shape)] = np.float32(-7.0)
    other = gpu(pred2, unc2, gt, K)
    for k in ("curves", "ause", "aurg", "n_valid"):
        assert np.array_equal(other[k], got[k], equal_nan=True), k
    # the running mean skips the empty image
    run = metrics.RunningSparsification()
    run.update({k: v[:3] for k, v in first.items()})
    run.update({k: v[3:] for k, v in first.items()})
    val = run.get_value()
    rows = [b for b in range(B) if b != 5]
    names = [f"{a}_{m}_{p}" for a in ("ause", "aurg") for m in ("rmse", "absrel") for p in ("std", "entropy", "pmax")]
    assert sorted(names + ["curves"]) == sorted(val)
    for a in ("ause", "aurg"):
        for m, mn in enumerate(("rmse", "absrel")):
            for u, pn in enumerate(("std", "entropy", "pmax")):
                assert abs(val[f"{a}_{mn}_{pn}"] - got[a][rows, u, m].mean()) <= 1e-12
    assert np.abs(np.array(val["curves"]) - got["curves"][rows].mean(0)).max() <= 1e-12
    with pytest.raises(ValueError):
        metrics.sparsification(P, U[:, :2], G, LO, HI)
    with pytest.raises(ValueError):
        metrics.sparsification(P, U.half(), G, LO, HI)
    with pytest.raises(RuntimeError, match="steps"):
        metrics.sparsification(P, U, G, LO, HI, steps=101)


# ---- 4. interpolated protocol ----------------------------------------------------------------------------------------------------------

def reference_spread(pred, unc, gt, lo, hi, K, mode):
    """(the ATen-order reference, the largest relative difference between reference runs that differ only in the rounding of the blend)."""
    runs = {how: R.image_interpolated(pred, unc, gt, lo, hi, K, mode, how) for how in ("aten", "ours", "f64")}
    spread = 0.0
    for a, b in (("ours", "f64"), ("ours", "aten")):
        x, y = runs[a], runs[b]
        fin = ~np.isnan(y["curves"])
        spread = max(spread, float((np.abs(x["curves"][fin] - y["curves"][fin]) / np.abs(y["curves"][fin])).max()))
        w = y["curves"]
        for u in range(3):
            for m in range(2):
                e0 = w[3 + m, m, 0]
                spread = max(spread, abs(x["ause"][u, m] - y["ause"][u, m]) / ((w[u, m].mean() + w[3 + m, m].mean()) / e0),
                             abs(x["aurg"][u, m] - y["aurg"][u, m]) / ((e0 + w[u, m].mean()) / e0))
    return runs["aten"], spread


def interp_inputs(hp, wp, H, W, seed, nonfinite):
    gt, pred = synthetic.make_eval_pair(H, W, hp, wp, seed, 0.3, 0.2)
    if nonfinite:
        pred[hp // 2, wp // 3] = np.nan
        pred[1, 2] = -np.inf
    else:
        pred[~np.isfinite(pred)] = 37.5                                      # mode 0 clips before the blend; inf is clipped like 37.5
    rng = np.random.default_rng(seed + 5)
    unc = np.stack([rng.uniform(0.0, 2.0, (hp, wp)), rng.uniform(0.0, 5.5, (hp, wp)), rng.uniform(0.0, 1.0, (hp, wp))]).astype(np.float32)
    return gt, pred, unc


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("sizes", [((24, 32), (48, 64)), ((23, 31), (47, 61))], ids=["24x32-48x64", "23x31-47x61"])
def test_interpolated_protocol(sizes, mode):
    from oracle import metrics_oracle as MO
    (hp, wp), (H, W) = sizes
    K = 20
    gt, pred, unc = interp_inputs(hp, wp, H, W, 40 + hp, nonfinite=mode == 1)
    want, spread = reference_spread(pred, unc, gt, LO, HI, K, mode)
    # the reference's prediction is the protocol of oracle/metrics_oracle.py
    g, v = (MO.protocol_evaluate_all if mode == 0 else MO.protocol_validate)(pred.copy(), gt, LO, HI)
    valid = np.logical_and(gt > LO, gt < HI)
    assert np.array_equal(R.protocol_v(pred, H, W, LO, HI, mode, "aten")[valid], v) and np.array_equal(gt[valid], g)
    tol = max(4 * spread, RTOL_FLOOR)
    print(f"{sizes} mode {mode}: reference spread {spread:.3e} -> bound {tol:.3e}")
    got = gpu(pred[None], unc[None], gt[None], K, mode=mode)
    compare(got, want, 0, tol, f"interpolated {sizes} mode {mode}")


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------

def test_engine_tensors_against_the_reference():
    """The default numerics mode on the two-image 480x640 case of test_uncertainty_gpu.py: the API on the engine's tensors against the
    reference on the downloaded ones."""
    from cfpnet_amd import spec, weights
    from cfpnet_amd.engine import Engine
    layers = spec.COMBINE1_LAYERS
    sd = weights.make_torch_state_dict(spec.model_manifest(layers))
    inp = synthetic.make_inputs(2, 480, 640, 8, 56, seed=9, drop_hist=0.34)          # _full_case(2, 480, 640, 8, 56, 9, 0.34)
    eng = Engine(sd, layer_names=layers, device=DEV)
    _, pred, prob, unc = eng.forward(synthetic.to_device(inp, DEV), uncertainty=True, return_prob=False)
    assert prob is None and pred.shape == (2, 1, 240, 320) and unc.shape == (2, 3, 240, 320)
    gt = np.stack([synthetic.make_depth(480, 640, seed=60 + i, holes=0.2) for i in range(2)])
    K = 20
    res = metrics.sparsification(pred, unc, torch.from_numpy(gt).to(DEV), LO, HI, steps=K)
    got = {k: res[k].cpu().numpy() for k in ("curves", "ause", "aurg", "n_valid")}
    p, u = pred.cpu().numpy()[:, 0], unc.cpu().numpy()
    for b in range(2):
        want, spread = reference_spread(p[b], u[b], gt[b], LO, HI, K, 0)
        tol = max(4 * spread, RTOL_FLOOR)
        print(f"engine image {b}: reference spread {spread:.3e} -> bound {tol:.3e}; AUSE {got['ause'][b].tolist()} AURG {got['aurg'][b].tolist()}")
        compare(got, want, b, tol, f"engine image {b}")


def _cli(argv):
    import evaluate_all
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        res = evaluate_all.main(argv)
    return res, out.getvalue().splitlines()


def test_evaluate_all_cli(tmp_path):
    from cfpnet_amd import config, data
    from cfpnet_amd.deltar import make_model
    base = ["@configs/cfpnet_combine1.txt", "--selected_epoch", "best", "--synthetic", "8"]
    cwd = os.getcwd()
    os.chdir(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        plain, lines0 = _cli(list(base))
        flagged, lines1 = _cli(base + ["--unc_metrics", "--save_dir", str(tmp_path)])
        # the same pipeline by hand
        args = config.parse_args(list(base[:3]))
        model = make_model(args, dtype="f32x3").to(torch.device(DEV)).eval()
        build = data.EvalInputBuilder(args, torch.device(DEV))
        run = metrics.RunningSparsification()
        with torch.no_grad():
            for img, dep, _ in data.batches(data.SyntheticEvalSamples(8, 480, 640), 8):
                inp, gt = build(img, dep)
                _, pred, _, unc = model(inp, return_uncertainty=True, return_prob=False)
                run.update(metrics.sparsification(pred, unc, gt, float(args.min_depth), float(args.max_depth), steps=20))
        want = run.get_value()
    finally:
        os.chdir(cwd)
    assert flagged == plain and len(plain) == 9
    assert len(lines0) == 2 and len(lines1) == 3 and lines1[:2] == lines0 and lines1[2].startswith("Uncertainty: {")
    printed = eval(lines1[2][len("Uncertainty: "):], {"nan": float("nan")})
    assert len(printed) == 12 and list(printed) == [k for k in want if k != "curves"]
    for k, v in printed.items():
        assert v == round(want[k], 4), (k, v, want[k])
    import json
    saved = json.load(open(os.path.join(str(tmp_path), "sparsification.json")))
    assert saved["steps"] == 20 and np.array(saved["curves"]).shape == (5, 2, 20)
    assert np.array_equal(np.array(saved["curves"]), np.array(want["curves"]))
