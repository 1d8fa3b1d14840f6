"""The restatement of the zone-consistency loss (`zone_loss_ref.py`) checked against itself, without a GPU: its analytic gradient
against central differences of its own loss with run and weights frozen, a perfect prediction against its own measurement, and the
reason for the weights."""
import numpy as np
import pytest

import zone_consistency_ref as ZR
import zone_loss_ref as R


def test_the_gather_blend_is_the_metrics_depth():
    """`blend64` (the float32 tap weights, float64 arithmetic) against the float32 depth of the metric on every case: the same non-finite
    pixels, and within the four float32 roundings of the blend elsewhere."""
    for name in R.CASES:
        c = R.CASES[name]
        pred = R.inputs(name)[0]
        d32 = R.depth(name, pred)
        for b in range(len(pred)):
            p = np.clip(pred[b], np.float32(c["lo"]), np.float32(c["hi"])).astype(np.float64)
            d64 = R.blend64(p, c["H"], c["W"], c["interp"])
            ok = np.isfinite(d32[b])
            assert np.array_equal(ok, np.isfinite(d64))
            assert np.abs(d64[ok] - d32[b][ok]).max() <= 4 * 2.0 ** -24 * np.abs(d64[ok]).max()


@pytest.mark.parametrize("name,floor", R.RUNS)
def test_analytic_gradient_equals_central_differences(name, floor):
    """Up to 240 elements of `pred` per case, among them every kind the case has.  Elements within the step of a clip bound sit on the
    kink of the clip and are left out; non-finite elements have gradient 0 by definition and no difference quotient."""
    a = R.run_args(name, floor)
    ref = R.loss(**a, exact_blend=True)                  # the difference quotients are taken where the float64 blend puts the zone means
    pred, B = a["pred"], a["pred"].shape[0]
    h = 1e-4
    rng = np.random.default_rng(3)
    worst, checked, nonzero = 0.0, 0, 0
    for b in range(B):
        p0 = pred[b].astype(np.float64)
        flat = np.flatnonzero(np.isfinite(p0) & (np.abs(p0 - np.float32(a["lo"])) > 2 * h) & (np.abs(p0 - np.float32(a["hi"])) > 2 * h))
        hot = np.intersect1d(flat, np.flatnonzero(ref["grad"][b] != 0))
        pick = np.concatenate([rng.permutation(hot)[:160], rng.permutation(flat)[:80]])
        f = lambda q: R.frozen_loss_image(q, ref["frozen"][b], B, a["H"], a["W"], a["interp"], a["lo"], a["hi"])
        for i in pick:
            y, x = divmod(int(i), p0.shape[1])
            qp, qm = p0.copy(), p0.copy()
            qp[y, x] += h
            qm[y, x] -= h
            fd = (f(qp) - f(qm)) / (2 * h)
            g = ref["grad"][b, y, x]
            worst = max(worst, abs(fd - g))
            checked += 1
            nonzero += g != 0
        assert not ref["grad"][b][~np.isfinite(p0)].any()
    scale = max(float(np.abs(ref["grad"]).max()), 1e-3)
    print(f"{name} floor {floor}: {checked} elements ({nonzero} with a gradient), worst |fd - analytic| {worst:.3e}, largest gradient {scale:.3e}")
    # the frozen loss is piecewise quadratic in one element, so inside a piece the central difference has no truncation error at any
    # step; what is left is the rounding of the two evaluations: a zone mean is a pairwise float64 sum of at most 4096 products of size
    # <= hi (relative error <= (log2(4096) + 2) * 2^-53), the slope of the loss in a zone mean is <= 1, and the quotient divides by 2 h
    assert worst <= 16 * 2.0 ** -53 * a["hi"] / h + 1e-9 * scale
    assert np.isfinite(ref["grad"]).all() and np.isfinite(ref["out"]).all()


def test_the_table_reaches_every_branch_of_the_definition():
    """Dead zone, quadratic and linear residuals, images with n_b = 0, a partial selection in every compared zone, and more zones than
    a chunk of the backward: what the GPU test relies on the cases to hold."""
    e = np.concatenate([R.reference(n)["e"][np.isfinite(R.reference(n)["zone"][..., R.R])].ravel() for n in R.CASES])
    assert (e == 0).any() and ((e > 0) & (e <= R.BIN_WIDTH)).any() and (e > R.BIN_WIDTH).any()
    nb0 = sum(int((np.isfinite(R.reference(n)["zone"][b, :, R.R]).sum() == 0)) for n in R.CASES for b in range(len(R.inputs(n)[0])))
    assert nb0 >= 2
    many = R.reference("many_zones_260")
    assert many["zone"].shape[1] == 260 and (many["zone"][0, 256:, R.COEF] != 0).any() and (many["zone"][0, :256, R.COEF] != 0).any()
    assert np.isnan(many["zone"][0, 7, R.R]) and many["zone"][0, 7, R.STATE] == ZR.UNMEASURED
    for name, floor in R.RUNS:
        ref = R.reference(name, floor)
        assert ref["out"][0] == ref["out"][1:].sum() / (len(ref["out"]) - 1)
        assert (ref["terms_abs"] >= np.abs(ref["grad"]) * (1 - 1e-12)).all()


@pytest.mark.parametrize("name", list(R.CASES))
def test_a_perfect_prediction_has_no_loss_at_any_floor(name):
    """Each image's prediction against its own simulated (mu, sigma): e_z <= n_pix * 2^-52 * max_d per zone, so L is 0 to rounding."""
    npix = R.n_pix(name)
    for floor in R.FLOORS:
        a = R.run_args(name, floor)
        a["mask"], a["raw"] = R.self_measurement(name, floor)
        got = R.loss(**a)
        bound = npix * 2.0 ** -52 * a["max_d"]
        print(f"{name} floor {floor}: compared {int(np.isfinite(got['zone'][..., R.R]).sum())}, worst e_z {got['e'].max():.3e}, L {got['out'][0]:.3e}")
        assert (got["e"] <= bound).all(), (name, floor, got["e"].max())
        assert got["out"][0] <= (bound.max() ** 2) / (2 * R.BIN_WIDTH)
        if got["e"].max() == 0:
            assert not got["grad"].any()


def test_the_unweighted_mean_fails_at_floor_20():
    """The mean of the run's pixels without the weights c'_j / cnt_j leaves the dead zone on a perfect prediction: the weights are not
    an ornament.  (At floor 0 every weight is 1 and the two agree.)"""
    worst = {True: 0.0, False: 0.0}
    for name in R.CASES:
        a = R.run_args(name, 20)
        a["mask"], a["raw"] = R.self_measurement(name, 20)
        for weighted in (True, False):
            worst[weighted] = max(worst[weighted], float(R.loss(**a, weighted=weighted)["e"].max()))
        a0 = R.run_args(name, 0)
        a0["mask"], a0["raw"] = R.self_measurement(name, 0)
        assert np.array_equal(R.loss(**a0, weighted=False)["zone"][..., R.M], R.loss(**a0)["zone"][..., R.M])
    print(f"floor 20, perfect prediction: worst e_z weighted {worst[True]:.3e}, unweighted {worst[False]:.3e}")
    assert worst[True] <= 4096 * 2.0 ** -52 * 40.96 and worst[False] > 1e-3
