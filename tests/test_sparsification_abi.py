"""`cfp_unc_sparsification` without a GPU: the symbols, the constants, the workspace query and the argument checks (no kernel is launched),
the `--unc_metrics` switch of evaluate_all.py, and the numpy reference of the definition (`sparsification_ref.py`) against independent
forms of it: a plain stable argsort, the mean over random tie-breaks, closed forms."""
import inspect
import os

import numpy as np
import pytest

import sparsification_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from cfpnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.load()


def test_symbols_and_constants(lib):
    from cfpnet_amd import hip, metrics
    assert hasattr(lib, "cfp_unc_sparsification") and hasattr(lib, "cfp_unc_sparsification_ws_bytes")
    text = open(os.path.join(ROOT, "include", "cfpnet_hip.h")).read()
    assert "enum { CFP_SPARS_STD = 0, CFP_SPARS_ENTROPY, CFP_SPARS_PMAX, CFP_SPARS_ORACLE_RMSE, CFP_SPARS_ORACLE_ABSREL };" in text
    assert (hip.SPARS_STD, hip.SPARS_ENTROPY, hip.SPARS_PMAX, hip.SPARS_ORACLE_RMSE, hip.SPARS_ORACLE_ABSREL) == (0, 1, 2, 3, 4)
    assert (hip.SPARS_STD, hip.SPARS_ENTROPY, hip.SPARS_PMAX) == (hip.UNC_STD, hip.UNC_ENTROPY, hip.UNC_PMAX)
    assert metrics.RANKINGS == R.RANKINGS and len(hip.SIGNATURES["cfp_unc_sparsification"][1]) == 19


def test_ws_bytes_monotone(lib):
    ws = lib.cfp_unc_sparsification_ws_bytes
    assert ws(1, 480, 640, 20) >= 5 * 480 * 640 * 4 and ws(1, 480, 640, 20) % 8 == 0 and ws(1, 3, 3, 1) % 8 == 0
    for a, b in zip(range(1, 9), range(2, 10)):
        assert ws(a, 37, 53, 20) < ws(b, 37, 53, 20)
    steps = [ws(2, 37, 53, k) for k in (1, 7, 20, 100)]
    assert steps == sorted(steps)
    assert ws(0, 8, 8, 20) == 0


def test_invalid_arguments_are_refused_with_a_message(lib):
    """16 = a non-null, 16-byte aligned dummy pointer; every case fails a check before anything is dereferenced or launched."""
    from cfpnet_amd import hip
    P, BIG = 16, 1 << 40
    EINVAL, ESHAPE = -1, -2

    def call(pred=P, unc=P, hp=8, wp=8, gt=P, h=8, w=8, b=1, interp=0, mode=0, lo=1e-3, hi=10.0, steps=20, ws=P, nbytes=BIG, curves=P,
             summary=P, nvalid=P):
        rc = lib.cfp_unc_sparsification(pred, unc, hp, wp, gt, h, w, b, interp, mode, lo, hi, steps, ws, nbytes, curves, summary, nvalid, 0)
        return rc, hip.last_error()

    for name in ("pred", "unc", "gt", "ws", "curves", "summary", "nvalid"):
        rc, msg = call(**{name: 0})
        assert rc == EINVAL and "cfp_unc_sparsification: null pointer" in msg, (name, rc, msg)
    for steps in (0, 101, -3):
        rc, msg = call(steps=steps)
        assert rc == EINVAL and "steps" in msg, (steps, rc, msg)
    rc, msg = call(hp=4, wp=4)
    assert rc == ESHAPE and "sizes differ" in msg
    rc, msg = call(b=0)
    assert rc == ESHAPE and "non-positive" in msg
    for lo, hi in ((2.0, 1.0), (1.0, 1.0)):
        rc, msg = call(lo=lo, hi=hi)
        assert rc == EINVAL and "empty depth range" in msg
    rc, msg = call(mode=2)
    assert rc == EINVAL and "mode" in msg
    rc, msg = call(nbytes=lib.cfp_unc_sparsification_ws_bytes(1, 8, 8, 20) - 1)
    assert rc == EINVAL and "workspace too small" in msg
    rc, msg = call(ws=20)
    assert rc == EINVAL and "8-byte aligned" in msg
    # the twin: cfp_eval_metrics answers the shared cases with the same codes
    assert lib.cfp_eval_metrics(P, 4, 4, P, 8, 8, 1, 0, 0, 1e-3, 10.0, P, BIG, P, 0) == ESHAPE
    assert lib.cfp_eval_metrics(P, 8, 8, P, 8, 8, 1, 0, 0, 2.0, 1.0, P, BIG, P, 0) == EINVAL
    with pytest.raises(RuntimeError, match="cfp_unc_sparsification failed"):
        hip.call("cfp_unc_sparsification", P, P, 8, 8, P, 8, 8, 1, 0, 0, 1e-3, 10.0, 0, P, BIG, P, P, P, 0)


def test_python_api_rejects_bad_unc_before_anything_runs():
    import torch
    from cfpnet_amd import metrics
    sig = inspect.signature(metrics.sparsification)
    assert list(sig.parameters) == ["pred", "unc", "gt", "lo", "hi", "steps", "mode", "out"] and sig.parameters["steps"].default == 20
    with pytest.raises(ValueError):
        metrics.sparsification(torch.ones(1, 4, 4), torch.ones(1, 3, 4, 4), torch.ones(1, 4, 4), 1e-3, 10.0)     # host tensors
    assert metrics.RunningSparsification().get_value() == {}


def test_evaluate_all_takes_the_switch_off_argv():
    import evaluate_all
    argv = ["--synthetic", "8", "--unc_metrics", "--unc_steps", "7", "--save_entropy"]
    assert evaluate_all._pop(argv, "--unc_metrics", False, None) is True
    assert evaluate_all._pop(argv, "--unc_steps", 20, int) == 7
    assert argv == ["--synthetic", "8", "--save_entropy"]
    assert evaluate_all._pop(argv, "--unc_metrics", False, None) is False and evaluate_all._pop(argv, "--unc_steps", 20, int) == 20
    src = inspect.getsource(evaluate_all.main)
    assert '_pop(argv, "--unc_metrics"' in src and '_pop(argv, "--unc_steps"' in src
    assert "return_uncertainty=True, return_prob=False" in src and "Uncertainty: " in src and "sparsification.json" in src


# ---- the numpy reference against independent forms of the definition -----------------------------------------------------------------

def _vectors(n, seed):
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.5, 9.0, n).astype(np.float32)
    v = (g + rng.choice([-1.0, 1.0], n) * rng.uniform(0.01, 0.8, n)).astype(np.float32)      # errors of at least 1 cm
    return rng, g, v


@pytest.mark.parametrize("n,K", [(5, 20), (1, 7), (1999, 7), (19200, 20), (19200, 100), (4001, 1)])
def test_reference_equals_stable_argsort_without_ties(n, K):
    rng, g, v = _vectors(n, n + K)
    t0, t1 = R.terms(g, v)
    s = rng.permutation(n).astype(np.float32) * np.float32(0.37) - np.float32(11.0)           # tie-free, both signs
    a, b = R.curve(s, t0, t1, K), R.curve_argsort(s, t0, t1, K)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    assert R.kept_counts(n, K)[0] == n and min(R.kept_counts(n, K)) >= 1


def test_reference_equals_the_mean_over_random_tie_breaks():
    """8 distinct score values: the t/c share is the expectation of the kept SUMS over a uniformly random order inside each tie group.
    200 random tie-breaks; the mean of S/n_k (abs-rel, and the squared RMSE) must lie within 5 standard errors at every point."""
    n, K, trials = 3001, 20, 200
    rng, g, v = _vectors(n, 3)
    t0, t1 = R.terms(g, v)
    s = rng.integers(0, 8, n).astype(np.float32)
    want = R.curve(s, t0, t1, K)
    got = np.empty((trials, 2, K))
    for i in range(trials):
        jitter = s.astype(np.float64) + rng.uniform(0.0, 0.5, n)                              # a random order inside every group
        got[i] = R.curve_argsort(jitter, t0, t1, K)
    got[:, 0] = got[:, 0] ** 2
    want[0] = want[0] ** 2
    mean, sem = got.mean(0), got.std(0, ddof=1) / np.sqrt(trials)
    assert (np.abs(mean - want) <= 5 * sem + 1e-12 * np.abs(want)).all(), np.abs(mean - want).max()
    assert sem.max() > 0                                                                       # the ties did matter


def test_reference_closed_forms():
    n, K = 2500, 20
    rng, g, v = _vectors(n, 11)
    t0, t1 = R.terms(g, v)
    planes = rng.uniform(0.0, 1.0, (3, n)).astype(np.float32)
    # the oracle score as the uncertainty: the same curve, AUSE exactly 0
    planes[0] = t0
    r = R.sparsify(g, v, planes, K)
    assert np.array_equal(r["curves"][0], r["curves"][3]) and r["ause"][0, 0] == 0.0
    assert (r["ause"][:, 0] >= 0).all() and (np.diff(r["curves"][3, 0]) <= 0).all() and (np.diff(r["curves"][4, 1]) <= 0).all()
    # a constant plane: flat curve at e0, AURG 0
    planes[1] = np.float32(0.25)
    r = R.sparsify(g, v, planes, K)
    assert np.abs(r["curves"][1] - r["curves"][1][:, :1]).max() <= 1e-12 * r["curves"][1].max() and np.abs(r["aurg"][1]).max() <= 1e-12
    # the negated oracle removes the best pixels first: worse than random
    planes[0] = -t0
    assert R.sparsify(g, v, planes, K)["aurg"][0, 0] < 0
    # -0 == +0 and NaN above +inf
    s = np.array([-0.0, 0.0, np.inf, np.nan, -1.0, np.nan], np.float32)
    inv, ng = R._groups(s)
    assert ng == 4 and inv.tolist() == [1, 1, 2, 3, 0, 3]
    # the same error everywhere: every curve is flat
    g2 = np.full(n, 2.0, np.float32)
    r = R.sparsify(g2, g2 + np.float32(0.5), planes, K)
    assert np.abs(r["curves"] - r["curves"][:, :, :1]).max() <= 1e-12
    # nothing valid, or no error at all: NaN
    assert np.isnan(R.sparsify(g[:0], v[:0], planes[:, :0], K)["curves"]).all()
    r = R.sparsify(g, g, planes, K)
    assert np.isnan(r["curves"]).all() and np.isnan(r["ause"]).all() and r["n_valid"] == n


def test_reference_interpolation_agrees_with_the_metrics_oracle():
    """`image_interpolated(how="aten")` is the protocol of oracle/metrics_oracle.py for the prediction, bit for bit; the two other
    roundings of the blend stay within float32 rounding of it."""
    from cfpnet_amd import synthetic
    from oracle import metrics_oracle as MO
    gt, pred = synthetic.make_eval_pair(47, 61, 23, 31, 5, 0.3, 0.2)
    pred[3, 4], pred[10, 20], pred[15, 7] = np.nan, np.inf, -np.inf
    lo, hi = 1e-3, 10.0
    valid = np.logical_and(gt > lo, gt < hi)
    for mode, proto in ((0, MO.protocol_evaluate_all), (1, MO.protocol_validate)):
        g, v = proto(pred.copy(), gt, lo, hi)
        a = R.protocol_v(pred, 47, 61, lo, hi, mode, "aten")[valid]
        assert np.array_equal(a, v, equal_nan=True)
        for how in ("ours", "f64"):
            o = R.protocol_v(pred, 47, 61, lo, hi, mode, how)[valid]
            assert np.array_equal(np.isnan(o), np.isnan(a))
            fin = ~np.isnan(a)
            assert np.abs(o[fin] - a[fin]).max() <= 4 * np.finfo(np.float32).eps * np.abs(a[fin]).max()
