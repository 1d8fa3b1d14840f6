"""`cfp_tof_zone_loss` on the GPU against the float64 restatement (`zone_loss_ref.py`, itself checked in test_zone_loss_ref.py), on every
case of its table at the case's own floor and at floor 20.

Tolerances, none of them measured on the kernel:
  integers   n_z, run_start, run_stop, state: equal.
  m_z, r_z   m_z within n_pix * 2^-52 relative (float64 summation in another order); r_z = m_z - mu_m within that of max(|m_z|, |mu_m|).
  rho, coef  functions of r_z in float64: the same bound propagated, n_pix * 2^-52 * max(|m_z|, |mu_m|) / delta relative to full scale.
  L, L_b     float32 roundings of float64 values: L_b within 2^-24 relative, L (the float64 mean of the float32 L_b) within 2 * 2^-24.
  grad_pred  within (T + 4) * 2^-24 * sum |terms| per element, T the number of terms; no element is exempt.
  accumulate one float32 addition: |got - (base + g)| <= 2^-24 * |base + g|, g the accumulate = 0 result."""
import functools

import numpy as np
import pytest
import torch

import zone_consistency_ref as ZR
import zone_loss_ref as R

pytestmark = pytest.mark.gpu

from cfpnet_amd import hip, tof, train_ops  # noqa: E402

DEV = "cuda:0"
GUARD = 4096
EPS32, EPS64 = 2.0 ** -24, 2.0 ** -52


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)        # a copy: the shared inputs are read-only arrays


def zl_abi(name, floor, grad=True, accumulate=0, base=None, delta=R.BIN_WIDTH, grad_scale=1.0):
    """The C entry point itself, every output pre-filled with a sentinel and with sentinel guard elements behind it -> numpy dict."""
    a = R.run_args(name, floor)
    p, r, m, w = dev(a["pred"]), dev(a["rect"]), dev(a["mask"]), dev(a["raw"])
    B, h, wd = a["pred"].shape
    Z, bins = a["rect"].shape[1], ZR.n_bins(a["max_d"])
    nws = int(hip.load().cfp_tof_zone_loss_ws_bytes(B, Z, bins))
    assert nws == B * Z * bins * 8
    ws = torch.full((nws // 8 + 8,), -88.0, dtype=torch.float64, device=DEV)
    zone = torch.full((B * Z * 8 + 8,), -77.0, dtype=torch.float64, device=DEV)
    out = torch.full((1 + B + 8,), -66.0, dtype=torch.float32, device=DEV)
    gp = None
    if grad:
        gp = torch.full((B * h * wd + GUARD,), -55.0, dtype=torch.float32, device=DEV)
        if base is not None:
            gp[:B * h * wd] = dev(base).reshape(-1)
    hip.call("cfp_tof_zone_loss", p.data_ptr(), h, wd, a["H"], a["W"], B, a["interp"], a["lo"], a["hi"], r.data_ptr(), m.data_ptr(), w.data_ptr(), Z,
             a["max_d"], bins, R.BIN_WIDTH, floor, delta, grad_scale, accumulate, ws.data_ptr(), nws, zone.data_ptr(), out.data_ptr(), hip.ptr(gp),
             hip.current_stream())
    ws, zone, out = ws.cpu().numpy(), zone.cpu().numpy(), out.cpu().numpy()
    assert (ws[nws // 8:] == -88.0).all() and (zone[B * Z * 8:] == -77.0).all() and (out[1 + B:] == -66.0).all()
    res = dict(zone=zone[:B * Z * 8].reshape(B, Z, 8), out=out[:1 + B], table=ws[:nws // 8].reshape(B, Z, bins))
    assert not (res["zone"] == -77.0).any() and not (res["out"] == -66.0).any() and not (res["table"] == -88.0).any()      # every entry written
    if grad:
        gp = gp.cpu().numpy()
        assert (gp[B * h * wd:] == -55.0).all()
        res["grad"] = gp[:B * h * wd].reshape(B, h, wd)
        if accumulate == 0:
            assert not (res["grad"] == -55.0).any()
    return res


@functools.lru_cache(maxsize=None)
def run(name, floor):
    """One call per (case, floor) with the gradient, shared by the tests; read-only."""
    return zl_abi(name, floor)


@pytest.mark.parametrize("name,floor", R.RUNS)
def test_zone_table_matches_the_restatement(name, floor):
    got, want = run(name, floor)["zone"], R.reference(name, floor)["zone"]
    raw, npix = R.inputs(name)[3], R.n_pix(name)
    for k in R.INT_COLS:
        assert np.array_equal(got[..., k], want[..., k]), (name, k, got[..., k].tolist(), want[..., k].tolist())
    assert np.array_equal(np.isnan(got[..., R.R]), np.isnan(want[..., R.R]))                 # the same zones are compared
    cmp_ = ~np.isnan(want[..., R.R])
    rel = npix * EPS64
    dm = np.abs(got[..., R.M] - want[..., R.M])
    assert (dm <= rel * np.abs(want[..., R.M])).all(), (name, float(dm.max()))
    size = np.maximum(np.abs(want[..., R.M]), np.abs(raw[..., 0]))
    dr = np.abs(got[..., R.R] - want[..., R.R])[cmp_]
    assert (dr <= (rel * size)[cmp_]).all(), (name, float(dr.max()) if dr.size else 0.0)
    # rho and coef are at most 1-Lipschitz / (1 / delta)-Lipschitz in r_z, in units of their full scale
    drho = np.abs(got[..., R.RHO] - want[..., R.RHO])
    assert (drho <= 2 * rel * size + 4 * EPS64 * np.abs(want[..., R.RHO])).all()
    nb = np.maximum(cmp_.sum(1, keepdims=True), 1)
    dco = np.abs(got[..., R.COEF] - want[..., R.COEF])
    assert (dco <= (2 * rel * size / R.BIN_WIDTH + 8 * EPS64) / (len(got) * nb)).all()
    assert not got[..., R.RHO][~cmp_].any() and not got[..., R.COEF][~cmp_].any()
    none = want[..., R.N] == 0
    assert (got[..., R.M][none] == 0.0).all()
    print(f"{name} floor {floor}: compared {int(cmp_.sum())}, worst |dm| {dm.max():.2e}, |dr| {dr.max() if dr.size else 0:.2e}, |dcoef| {dco.max():.2e}")


@pytest.mark.parametrize("name,floor", R.RUNS)
def test_workspace_table_is_omega_over_n(name, floor):
    """The per-zone, per-bin table the backward reads: omega_j / n_z on the run, 0 elsewhere; a ratio of integers, two float64 divisions."""
    got = run(name, floor)
    a = R.run_args(name, floor)
    d = R.depth(name, a["pred"])
    bins = ZR.n_bins(a["max_d"])
    for b in range(d.shape[0]):
        for z in range(a["rect"].shape[1]):
            v = d[b][ZR.members(a["rect"][b, z], a["H"], a["W"])]
            bn, w, s, e, n = R.zone_run(v, a["max_d"], bins, floor)
            want = np.zeros(bins)
            if n > 0:
                sel = w > 0
                want[bn[sel]] = w[sel] / n
            assert np.abs(got["table"][b, z] - want).max() <= 2 * EPS64 * max(want.max(), 1e-300), (name, b, z)


@pytest.mark.parametrize("name,floor", R.RUNS)
def test_loss_values_are_float32_roundings_of_the_restatement(name, floor):
    got, want = run(name, floor)["out"], R.reference(name, floor)["out"]
    print(f"{name} floor {floor}: L {got[0]:.9g} (ref {want[0]:.17g}), L_b {got[1:].tolist()}")
    assert got.dtype == np.float32 and np.isfinite(got).all()
    slack = 4096 * EPS64 * 50.0                                     # the zone means' summation order (n_pix <= 4096, depths <= 50), rho is 1-Lipschitz
    assert (np.abs(got[1:] - want[1:]) <= EPS32 * np.abs(want[1:]) + slack).all()
    assert abs(got[0] - want[0]) <= 2 * EPS32 * abs(want[0]) + slack
    assert (got[1:][want[1:] == 0] == 0).all()                      # n_b = 0 contributes exactly 0


@pytest.mark.parametrize("name,floor", R.RUNS)
def test_gradient_is_within_float32_rounding_of_its_terms(name, floor):
    got, ref = run(name, floor)["grad"], R.reference(name, floor)
    bound = (ref["terms_n"] + 4) * EPS32 * ref["terms_abs"]
    err = np.abs(got.astype(np.float64) - ref["grad"])
    worst = float((err / np.maximum(bound, 1e-300)).max()) if (bound > 0).any() else 0.0
    print(f"{name} floor {floor}: {int((ref['grad'] != 0).sum())} of {got.size} elements with a gradient, largest {np.abs(ref['grad']).max():.3e}, "
          f"worst error / bound {worst:.3f}")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), (name, floor, float(err.max()))                # where there are no terms the gradient is exactly 0
    if name == "batch3_nonfinite":
        pred = R.inputs(name)[0]
        assert not np.isfinite(pred).all() and not got[~np.isfinite(pred)].any()


@pytest.mark.parametrize("name,floor", R.RUNS)
def test_accumulate_value_only_and_repeat(name, floor):
    first = run(name, floor)
    again = zl_abi(name, floor)
    for k in ("zone", "out", "grad", "table"):
        assert first[k].tobytes() == again[k].tobytes(), k                       # two calls: identical bits
    value = zl_abi(name, floor, grad=False)
    assert value["out"].tobytes() == first["out"].tobytes() and value["zone"].tobytes() == first["zone"].tobytes()
    base = np.random.default_rng(7).normal(0.0, 1e-3, first["grad"].shape).astype(np.float32)
    acc = zl_abi(name, floor, accumulate=1, base=base)
    want = base.astype(np.float64) + first["grad"].astype(np.float64)
    assert (np.abs(acc["grad"].astype(np.float64) - want) <= EPS32 * np.abs(want)).all()
    assert acc["out"].tobytes() == first["out"].tobytes()


def test_delta_and_grad_scale():
    """Another Huber threshold and a gradient scale, on the case with residuals in all three parts."""
    name, floor = "interp_19x27_to_37x53", 2
    got = zl_abi(name, floor, delta=0.1, grad_scale=0.25)
    ref = R.loss(**R.run_args(name, floor), delta=0.1, grad_scale=0.25)
    assert (np.abs(got["out"] - ref["out"]) <= 2 * EPS32 * np.abs(ref["out"]) + 1e-12).all()
    err = np.abs(got["grad"].astype(np.float64) - ref["grad"])
    assert (err <= (ref["terms_n"] + 4) * EPS32 * ref["terms_abs"]).all() and np.abs(ref["grad"]).max() > 0
    assert not np.array_equal(got["out"], run(name, floor)["out"])


def test_python_wrapper_and_autograd_function():
    """train_ops.ZoneLoss keeps its buffers, adds into `grad_out`, and `zone_loss` is differentiable w.r.t. `pred` at the module boundary."""
    name = "batch3_nonfinite"
    a = R.run_args(name)
    ref = R.reference(name)
    p, r, m, w = dev(a["pred"]), dev(a["rect"]), dev(a["mask"]), dev(a["raw"])
    kw = dict(size=(a["H"], a["W"]), max_distance=a["max_d"], floor_count=a["floor"])
    crit = train_ops.ZoneLoss()
    L = crit(p, w, r, m, a["lo"], a["hi"], **kw)
    first = run(name, a["floor"])
    assert train_ops.ZONE_LOSS_COLUMNS == R.COLUMNS and tof.BIN_WIDTH == R.BIN_WIDTH
    assert np.array_equal(crit.zone.cpu().numpy(), first["zone"], equal_nan=True) and float(L) == first["out"][0]
    assert np.array_equal(crit.per_image.cpu().numpy(), first["out"][1:]) and np.array_equal(crit.grad_pred.cpu().numpy(), first["grad"])
    ptrs = (crit._ws.data_ptr(), crit._out.data_ptr(), crit.zone.data_ptr(), crit.grad_pred.data_ptr())
    crit(p, w, r, m, a["lo"], a["hi"], **kw)
    assert ptrs == (crit._ws.data_ptr(), crit._out.data_ptr(), crit.zone.data_ptr(), crit.grad_pred.data_ptr())     # kept between calls
    assert torch.equal(crit.backward(2.0), crit.grad_pred * 2.0)
    base = torch.full_like(p, 0.5)
    crit(p, w, r, m, a["lo"], a["hi"], grad_scale=0.5, grad_out=base, **kw)
    assert crit.grad_pred is base
    assert np.abs(base.cpu().numpy() - (0.5 + 0.5 * ref["grad"])).max() <= 2 * EPS32
    # the module boundary: a finite prediction so that torch's own clamp / sum have a gradient to compare
    q = torch.nan_to_num(p, nan=1.5, posinf=2.0, neginf=1.0).requires_grad_(True)
    loss = 3.0 * train_ops.zone_loss(q[:, None], w, r, m, a["lo"], a["hi"], **kw)
    loss.backward()
    crit2 = train_ops.ZoneLoss()
    crit2(q.detach(), w, r, m, a["lo"], a["hi"], **kw)
    assert q.grad.shape == q.shape and torch.equal(q.grad, 3.0 * crit2.grad_pred) and float(q.grad.abs().max()) > 0
    with pytest.raises(ValueError, match="rect_data"):
        crit(p, w, r[:, :, :3], m, a["lo"], a["hi"], **kw)
    with pytest.raises(ValueError, match="raw_data"):
        crit(p, w.cpu(), r, m, a["lo"], a["hi"], **kw)
