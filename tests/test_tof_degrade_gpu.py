"""`cfp_tof_degrade` / `TofSimulator.degrade` on the device against the numpy mirror (`tof_degrade_ref`), at the smallest shapes where each
mechanism can break: a partial wave and compaction over gaps (Z = 36), Z = 4, the cross-wave prefix (Z = 256), an image without a valid
zone, k = 0, and drop = 1 (k = n draws with replacement)."""
import types

import numpy as np
import pytest
import torch

import tof_degrade_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _sim(uniform=False):
    from cfpnet_amd.tof import TofSimulator
    return TofSimulator(types.SimpleNamespace(mode="train", train_zone_num=6, zone_sample_num=16, sample_uniform=uniform), DEV)


def _zones(B, Z, seed, valid=0.85):
    """Plausible (mu, sigma) per zone and a validity mask with gaps."""
    rng = np.random.default_rng(seed)
    fh = np.stack([0.4 + 3.2 * rng.random((B, Z)), 0.01 + 0.2 * rng.random((B, Z))], -1)
    return fh, rng.random((B, Z)) < valid


def _case(name):
    if name == "z36_gaps":
        fh, mask = _zones(3, 36, 1)
        mask[0, [0, 5, 35]] = False
        return fh, mask, 0.34, (0.5, 0.01, 0.05), False
    if name == "z4":
        fh, mask = _zones(2, 4, 2, valid=1.0)
        mask[1, 2] = False
        return fh, mask, 0.5, (1.0, 0.0, 0.02), False
    if name == "z256_cross_wave":
        fh, mask = _zones(1, 256, 3, valid=0.8)
        mask[0, [63, 64, 255]] = True, False, True
        return fh, mask, 0.34, (0.3, 0.0, 0.05), False
    if name == "z64_empty_image":
        fh, mask = _zones(2, 64, 4)
        mask[0] = False
        return fh, mask, 0.34, (0.0, 0.0, 0.0), False
    if name == "one_valid_k0":
        fh, mask = _zones(1, 36, 5)
        mask[0] = False
        mask[0, 17] = True
        return fh, mask, 0.99, (0.0, 0.0, 0.0), False
    if name == "drop_all_with_replacement":
        fh, mask = _zones(2, 36, 6)
        return fh, mask, 1.0, (0.0, 0.0, 0.0), False
    if name == "z36_uniform_samples":
        fh, mask = _zones(2, 36, 7)
        return fh, mask, 0.34, (0.5, -0.02, 0.03), True
    raise KeyError(name)


CASES = ("z36_gaps", "z4", "z256_cross_wave", "z64_empty_image", "one_valid_k0", "drop_all_with_replacement", "z36_uniform_samples")
SEED, STEP = 0x1234567890ABCDEF, 5
_done = {}


def _run(name):
    """(inputs, mirror, device result as numpy, device sample_points of the device's own (fh, mask)), computed once per case."""
    if name not in _done:
        fh, mask, drop, noise, uniform = _case(name)
        sim = _sim(uniform)
        w0, w1 = sim.w0.cpu().numpy(), None if sim.w1 is None else sim.w1.cpu().numpy()
        ref = R.degrade(fh, mask, drop, noise, SEED, STEP, w0, w1)
        d = sim.degrade({"fh": torch.from_numpy(fh).to(DEV), "mask": torch.from_numpy(mask).to(DEV)}, drop=drop, noise=noise, seed=SEED, step=STEP)
        plain = sim.sample_points(d["fh"], d["mask"])
        torch.cuda.synchronize()
        _done[name] = (fh, mask, drop, ref, {k: v.cpu().numpy() for k, v in d.items()}, plain.cpu().numpy())
    return _done[name]


@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_the_mirror(name):
    fh, mask, drop, ref, got, plain = _run(name)
    assert np.array_equal(got["mask"], ref["mask"])
    assert np.array_equal(got["counts"], ref["counts"]), (got["counts"], ref["counts"])
    pts = got["hist_data"]
    assert not pts[~ref["mask"]].any()                                                           # exactly zero rows
    quiet = ref["mask"] & ~ref["noised"]
    assert np.array_equal(got["fh"][~ref["noised"]], fh[~ref["noised"]])                         # untouched (mu, sigma) bit for bit
    assert np.array_equal(pts[quiet], plain[quiet]) and np.array_equal(pts[quiet], ref["pts"][quiet])
    assert np.array_equal(got["fh"][..., 1], fh[..., 1])                                         # sigma is never touched
    hit = ref["noised"]
    if hit.any():
        err = np.abs(got["fh"][hit][:, 0] - ref["fh"][hit][:, 0]).max()
        ulp = np.spacing(np.abs(ref["pts"][hit]).astype(np.float32))
        perr = (np.abs(pts[hit].astype(np.float64) - ref["pts"][hit].astype(np.float64)) / ulp).max()
        print(f"{name}: {int(hit.sum())} zones noised, mu error {err:.2e}, samples {perr:.2f} ulp")
        assert err <= 1e-12
        assert perr <= 1.0
        assert np.array_equal(pts[hit], plain[hit])          # the samples are those of the device's own noised (mu, sigma)
    # what each case is there for
    n = mask.sum(1)
    if name == "z64_empty_image":
        assert n[0] == 0 and not got["counts"][0].any() and not got["mask"][0].any() and got["counts"][1, 1] > 0
    if name == "one_valid_k0":
        assert got["counts"].tolist() == [[1, 0, 0]] and np.array_equal(got["mask"], mask)
    if name == "drop_all_with_replacement":
        assert (got["counts"][:, 1] < n).all() and got["mask"].any(1).all()          # k = n draws, yet not everything is dropped
    if name == "z256_cross_wave":
        assert n[0] > 192 and got["counts"][0, 1] > 40          # the list spans all four waves, and so do the draws


def test_nothing_asked_changes_nothing():
    sim = _sim()
    fh, mask = _zones(3, 36, 11)
    s = {"fh": torch.from_numpy(fh).to(DEV), "mask": torch.from_numpy(mask).to(DEV), "rect_data": torch.zeros(3, 36, 4, device=DEV)}
    d = sim.degrade(s, drop=0.0, noise=(0.0, 0.5, 0.5), seed=1, step=2)
    assert torch.equal(d["mask"], s["mask"]) and torch.equal(d["fh"], s["fh"]) and torch.equal(d["hist_data"], sim.sample_points(s["fh"], s["mask"]))
    assert d["rect_data"] is s["rect_data"]
    assert d["counts"].cpu().tolist() == [[int(m.sum()), 0, 0] for m in mask]


def _equal(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("mask", "fh", "hist_data", "counts"))


def test_same_seed_and_step_same_result_and_another_step_another_mask():
    sim = _sim()
    fh, mask = _zones(3, 36, 12)
    s = {"fh": torch.from_numpy(fh).to(DEV), "mask": torch.from_numpy(mask).to(DEV)}
    kw = dict(drop=0.34, noise=(0.5, 0.0, 0.05), seed=4242)
    a, b, c = sim.degrade(s, step=7, **kw), sim.degrade(s, step=7, **kw), sim.degrade(s, step=8, **kw)
    assert _equal(a, b)
    assert not torch.equal(a["mask"], c["mask"])
    e = sim.degrade(s, step=7, drop=0.34, noise=(0.5, 0.0, 0.05), seed=4243)
    assert not torch.equal(a["mask"], e["mask"])
    # results written into caller-owned tensors are the same ones
    out = {k: torch.empty_like(v) for k, v in a.items()}
    assert sim.degrade(s, step=7, out=out, **kw) is out and _equal(a, out)


def test_an_image_depends_on_its_own_inputs_and_index_only():
    """Image b of a B = 3 launch keeps its result when the other images' data change; image 0 is what a launch of it alone gives."""
    sim = _sim()
    fh, mask = _zones(3, 36, 13)
    kw = dict(drop=0.34, noise=(0.5, 0.0, 0.05), seed=99, step=3)
    base = sim.degrade({"fh": torch.from_numpy(fh).to(DEV), "mask": torch.from_numpy(mask).to(DEV)}, **kw)
    fh2, mask2 = _zones(3, 36, 14, valid=0.5)
    for b in range(3):
        f, m = fh2.copy(), mask2.copy()
        f[b], m[b] = fh[b], mask[b]
        other = sim.degrade({"fh": torch.from_numpy(f).to(DEV), "mask": torch.from_numpy(m).to(DEV)}, **kw)
        assert all(torch.equal(base[k][b], other[k][b]) for k in ("mask", "fh", "hist_data", "counts")), b
        assert not torch.equal(base["mask"][(b + 1) % 3], other["mask"][(b + 1) % 3])
    alone = sim.degrade({"fh": torch.from_numpy(fh[:1]).to(DEV), "mask": torch.from_numpy(mask[:1]).to(DEV)}, **kw)
    assert all(torch.equal(base[k][:1], alone[k]) for k in ("mask", "fh", "hist_data", "counts"))


def test_degrade_refuses_what_it_cannot_take():
    sim = _sim()
    fh, mask = _zones(2, 36, 15)
    fh, mask = torch.from_numpy(fh).to(DEV), torch.from_numpy(mask).to(DEV)
    for bad in ({"fh": fh.cpu(), "mask": mask}, {"fh": fh, "mask": mask.cpu()}, {"fh": fh.float(), "mask": mask}, {"fh": fh, "mask": mask.to(torch.uint8)},
                {"fh": fh, "mask": mask[:1]}):
        with pytest.raises(ValueError):
            sim.degrade(bad, drop=0.34)
    with pytest.raises(ValueError, match="out"):
        sim.degrade({"fh": fh, "mask": mask}, drop=0.34, out={"mask": torch.empty(2, 36, dtype=torch.bool, device=DEV)})
    with pytest.raises(RuntimeError, match="drop must be"):
        sim.degrade({"fh": fh, "mask": mask}, drop=1.5)


def test_simulate_then_degrade_never_waits_for_the_device(monkeypatch):
    """The host path (`train.drop_zones`) copies the mask to the host; `degrade` must not.  The probe is torch's sync debug mode, shown to
    work on `drop_zones` first; on a build that does not implement it, `Tensor.cpu` / `Tensor.item` are patched to raise instead."""
    import train
    from cfpnet_amd import synthetic
    sim = _sim()
    depth = torch.from_numpy(np.stack([synthetic.make_depth(416, 544, seed=3 + i, holes=0.1) for i in range(2)])).to(DEV)
    s = sim.simulate(depth)
    torch.cuda.synchronize()

    def device_path():
        s2 = sim.simulate(depth)
        return s2, sim.degrade(s2, drop=0.34, noise=(0.5, 0.0, 0.02), seed=4242, step=0)

    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            train.drop_zones(sim, s, 0.34, np.random.default_rng(0))
            probe_works = False
        except RuntimeError:
            probe_works = True
        if probe_works:
            s2, d = device_path()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not probe_works:
        def refuse(*a, **kw):
            raise AssertionError("device-to-host copy")
        monkeypatch.setattr(torch.Tensor, "cpu", refuse)
        monkeypatch.setattr(torch.Tensor, "item", refuse)
        with pytest.raises(AssertionError, match="device-to-host"):
            train.drop_zones(sim, s, 0.34, np.random.default_rng(0))
        s2, d = device_path()
        monkeypatch.undo()
    torch.cuda.synchronize()
    assert torch.equal(s2["mask"], s["mask"]) and int(d["counts"][:, 1].sum()) > 0 and not bool((d["mask"] & ~s["mask"]).any())
