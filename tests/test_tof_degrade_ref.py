"""ToF degradation (`cfp_tof_degrade`), the parts that need no GPU: known answers of Philox4x32-10, the statistics of the mirror
(`tof_degrade_ref`), the header's statement of the definition, argument validation of the entry point, and the plumbing of the flags
(`train.py --tof_rng`, `evaluate_all.py --robust_*`)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import tof_degrade_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from cfpnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.load()


@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
], ids=["zeros", "ones", "pi"])
def test_philox_known_answers(ctr, key, want):
    assert " ".join(f"{w:08x}" for w in R.philox4x32_10(ctr, key)) == want


def test_dropout_of_the_mirror_is_unbiased():
    """2000 images with all 36 zones valid, drop 0.34: k = 12 draws with replacement.  The number of distinct zones dropped has mean
    36 (1 - (35/36)^12) = 10.326; the 24000 draws are uniform over the zones (chi-square with 35 degrees of freedom: mean 35,
    standard deviation sqrt(70))."""
    N, Z = 2000, 36
    key = R.seed_key(4242)
    full = np.ones(Z, dtype=bool)
    distinct, hits = [], np.zeros(Z)
    for b in range(N):
        drawn = R.dropped_zones(full, 0.34, key, b % 7, b)
        assert len(drawn) == 12
        distinct.append(len(set(drawn)))
        np.add.at(hits, drawn, 1)
    distinct = np.array(distinct, dtype=np.float64)
    want = Z * (1 - (35 / 36) ** 12)
    se = distinct.std(ddof=1) / math.sqrt(N)
    chi2 = float(((hits - hits.sum() / Z) ** 2 / (hits.sum() / Z)).sum())
    print(f"mean distinct dropped {distinct.mean():.4f} (closed form {want:.4f}, {(distinct.mean() - want) / se:+.2f} SE), chi-square {chi2:.1f}")
    assert abs(distinct.mean() - want) <= 4 * se
    assert chi2 <= 35 + 4 * math.sqrt(70)


def test_noise_of_the_mirror_is_standard_normal():
    N = 20000
    v = np.array([R.standard_normal(R.philox4x32_10((b % 64, b // 64, 3, 1), (7, 0))) for b in range(N)])
    print(f"mean {v.mean() * math.sqrt(N):+.2f} / sqrt(N), std {v.std():.5f}")
    assert abs(v.mean()) <= 4 / math.sqrt(N)
    assert abs(v.std() - 1) <= 0.03


def test_mirror_order_and_identity():
    """Dropout first, then noise on what is still valid, then the samples; nothing asked = nothing changed."""
    from oracle import tof_oracle as TO
    rng = np.random.default_rng(0)
    fh = np.stack([1 + rng.random((2, 36)), 0.02 + 0.1 * rng.random((2, 36))], -1)
    mask = rng.random((2, 36)) < 0.8
    w0 = TO.icdf_table_f32(16)
    same = R.degrade(fh, mask, w0=w0)
    assert np.array_equal(same["mask"], mask) and np.array_equal(same["fh"], fh) and not same["counts"][:, 1:].any()
    assert np.array_equal(same["pts"][0], TO.sample_points_icdf(fh[0], mask[0], w0))
    d = R.degrade(fh, mask, drop=0.5, noise=(1.0, 0.0, 0.05), seed=9, step=2, w0=w0)
    assert np.array_equal(d["noised"], d["mask"]) and not (d["mask"] & ~mask).any()
    assert np.array_equal(d["counts"][:, 0], mask.sum(1)) and np.array_equal(d["counts"][:, 1], (mask & ~d["mask"]).sum(1))
    assert (d["counts"][:, 1] <= (mask.sum(1) * 0.5).astype(int)).all() and (d["counts"][:, 1] > 0).all()
    assert np.array_equal(d["fh"][~d["mask"]], fh[~d["mask"]]) and not (d["fh"][d["mask"]][:, 0] == fh[d["mask"]][:, 0]).any()
    assert np.array_equal(d["fh"][..., 1], fh[..., 1])
    assert not d["pts"][~d["mask"]].any()


def test_header_states_the_definition():
    text = open(os.path.join(ROOT, "include", "cfpnet_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int cfp_tof_degrade\(", text, flags=re.S)
    assert m, "cfp_tof_degrade has no comment in front of it"
    doc = " ".join(re.sub(r"^\s*\*", "", m.group(1), flags=re.M).split())
    for needle in ("Philox4x32-10", "key (seed & 0xffffffff, seed >> 32)", "counter (i, b, step, stream)", "k = (int)(n * drop)",
                   "with replacement", "(word0(j) * n) >> 32", "bias below n / 2^32", "w0 * 2^-32 < noise_prob",
                   "noise_mean + noise_sigma * sqrt(-2 ln((w1 + 1) * 2^-32)) * cos(2 pi * w2 * 2^-32)", "Z <= 256", "2^31", "bit for bit"):
        assert needle in doc, needle


def test_argument_validation_is_reported_not_faulted(lib):
    """Fake non-null pointers: every call below returns before anything is launched."""
    from cfpnet_amd import hip

    def call(fh=16, mask=16, B=2, Z=36, drop=0.34, prob=0.0, mean=0.0, sigma=0.0, w0=16, w1=0, nsamp=16, mode=hip.TOF_SAMPLE_ICDF, mask_out=16,
             fh_out=16, pts=16, counts=0):
        return lib.cfp_tof_degrade(fh, mask, B, Z, drop, prob, mean, sigma, 4242, 0, w0, w1, nsamp, mode, mask_out, fh_out, pts, counts, 0)

    for name in ("fh", "mask", "w0", "mask_out", "pts"):
        assert call(**{name: 0}) == -1 and "null" in hip.last_error(), name
    assert call(mode=hip.TOF_SAMPLE_UNIFORM) == -1 and "null" in hip.last_error()             # the uniform branch needs w1
    assert call(fh_out=0, prob=0.5) == -1 and "null" in hip.last_error()                      # fh_out may be NULL only without noise
    assert call(mode=7, w1=16) == -1 and "sample_mode" in hip.last_error()
    for Z in (0, 257, -1):
        assert call(Z=Z) == -2 and "1..256" in hip.last_error(), Z
    assert call(B=0) == -2 and call(nsamp=0) == -2
    assert call(B=1 << 24, Z=256) == -2 and "2^31" in hip.last_error()
    for drop in (1.5, -0.1, float("nan")):
        assert call(drop=drop) == -1 and "drop" in hip.last_error(), drop
    for prob in (1.5, -0.1, float("nan")):
        assert call(prob=prob) == -1 and "noise_prob" in hip.last_error(), prob
    for sigma in (-1e-9, -1.0, float("nan"), float("inf")):
        assert call(prob=0.5, sigma=sigma) == -1 and "noise_sigma" in hip.last_error(), sigma
    with pytest.raises(RuntimeError, match=r"cfp_tof_degrade failed \(-2\)"):
        hip.call("cfp_tof_degrade", 16, 16, 2, 257, 0.0, 0.0, 0.0, 0.0, 1, 0, 16, 0, 16, hip.TOF_SAMPLE_ICDF, 16, 16, 16, 0, 0)


def test_degrade_refuses_host_tensors_and_wrong_dtypes():
    """`TofSimulator.degrade` checks its tensors before the library sees a pointer (no device needed to be refused)."""
    from cfpnet_amd.tof import TofSimulator
    sim = TofSimulator.__new__(TofSimulator)
    sim.nsamp, sim.uniform, sim.w0, sim.w1 = 16, False, torch.zeros(16), None
    fh, mask = torch.zeros(2, 36, 2, dtype=torch.float64), torch.zeros(2, 36, dtype=torch.bool)
    with pytest.raises(ValueError, match="fh must be"):
        sim.degrade({"fh": fh, "mask": mask})
    with pytest.raises(ValueError, match="fh must be"):
        sim.degrade({"fh": fh.float(), "mask": mask})


def _stop_at(monkeypatch, module, name):
    seen = {}

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(module, name, fake)
    return seen, Stop


def test_train_cli_pops_the_flag(monkeypatch):
    """`--tof_rng host|device` is taken out of argv before the reference's flag table sees it; anything else is refused."""
    import train
    from cfpnet_amd import config, trainer
    assert "tof_rng" not in vars(config.defaults())
    _, Stop = _stop_at(monkeypatch, trainer, "Trainer")
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)
    for mode in ("host", "device"):
        with pytest.raises(Stop):
            train.main(["--synthetic", "4", "--max_steps", "1", "--tof_rng", mode, "--eager"])
    with pytest.raises(ValueError, match="--tof_rng"):
        train.main(["--synthetic", "4", "--max_steps", "1", "--tof_rng", "numpy", "--eager"])


def test_train_cli_says_what_the_noise_flags_do(monkeypatch, capsys):
    import train
    from cfpnet_amd import trainer
    _, Stop = _stop_at(monkeypatch, trainer, "Trainer")
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)
    with pytest.raises(Stop):
        train.main(["--synthetic", "4", "--max_steps", "1", "--noise_prob", "0.5", "--noise_sigma", "0.03", "--tof_rng", "device", "--eager"])
    out = capsys.readouterr().out
    assert "as nyu.py:159-163 intended" in out and "has no effect" not in out
    with pytest.raises(Stop):
        train.main(["--synthetic", "4", "--max_steps", "1", "--noise_prob", "0.5", "--noise_sigma", "0.03", "--eager"])
    assert "has no effect" in capsys.readouterr().out


def test_evaluate_cli_pops_the_flags(monkeypatch):
    """`--robust_drop`, `--robust_sigma` and `--robust_seed` are popped before the reference's flag table; bad lists are refused before the
    model is built."""
    import evaluate_all
    from cfpnet_amd import config, deltar
    d = vars(config.defaults())
    assert not [k for k in d if k.startswith("robust")]
    seen, Stop = _stop_at(monkeypatch, deltar, "make_model")
    with pytest.raises(Stop):
        evaluate_all.main(["--synthetic", "2", "--robust_drop", "0,0.5", "--robust_sigma", "0.05", "--robust_seed", "3"])
    for bad in (["--robust_drop", "1.5"], ["--robust_drop", "-0.1"], ["--robust_sigma", "-1"], ["--robust_drop", "0.5,0.5"], ["--robust_seed", "3"]):
        with pytest.raises(ValueError, match="--robust_"):
            evaluate_all.main(["--synthetic", "2"] + bad)
    assert evaluate_all.ROBUST_SEED == 117010053
