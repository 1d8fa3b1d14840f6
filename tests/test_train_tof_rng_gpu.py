"""`train.py --tof_rng device`: the zone dropout of `--drop_hist` drawn by `cfp_tof_degrade` instead of numpy on the host.  The run repeats
itself, a resumed run repeats the uninterrupted one with no generator state to restore, `drop_zones` (the host path with its copy of the
mask to the host) is never reached, and `--tof_rng host` still is what it was."""
import contextlib
import io
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

COMMON = ["@" + os.path.join(ROOT, "configs", "cfpnet_combine1.txt"), "--synthetic", "8", "--bs", "2", "--epochs", "2", "--max_steps", "3",
          "--drop_hist", "0.34", "--seed", "3", "--log_every", "1"]


def _train(*extra):
    """train.main in this process -> the losses it logged."""
    import train
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train.main(COMMON + list(extra))
    text = buf.getvalue()
    losses = [float(m) for m in re.findall(r"step \d+/\d+ loss ([-\d.naninf]+)", text)]
    assert losses and all(np.isfinite(losses)), text[-2000:]
    return losses, text


def _refuse(*a, **kw):
    raise AssertionError("drop_zones reached in --tof_rng device mode")


_first = {}


def _uninterrupted(tmp_path_factory, monkeypatch):
    if not _first:
        import train
        monkeypatch.setattr(train, "drop_zones", _refuse)
        path = tmp_path_factory.mktemp("tof_rng") / "a.pt"
        _first["losses"], _ = _train("--tof_rng", "device", "--save", str(path))
        _first["weights"] = torch.load(path, map_location="cpu")
    return _first


def _same_weights(a, b):
    assert set(a) == set(b)
    return [k for k in a if torch.is_tensor(a[k]) and not torch.equal(a[k], b[k])]


def test_device_mode_repeats_itself_without_the_host_path(tmp_path, tmp_path_factory, monkeypatch):
    import train
    first = _uninterrupted(tmp_path_factory, monkeypatch)
    monkeypatch.setattr(train, "drop_zones", _refuse)
    losses, _ = _train("--tof_rng", "device", "--save", str(tmp_path / "b.pt"))
    print(first["losses"], losses)
    assert len(losses) == 3 and losses == first["losses"]
    assert not _same_weights(first["weights"], torch.load(tmp_path / "b.pt", map_location="cpu"))


def test_resumed_device_run_repeats_the_uninterrupted_one(tmp_path, tmp_path_factory, monkeypatch):
    """2 steps, then `--resume` for the third: the draws are a function of (seed, global step), so nothing has to be restored for them."""
    import train
    first = _uninterrupted(tmp_path_factory, monkeypatch)
    monkeypatch.setattr(train, "drop_zones", _refuse)
    l2, _ = _train("--tof_rng", "device", "--save", str(tmp_path / "c.pt"), "--stop_after", "2")
    ck = str(tmp_path / "c.ckpt.pt")
    assert torch.load(ck, map_location="cpu", weights_only=False)["global_step"] == 2
    l1, _ = _train("--tof_rng", "device", "--save", str(tmp_path / "d.pt"), "--resume", ck)
    assert l2 + l1 == first["losses"], (l2, l1, first["losses"])
    assert not _same_weights(first["weights"], torch.load(tmp_path / "d.pt", map_location="cpu"))


def test_host_mode_is_the_existing_path_and_device_mode_applies_the_noise(tmp_path_factory, monkeypatch):
    import train
    first = _uninterrupted(tmp_path_factory, monkeypatch)
    calls, real = [], train.drop_zones

    def counting(sim, s, drop, rng):
        calls.append(drop)
        return real(sim, s, drop, rng)

    monkeypatch.setattr(train, "drop_zones", counting)
    host, _ = _train("--tof_rng", "host", "--stop_after", "1")
    assert calls == [0.34]
    default, _ = _train("--stop_after", "1")                     # the default is the host path
    assert calls == [0.34, 0.34] and default == host
    monkeypatch.setattr(train, "drop_zones", _refuse)
    noisy, text = _train("--tof_rng", "device", "--stop_after", "1", "--noise_prob", "1.0", "--noise_sigma", "0.2")
    assert "as nyu.py:159-163 intended" in text and "has no effect" not in text
    assert noisy[0] != first["losses"][0]                        # same dropped zones, noised mu: another loss
    # nothing to drop and no noise: the device mode launches nothing extra
    from cfpnet_amd.tof import TofSimulator

    def no_launch(*a, **kw):
        raise AssertionError("degrade called with nothing to do")

    monkeypatch.setattr(TofSimulator, "degrade", no_launch)
    _train("--tof_rng", "device", "--stop_after", "1", "--drop_hist", "0")
