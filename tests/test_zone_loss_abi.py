"""Zone-consistency loss, the parts that need no GPU: the header's statement of the definition, argument validation of the entry point
(every refusal returns before anything is launched), and the plumbing of the weight (`train.py --w_zone`, `Trainer`, `TrainNet`)."""
import inspect
import os
import re

import pytest
import torch

import zone_loss_ref as R
from zone_abi_cases import EINVAL, ESHAPE, check_shared_refusals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cfpnet_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    from cfpnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.load()


def test_header_states_the_definition():
    text = open(os.path.join(ROOT, "include", "cfpnet_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*size_t cfp_tof_zone_loss_ws_bytes", text, flags=re.S)
    assert m, "cfp_tof_zone_loss_ws_bytes has no comment in front of it"
    doc = " ".join(re.sub(r"\n \*", "\n", m.group(1)).split())
    for needle in ("omega_j = c'_j / cnt_j for j in [a, b), 0 elsewhere",                                   # weights
                   "m_z = (1/n_z) sum_{i in zone} omega_{bin(d_i)} * d_i", "accumulated in float64 over the float32 d_i",
                   "|m_z - mu_z| <= bin_width/2", "lowest start winning ties",
                   "e_z = max(|r_z| - bin_width/2, 0)",                                                     # dead zone
                   "rho_z = e_z^2 / (2 delta) if e_z <= delta, else e_z - delta/2", "delta > 0",             # Huber
                   "n_b = 0 contributes 0", "L = (1/B) sum_b L_b", "mu_m (raw[b][z][0]) is finite",
                   "grad_scale * min(e_z/delta, 1) * sgn(r_z) * omega_{bin(d_i)} / (B * n_b * n_z)",
                   "[lo <= pred_t <= hi]", "closed interval, as torch.clamp", "A NaN d_i has no bin and no gradient",   # clip derivative
                   "the run and the weights held constant", "sigma column of raw is not used",
                   "{m_z, n_z, r_z, rho_z, run_start, run_stop, state, coef}", "accumulate = 1 adds",
                   "no global atomics and no floating-point atomics", "identical bits",                    # determinism
                   "csrc/metrics_pred.h", "csrc/tof_cluster.h", "16-byte aligned"):
        assert needle in doc, needle
    assert "int cfp_tof_zone_loss(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi," in text
    assert "double* zone /* [B][Z][8] */, float* out /* [1+B] */, float* grad_pred /* [B][Hp][Wp] or NULL */" in text


def test_symbol_binding_makefile_and_shared_code(lib):
    from cfpnet_amd import hip, tof, train_ops
    assert hasattr(lib, "cfp_tof_zone_loss") and hasattr(lib, "cfp_tof_zone_loss_ws_bytes")
    # the metric's arguments up to floor_count, then delta, grad_scale, accumulate, ws, ws_bytes, zone, out, grad_pred, stream
    assert hip.SIGNATURES["cfp_tof_zone_loss"][1][:17] == hip.SIGNATURES["cfp_tof_zone_consistency"][1][:17]
    assert len(hip.SIGNATURES["cfp_tof_zone_loss"][1]) == 26
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert " zone_loss.hip " in mk and re.search(r"^zone_loss\.o:.*tof_cluster\.h", mk, flags=re.M) and re.search(r"^zone_loss\.o:.*metrics_pred\.h", mk, flags=re.M)
    assert re.search(r"^zone_consistency\.o zone_loss\.o: zone_core\.h$", mk, flags=re.M)
    src = open(os.path.join(CSRC, "zone_loss.hip")).read()
    core = open(os.path.join(CSRC, "zone_core.h")).read()   # what it shares with the metric; both headers reach it through the core
    assert '#include "zone_core.h"' in src and '#include "metrics_pred.h"' in core and '#include "tof_cluster.h"' in core
    for call in ("met_pred(", "tof_bin(", "tof_hist_add(", "tof_cluster(", "ZoneSweep sweep(", "zone_args("):   # the metric's bits: included, not restated
        assert call in src, call
    metric = open(os.path.join(CSRC, "zone_consistency.hip")).read()
    for shared in ("zc_span(", "npx - 1", "__ballot(keep)", "non-positive dimension", "met_params("):   # the sweep, the staging and the checks: once
        assert shared in core and shared not in src and shared not in metric, shared
    for restated in ("clipf(", "atomicMax(", "__ffsll(", "max_d - 0.f", "ceilf(a)"):
        assert restated not in src and restated not in core, restated
    for atomic in ("atomicAdd(", "atomicExch(", "atomicCAS("):                                        # its only atomics are tof_cluster.h's, on LDS integers
        assert atomic not in src and atomic not in core, atomic
    assert train_ops.ZONE_LOSS_COLUMNS == R.COLUMNS and tof.BIN_WIDTH == R.BIN_WIDTH
    assert lib.cfp_tof_zone_loss_ws_bytes(2, 9, 100) == 2 * 9 * 100 * 8


def test_entry_point_refuses_bad_arguments_with_a_message(lib):
    """16 = a non-null dummy device pointer: every case fails a check before anything is dereferenced or launched."""
    from cfpnet_amd import hip
    P = 16
    need = lib.cfp_tof_zone_loss_ws_bytes(1, 4, 100)
    assert need == 4 * 100 * 8

    def call(pred=P, hp=8, wp=8, h=8, w=8, b=1, interp=0, lo=1e-3, hi=10.0, rect=P, mask=P, raw=P, z=4, md=4.0, bins=100, bw=0.04, floor=20,
             delta=0.04, scale=1.0, acc=0, ws=P, nws=None, zone=P, out=P, grad=0):
        rc = lib.cfp_tof_zone_loss(pred, hp, wp, h, w, b, interp, lo, hi, rect, mask, raw, z, md, bins, bw, floor, delta, scale, acc, ws,
                                   need if nws is None else nws, zone, out, grad, 0)
        return rc, hip.last_error()

    for name in ("pred", "rect", "mask", "raw", "ws", "zone", "out"):
        rc, msg = call(**{name: 0})
        assert rc == EINVAL and "cfp_tof_zone_loss: null pointer" in msg, (name, rc, msg)
    check_shared_refusals("cfp_tof_zone_loss", call)      # dimensions, sizes, range, bins, histogram, B * Z, and their order
    for bins in (0, -1, 1025):
        assert lib.cfp_tof_zone_loss_ws_bytes(1, 4, bins) == 0
    # its own two come after the histogram parameters and before B * Z
    assert "delta must be" in call(delta=0.0, acc=2)[1] and "bad histogram" in call(md=0.0, delta=0.0)[1]
    assert "accumulate" in call(acc=2, b=1 << 16, z=1 << 15)[1]
    for delta in (0.0, -0.04, float("nan"), float("inf")):
        rc, msg = call(delta=delta)
        assert rc == EINVAL and "delta must be positive" in msg, (delta, rc, msg)
    for acc in (2, -1):
        rc, msg = call(acc=acc)
        assert rc == EINVAL and "accumulate" in msg, (acc, rc, msg)
    rc, msg = call(b=1 << 16, z=1 << 15, nws=1 << 60)
    assert rc == ESHAPE and "too many zones" in msg, (rc, msg)
    assert lib.cfp_tof_zone_loss_ws_bytes(1 << 16, 1 << 15, 100) == 0 and lib.cfp_tof_zone_loss_ws_bytes(0, 4, 100) == 0
    rc, msg = call(ws=24)
    assert rc == EINVAL and "aligned" in msg, (rc, msg)
    rc, msg = call(nws=need - 1)
    assert rc == EINVAL and "too small" in msg, (rc, msg)
    rc, msg = call(z=5)                                    # the workspace of 4 zones
    assert rc == EINVAL and "too small" in msg, (rc, msg)
    with pytest.raises(RuntimeError, match=r"cfp_tof_zone_loss failed \(-2\)"):
        hip.call("cfp_tof_zone_loss", P, 8, 8, 8, 8, 1, 0, 1e-3, 10.0, P, P, P, 4, 4.0, 2000, 0.04, 20, 0.04, 1.0, 0, P, need, P, P, 0, 0)


def test_trainer_and_trainnet_take_the_weight():
    from cfpnet_amd import train_ops
    from cfpnet_amd.train_model import TrainNet
    from cfpnet_amd.trainer import Trainer
    fb = inspect.signature(TrainNet.forward_backward).parameters
    assert fb["w_zone"].default == 0.0 and fb["zone_target"].default is None and fb["silog"].default is True
    init = inspect.signature(Trainer.__init__).parameters
    assert init["w_zone"].default == 0.0 and init["zone_only"].default is False
    assert isinstance(Trainer.last_zone, property)
    for name in ("ZoneLoss", "zone_loss", "ZONE_LOSS_COLUMNS"):
        assert hasattr(train_ops, name), name
    fw = inspect.signature(train_ops.ZoneLoss.forward).parameters
    assert list(fw)[1:7] == ["pred", "raw_data", "rect_data", "mask", "lo", "hi"]
    assert fw["delta"].default is None and fw["grad_scale"].default == 1.0 and fw["grad_out"].default is None and fw["max_distance"].default == 4.0
    sd = {"w": torch.zeros(1)}
    with pytest.raises(ValueError, match="w_zone must be >= 0"):
        Trainer(sd, [], lr=1e-3, total_steps=2, device="cpu", w_zone=-1.0)
    with pytest.raises(ValueError, match="zone_only"):
        Trainer(sd, [], lr=1e-3, total_steps=2, device="cpu", zone_only=True)


def test_train_cli_pops_the_flags(monkeypatch):
    """`--w_zone F` and `--zone_only` are taken out of argv before the reference's flag table sees them, and reach the Trainer."""
    import train
    from cfpnet_amd import config, trainer
    assert "w_zone" not in vars(config.defaults()) and "zone_only" not in vars(config.defaults())        # not reference flags
    seen = {}

    class Stop(Exception):
        pass

    def fake_trainer(*a, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(trainer, "Trainer", fake_trainer)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)
    with pytest.raises(Stop):
        train.main(["--synthetic", "4", "--max_steps", "1", "--w_zone", "0.25", "--eager"])
    assert seen["w_zone"] == 0.25 and seen["zone_only"] is False and seen["zone_max_distance"] == 4.0 and seen["w_chamfer"] == 0.0
    seen.clear()
    with pytest.raises(Stop):
        train.main(["--synthetic", "4", "--max_steps", "1", "--w_zone", "0.5", "--zone_only", "--eager"])
    assert seen["w_zone"] == 0.5 and seen["zone_only"] is True
    seen.clear()
    with pytest.raises(Stop):
        train.main(["--synthetic", "4", "--max_steps", "1", "--eager"])
    assert seen["w_zone"] == 0.0 and seen["zone_only"] is False
    seen.clear()
    with pytest.raises(ValueError, match="--random_simu_max_d"):
        train.main(["--synthetic", "4", "--max_steps", "1", "--w_zone", "0.25", "--random_simu_max_d", "--eager"])
    with pytest.raises(ValueError, match="--zone_only needs --w_zone"):
        train.main(["--synthetic", "4", "--max_steps", "1", "--zone_only", "--eager"])
    assert not seen
    text = train.__doc__
    assert "--w_zone F" in text and "--zone_only" in text and "--random_simu_max_d" in text and "zone=" in text


def test_optimizer_state_carries_the_weight():
    """The weight is part of the checkpoint's optimizer entry; a resumed run with another weight is refused, after the chamfer check, and
    a checkpoint from before the flag counts as weight 0."""
    from cfpnet_amd.trainer import Trainer
    src = inspect.getsource(Trainer.optimizer_state_dict)
    assert '"w_zone": self.w_zone' in src and '"w_chamfer": self.w_chamfer' in src
    fmt = {"format": "cfpnet_amd.FlatAdamW/1"}
    t = Trainer.__new__(Trainer)
    t.w_chamfer, t.w_zone, t.zone_only = 0.0, 0.1, False
    with pytest.raises(ValueError, match="w_zone=0.0"):
        Trainer.load_optimizer_state_dict(t, dict(fmt, w_chamfer=0.0, w_zone=0.0))
    with pytest.raises(ValueError, match="w_zone"):
        Trainer.load_optimizer_state_dict(t, dict(fmt))                                   # a checkpoint from before the flag: weight 0
    with pytest.raises(ValueError, match="zone_only=True"):
        Trainer.load_optimizer_state_dict(t, dict(fmt, w_zone=0.1, zone_only=True))
    with pytest.raises(ValueError, match="w_chamfer"):                                    # the chamfer refusal comes first
        Trainer.load_optimizer_state_dict(t, dict(fmt, w_chamfer=0.3, w_zone=0.0))
    old = Trainer.__new__(Trainer)                                                        # an object with only w_chamfer set reads w_zone as 0
    old.w_chamfer = 0.0
    with pytest.raises(ValueError, match="w_zone=0.2"):
        Trainer.load_optimizer_state_dict(old, dict(fmt, w_zone=0.2))
