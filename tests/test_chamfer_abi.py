"""Bin-centre chamfer loss, the parts that need no GPU: the kernel's interval scheme (numpy, `chamfer_ref.interval_scheme`) against
brute force over the case table and random cases, the header's statement of the definition, argument validation of the entry point,
and the plumbing of the weight (`train.py --w_chamfer`, `Trainer`, `TrainNet`)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import chamfer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from cfpnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.load()


@pytest.mark.parametrize("name", list(R.CASES))
def test_interval_scheme_equals_brute_force_on_the_case_table(name):
    wn, target, mask = R.make_case(name)
    edges = torch.from_numpy(R.edges_from_widths(wn.numpy()))
    a, b = R.tie_margins(edges, target, mask)
    assert a > 1e-5 and b > 1e-5, (a, b)                      # the seeds of the table keep every case away from a tie
    L, Lb, g = R.chamfer_ref(edges, target, mask, torch.float64)
    Ls, Lbs, gs = R.interval_scheme(edges.numpy(), target.numpy(), None if mask is None else mask.numpy())
    assert abs(Ls - float(L)) <= 1e-12 * max(abs(float(L)), 1.0)
    assert np.abs(Lbs - Lb.numpy()).max() <= 1e-12 * max(float(Lb.abs().max()), 1.0)
    assert np.abs(gs - g.numpy()).max() <= 1e-12 * max(float(g.abs().max()), 1.0)
    if name == "empty_middle_image":
        assert Lbs[1] == 0.0 and not gs[1].any() and Lbs[0] > 0 and Lbs[2] > 0


def test_interval_scheme_equals_brute_force_on_random_cases():
    """300 small random cases, with the corners the scans can get wrong: P = 1, no valid pixel, every target below the first centre,
    above the last one, inside one bin."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for i in range(300):
        B, P, n = int(rng.integers(1, 4)), int(rng.choice([1, 2, 3, 7, 16, 40])), int(rng.integers(1, 60))
        w = rng.random((B, P)) + 0.1
        e = R.edges_from_widths((w / w.sum(1, keepdims=True)).astype(np.float32))
        kind = i % 6
        t = 0.2 + 9.7 * rng.random((B, 1, 1, n))
        if kind == 1:
            t = 1e-3 + 0.4 * (e[:, 1] - e[:, 0])[:, None, None, None] * rng.random((B, 1, 1, n))
        elif kind == 2:
            t = 10.2 + rng.random((B, 1, 1, n))
        elif kind == 3:
            j = int(rng.integers(0, P))
            t = e[:, j, None, None, None] + (e[:, j + 1] - e[:, j])[:, None, None, None] * rng.random((B, 1, 1, n))
        mask = rng.random((B, 1, 1, n)) < (0.0 if kind == 4 else 0.7)
        if kind == 5:
            mask[rng.integers(0, B)] = False
        e, t, m = torch.from_numpy(e), torch.from_numpy(t.astype(np.float32)), torch.from_numpy(mask)
        L, Lb, g = R.chamfer_ref(e, t, m, torch.float64)
        Ls, Lbs, gs = R.interval_scheme(e.numpy(), t.numpy(), m.numpy())
        a, b = R.tie_margins(e, t, m)
        if min(a, b) < 1e-9:             # an exact tie is decided by the tie rule, which brute-force argmin does not state
            continue
        worst = max(worst, abs(Ls - float(L)), float(np.abs(gs - g.numpy()).max()))
    assert worst <= 1e-11, worst


def test_header_states_the_definition_and_the_tie_rule():
    text = open(os.path.join(ROOT, "include", "cfpnet_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*size_t cfp_bins_chamfer_ws_bytes", text, flags=re.S)
    assert m, "cfp_bins_chamfer_ws_bytes has no comment in front of it"
    doc = " ".join(m.group(1).split())
    for needle in ("c_p = 0.5 (e_p + e_{p+1})", "(1/P) sum_p min_{t in T_b} (c_p - t)^2", "(1/N_b) sum_{t in T_b} min_p (c_p - t)^2",
                   "(1/B) sum_b L_b", "N_b = 0 contributes 0", "target >= 1e-3", "lower centre index wins", "lower target value wins",
                   "quantum 2^-40", "1 <= P <= 1024", "2^31", "strictly increasing"):
        assert needle in doc, needle


def test_argument_validation_is_reported_not_faulted(lib):
    from cfpnet_amd import hip
    ok = (16, 16, 0, 2, 4, 4, 8, 1.0)          # fake non-null pointers: every call below returns before anything is launched
    need = lib.cfp_bins_chamfer_ws_bytes(2, 4, 4, 8)
    assert need > 0
    assert lib.cfp_bins_chamfer(0, 16, 0, 2, 4, 4, 8, 1.0, 16, need, 16, 16, 0) == -1 and "null" in hip.last_error()
    assert lib.cfp_bins_chamfer(16, 16, 0, 2, 4, 4, 8, 1.0, 16, need, 0, 16, 0) == -1 and "null" in hip.last_error()
    assert lib.cfp_bins_chamfer(*ok[:3], 0, 4, 4, 8, 1.0, 16, need, 16, 16, 0) == -2 and "non-positive" in hip.last_error()
    for P in (0, 1025, -3):
        assert lib.cfp_bins_chamfer(*ok[:3], 2, 4, 4, P, 1.0, 16, need, 16, 16, 0) == -2 and "1..1024" in hip.last_error()
        assert lib.cfp_bins_chamfer_ws_bytes(2, 4, 4, P) == 0
    assert lib.cfp_bins_chamfer(*ok[:3], 2, 32768, 32768, 8, 1.0, 16, 1 << 40, 16, 16, 0) == -2 and "2^31" in hip.last_error()
    assert lib.cfp_bins_chamfer_ws_bytes(2, 32768, 32768, 8) == 0
    assert lib.cfp_bins_chamfer(*ok, 24, need, 16, 16, 0) == -1 and "aligned" in hip.last_error()
    assert lib.cfp_bins_chamfer(*ok, 16, need - 1, 16, 16, 0) == -1 and "too small" in hip.last_error()
    with pytest.raises(RuntimeError, match=r"cfp_bins_chamfer failed \(-2\)"):
        hip.call("cfp_bins_chamfer", 16, 16, 0, 2, 4, 4, 1025, 1.0, 16, need, 16, 16, 0)
    # the workspace grows with the slabs of partials: one per 4096 pixels of an image, 64 per image at the most
    assert lib.cfp_bins_chamfer_ws_bytes(1, 64, 64, 8) < lib.cfp_bins_chamfer_ws_bytes(1, 128, 64, 8)
    assert lib.cfp_bins_chamfer_ws_bytes(1, 4096, 4096, 8) == lib.cfp_bins_chamfer_ws_bytes(1, 4096, 2048, 8)


def test_trainer_and_trainnet_take_the_weight():
    from cfpnet_amd import train_ops
    from cfpnet_amd.train_model import TrainNet
    from cfpnet_amd.trainer import Trainer
    assert inspect.signature(TrainNet.forward_backward).parameters["w_chamfer"].default == 0.0
    assert inspect.signature(Trainer.__init__).parameters["w_chamfer"].default == 0.0
    assert isinstance(Trainer.last_chamfer, property)
    for name in ("BinsChamferLoss", "bins_chamfer"):
        assert hasattr(train_ops, name), name
    # the fold from a centre gradient to an edge gradient, and the module boundary's way back to the widths, are adjoint to
    # deltar.py:53-57 (edges = min + span * cumsum(widths), centres = edge midpoints)
    from cfpnet_amd.deltar import _edges_grad_to_widths
    torch.manual_seed(0)
    wn = torch.rand(2, 7, dtype=torch.float64, requires_grad=True)
    edges = torch.cat([torch.full((2, 1), 1e-3, dtype=torch.float64), 1e-3 + (10.0 - 1e-3) * wn.cumsum(1)], 1)
    centres = 0.5 * (edges[:, :-1] + edges[:, 1:])
    gc = torch.rand(2, 7, dtype=torch.float64)
    (centres * gc).sum().backward()
    ge = train_ops.centers_grad_to_edges(gc)
    assert ge.shape == (2, 8)
    assert torch.allclose(_edges_grad_to_widths(ge, 1e-3, 10.0), wn.grad, rtol=1e-12, atol=0)


def test_train_cli_pops_the_flag(monkeypatch):
    """`--w_chamfer F` is taken out of argv before the reference's flag table sees it, and reaches the Trainer."""
    import train
    from cfpnet_amd import config, trainer
    assert "w_chamfer" not in vars(config.defaults())             # not a reference flag
    seen = {}

    class Stop(Exception):
        pass

    def fake_trainer(*a, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(trainer, "Trainer", fake_trainer)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)
    with pytest.raises(Stop):
        train.main(["--synthetic", "4", "--max_steps", "1", "--w_chamfer", "0.25", "--eager"])
    assert seen["w_chamfer"] == 0.25
    seen.clear()
    with pytest.raises(Stop):
        train.main(["--synthetic", "4", "--max_steps", "1", "--eager"])
    assert seen["w_chamfer"] == 0.0


def test_optimizer_state_carries_the_weight():
    """The weight is part of the checkpoint's optimizer entry; a resumed run with another weight is refused."""
    from cfpnet_amd.trainer import Trainer
    src = inspect.getsource(Trainer.optimizer_state_dict)
    assert '"w_chamfer": self.w_chamfer' in src
    t = Trainer.__new__(Trainer)
    t.w_chamfer = 0.1
    with pytest.raises(ValueError, match="w_chamfer"):
        Trainer.load_optimizer_state_dict(t, {"format": "cfpnet_amd.FlatAdamW/1", "w_chamfer": 0.0})
    with pytest.raises(ValueError, match="w_chamfer"):
        Trainer.load_optimizer_state_dict(t, {"format": "cfpnet_amd.FlatAdamW/1"})       # a checkpoint from before the flag: weight 0
