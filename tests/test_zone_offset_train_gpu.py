"""Training with per-sample ToF zone offsets (`--train_zone_random_offset`): TrainNet / Trainer with zone_offset_bound > 0 read
the batch's zone rectangle from device records, so one captured step serves every offset draw.  Checked against float64
autograd of the oracle, against the eager step, against the static path, and through train.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from cfpnet_amd import geometry, spec, synthetic, weights
from oracle import cfpnet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

H, W, ZN, ZP = 256, 320, 3, 64
LAYOUT = (ZN, ZP, int((H - ZP * ZN) / 2), int((W - ZP * ZN) / 2))
POS = {"cross_atten3": (3, 5), "cross_atten2": (7, 2), "cross_atten1": (11, 30)}


def _batch(offsets, seed=11):
    """A synthetic batch whose sample b has its zone grid shifted by offsets[b] (rect_data and the collated patch_info)."""
    B = len(offsets)
    inp = synthetic.make_inputs(B, H, W, ZN, ZP, seed=seed, drop_hist=0.25)
    pi = geometry.offsets_patch_info(offsets, LAYOUT, (H, W))
    patch_info = {s: {k: torch.from_numpy(v) for k, v in pi[s].items()} for s in (4, 8, 16)}
    patch_info["zone_num"] = torch.from_numpy(pi["zone_num"])
    inp["additional"]["patch_info"] = patch_info
    inp["additional"]["rect_data"] = torch.from_numpy(np.stack([geometry.centered_zone_rects(H, W, ZN, ZP, int(o)) for o in offsets]))
    target = torch.from_numpy(np.stack([synthetic.make_depth(H, W, seed=seed + 5 + i, holes=0.1) for i in range(B)]))[:, None]
    return inp, target


def _oracle_step(sd, inp, target, dtype):
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    sdg = {}
    for k, v in sd.items():
        v = v.detach().clone()
        if v.is_floating_point():
            v = v.to(dtype)
            if not k.endswith(("running_mean", "running_var")):
                v.requires_grad_(True)
        sdg[k] = v
    cast = lambda x: x.to(dtype) if torch.is_tensor(x) and x.is_floating_point() else x
    i2 = {"rgb": cast(inp["rgb"]), "additional": {k: cast(v) for k, v in inp["additional"].items()}}
    O.BN_TRAIN = True
    try:
        edges, pred, prob = O.forward(sdg, i2, layer_names=spec.COMBINE1_LAYERS, pos_offsets=POS, grad=True)
        loss = O.silog_loss(pred, target.to(dtype), target > 1e-3, interpolate=True)
        loss.backward()
    finally:
        O.BN_TRAIN = False
    grads = {k: v.grad.double() for k, v in sdg.items() if getattr(v, "grad", None) is not None}
    return float(loss.detach()), pred.detach().double(), grads


# all equal and non-zero; different (a widened union: the bilinear regroup); a rectangle overhanging the image (-40 < -sy0 = -32)
DRAWS = {"equal": (5, 5), "different": (-7, 9), "overhang": (-40, -3)}


@pytest.mark.parametrize("draw", list(DRAWS), ids=list(DRAWS))
def test_dynamic_geometry_step_matches_autograd_of_the_oracle(draw):
    """Tolerance rule of test_training_step_matches_autograd_of_the_oracle: the float32 HIP step must be as close to float64
    autograd of the oracle (which reduces the collated patch_info the reference's way) as float32 autograd of the oracle is."""
    from cfpnet_amd.train_model import TrainNet
    sd = weights.make_torch_state_dict(spec.model_manifest(spec.COMBINE1_LAYERS))
    inp, target = _batch(DRAWS[draw])
    loss64, pred64, g64 = _oracle_step(sd, inp, target, torch.float64)
    loss32, _, g32 = _oracle_step(sd, inp, target, torch.float32)
    net = TrainNet(sd, spec.COMBINE1_LAYERS, "cuda:0", zone_offset_bound=40)
    loss1, pred1, _ = net.forward_backward(inp, target, target > 1e-3, pos_offsets=POS)
    torch.cuda.synchronize()
    gh = {k: v.double().cpu() for k, v in net.grads().items()}
    print(f"{draw}: loss f64 {loss64:.7f}  f32 oracle {loss32:.7f}  hip {float(loss1):.7f}")
    assert abs(float(loss1) - loss64) <= 2e-6 * abs(loss64) + abs(loss32 - loss64)
    assert float((pred1.double().cpu() - pred64).abs().max()) <= 1e-4 * float(pred64.abs().max())
    live = {k for k, g in g64.items() if float(g.abs().max()) > 0}
    assert not sorted(live - set(gh)), sorted(live - set(gh))[:10]
    assert not [k for k in gh if k not in g64]
    gmax = max(float(g.abs().max()) for g in g64.values())
    e_hip, e_ref = [], []
    for k in sorted(live):
        den = max(float(g64[k].abs().max()), 1e-5 * gmax)
        e_hip.append(float((gh[k] - g64[k]).abs().max()) / den)
        e_ref.append(float((g32[k] - g64[k]).abs().max()) / den)
    e_hip, e_ref = np.array(e_hip), np.array(e_ref)
    print(f"median hip {np.median(e_hip):.2e} / f32 autograd {np.median(e_ref):.2e}; worst hip {e_hip.max():.2e}")
    assert np.median(e_hip) <= 1.5 * np.median(e_ref) + 1e-4
    assert np.quantile(e_hip, 0.99) <= 3 * np.quantile(e_ref, 0.99) + 1e-3
    assert e_hip.max() < 0.15


@pytest.mark.parametrize("form", ["graph", "split", "wgrad_beside"])
def test_captured_dynamic_step_follows_the_eager_one(form):
    """One capture, fed batches with different offset draws (different rectangles, extents and inside counts): the replayed
    step follows the eager Trainer -- losses to 1e-6, parameters bit-identical."""
    from cfpnet_amd.trainer import Trainer
    sd = weights.make_torch_state_dict(spec.model_manifest(spec.COMBINE1_LAYERS))
    batches = []
    for s, offs in enumerate([(0, 0), (-8, 6), (7, 7), (-8, -8)]):
        inp, tgt = _batch(offs, seed=70 + s)
        o2 = {"cross_atten3": (s, 2 * s), "cross_atten2": (3 * s, s), "cross_atten1": (5 * s, 7 * s)}
        batches.append((synthetic.to_device(inp, "cuda:0"), tgt.cuda(), o2, offs))
    kw = dict(lr=3e-4, total_steps=20, zone_offset_bound=8, zone_layout=LAYOUT)
    eager, graph = Trainer(spec_sd(sd), spec.COMBINE1_LAYERS, **kw), Trainer(spec_sd(sd), spec.COMBINE1_LAYERS, **kw)
    graph.capture(*batches[1][:2], split=form == "split", wgrad_beside=form == "wgrad_beside")
    for inp_b, tgt_b, pos_b, offs in batches:
        l0, _, _ = eager.step(inp_b, tgt_b, pos_offsets=pos_b, zone_offsets=offs)
        l1, _, _ = graph.step(inp_b, tgt_b, pos_offsets=pos_b, zone_offsets=offs)
        torch.cuda.synchronize()
        assert abs(float(l0) - float(l1)) <= 1e-6 * abs(float(l0)), (offs, float(l0), float(l1))
    assert torch.equal(eager.flat.param, graph.flat.param)


def spec_sd(sd):
    return {k: v.clone() for k, v in sd.items()}


def test_dynamic_path_with_zero_offsets_matches_the_static_path():
    """All-zero offsets: the crop / paste weights are exactly 1 / 0; only DAPM's key buffer (capacity rows, device count) and its
    split differ -- float32 summation-order noise, amplified by batch-statistics BatchNorm."""
    from cfpnet_amd.train_model import TrainNet
    sd = weights.make_torch_state_dict(spec.model_manifest(spec.COMBINE1_LAYERS))
    inp, target = _batch((0, 0))
    st = TrainNet(sd, spec.COMBINE1_LAYERS, "cuda:0")
    dy = TrainNet(sd, spec.COMBINE1_LAYERS, "cuda:0", zone_offset_bound=8)
    l0, p0, _ = st.forward_backward(inp, target, target > 1e-3, pos_offsets=POS)
    l1, p1, _ = dy.forward_backward(inp, target, target > 1e-3, pos_offsets=POS)
    torch.cuda.synchronize()
    assert abs(float(l0) - float(l1)) <= 1e-5 * abs(float(l0))
    assert float((p0 - p1).abs().max()) <= 1e-5 * float(p0.abs().max())
    g0, g1 = st.grads(), dy.grads()
    assert set(g0) == set(g1)
    gmax = max(float(g.abs().max()) for g in g0.values())
    errs = np.array([float((g1[k] - g0[k]).abs().max()) / max(float(g0[k].abs().max()), 1e-5 * gmax) for k in g0])
    print(f"dynamic vs static: median {np.median(errs):.2e} max {errs.max():.2e}")
    assert np.median(errs) < 1e-4 and errs.max() < 2e-2


def _train_losses(tmp_path, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "@" + os.path.join(ROOT, "configs", "cfpnet_combine1.txt"), "--synthetic", "32",
           "--max_steps", "3", "--train_zone_random_offset", "8", "--seed", "5", "--log_every", "1", *extra]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    losses = [float(m) for m in re.findall(r"step \d+/\d+ loss ([-\d.naninf]+)", r.stdout)]
    assert len(losses) == 3 and all(np.isfinite(losses)), r.stdout[-2000:]
    return losses


@pytest.mark.parametrize("mode", ["captured", "eager"])
def test_train_cli_with_random_zone_offsets(tmp_path, mode):
    extra = ("--eager",) if mode == "eager" else ()
    a = _train_losses(tmp_path, *extra)
    b = _train_losses(tmp_path, *extra)
    print(mode, a)
    assert a == b


def test_deltar_module_captures_once_for_per_sample_rectangles():
    """A reference-style loop (model(input_data) in .train(), loss.backward(), torch AdamW) on a Deltar built with
    train_zone_random_offset > 0, fed batches whose samples have different grid offsets: the training graphs capture once and
    follow the launch-by-launch loop exactly."""
    import types
    from cfpnet_amd.deltar import Deltar
    sd = weights.make_torch_state_dict(spec.model_manifest(spec.COMBINE1_LAYERS))
    args = types.SimpleNamespace(attention_layer=spec.COMBINE1_LAYERS, zone_sample_num=16, change_embedding=True, no_skip_inside=False,
                                 hist_encoder_10x=True, train_zone_random_offset=8)
    batches = []
    for s, offs in enumerate([(3, -5), (-8, 8), (6, 6)]):
        inp, tgt = _batch(offs, seed=170 + s)
        o2 = {"cross_atten3": (s, 2 * s), "cross_atten2": (3 * s, s), "cross_atten1": (5 * s, 7 * s)}
        batches.append((synthetic.to_device(inp, "cuda:0"), tgt.cuda(), o2))
    results = []
    for graphs in (False, True):
        model = Deltar(n_bins=256, min_val=1e-3, max_val=10.0, norm="linear", args=args, dtype=torch.float32)
        model.load_state_dict(sd)
        model = model.to("cuda:0").train()
        model.train_graphs = graphs
        opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.1)
        losses, caps = [], set()
        for dinp, tgt, o2 in batches:
            opt.zero_grad()
            edges, pred = model(dinp, pos_offsets=o2)
            loss = O.silog_loss(torch.clip(pred, 1e-3), tgt, tgt > 1e-3, interpolate=True)
            loss.backward()
            opt.step()
            losses.append(float(loss))
            caps.update(id(c) for c in model._train_captures.values())
        torch.cuda.synchronize()
        assert len(caps) == (1 if graphs else 0)
        results.append((losses, {k: v.detach().clone() for k, v in model.state_dict().items()}))
    (l0, s0), (l1, s1) = results
    assert l0 == l1, (l0, l1)
    assert all(torch.equal(s0[k], s1[k]) for k in s0), [k for k in s0 if not torch.equal(s0[k], s1[k])][:5]
