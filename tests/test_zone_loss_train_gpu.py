"""The zone-consistency term in the training step (`w_zone`): TrainNet, Trainer (eager and captured) and the step without ground truth
(`zone_only`).  Geometry of the training-step tests: 2 images of 256 x 320, 3 x 3 zones of 64 px.  The zone target is what
`TofSimulator` measures on the depth map.  The sensor's distance is 10 m here (250 bins), not train.py's 4 m: the untrained network
predicts about 5 m everywhere, beyond a 4 m sensor, and no zone would be compared."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import zone_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cfpnet_amd import spec, synthetic, tof, weights  # noqa: E402
from oracle import cfpnet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OFFS = {"cross_atten3": (3, 5), "cross_atten2": (7, 2), "cross_atten1": (11, 30)}
BIAS = "depth_head.regressor.4.bias"
MAX_D = 10.0
W = 0.5
_HIP, _SIM = {}, {}


def _sim(bound=0):
    if bound not in _SIM:
        cfg = types.SimpleNamespace(mode="train", train_zone_num=3, train_zone_random_offset=bound, simu_max_distance=MAX_D, zone_sample_num=16,
                                    sample_uniform=True)
        _SIM[bound] = tof.TofSimulator(cfg, DEV)
    return _SIM[bound]


def _measure(target, offsets=None):
    """What the sensor measured on the depth map -> the zone target of the step (device tensors)."""
    s = _sim(0 if offsets is None else 8).simulate(target.to(DEV), offsets=None if offsets is None else torch.tensor(offsets, dtype=torch.int32).to(DEV))
    return {"raw_data": s["fh"], "rect_data": s["rect_data"], "mask": s["mask"], "max_distance": MAX_D}


def _case(B=2, H=256, W_=320, zn=3, zpx=64, seed=11):
    layers = spec.COMBINE1_LAYERS
    sd = weights.make_torch_state_dict(spec.model_manifest(layers))
    inp = synthetic.make_inputs(B, H, W_, zn, zpx, seed=seed, drop_hist=0.25)
    target = torch.from_numpy(np.stack([synthetic.make_depth(H, W_, seed=seed + 5 + i, holes=0.1) for i in range(B)]))[:, None]
    return layers, sd, inp, target


def _hip_step(w, dtype=torch.float32):
    """(loss, zone value or None, gradients, zone table) of TrainNet.forward_backward with weight `w` (None: the call without the
    argument), once per (w, dtype)."""
    if (w, dtype) not in _HIP:
        from cfpnet_amd.train_model import TrainNet
        layers, sd, inp, target = _case()
        net = TrainNet(sd, layers, DEV, dtype=dtype)
        kw = {} if w is None else {"w_zone": w, "zone_target": _measure(target)}
        loss, _, _ = net.forward_backward(inp, target, target > 1e-3, pos_offsets=OFFS, **kw)
        torch.cuda.synchronize()
        zone = None if net.last_zone is None else float(net.last_zone)
        table = net._zone.zone.cpu().numpy() if zone is not None else None
        _HIP[(w, dtype)] = (loss.clone(), zone, {k: v.clone() for k, v in net.grads().items()}, table)
    return _HIP[(w, dtype)]


def _oracle_step(w, dtype):
    """float autograd of the oracle: SILog + w * the restatement's loss on its own prediction (run and weights held constant)."""
    layers, sd, inp, target = _case()
    zt = _measure(target)
    rect, mask, raw = zt["rect_data"].cpu().numpy(), zt["mask"].cpu().numpy().astype(np.uint8), zt["raw_data"].cpu().numpy()
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
        _, pred, _ = O.forward(sdg, i2, layer_names=layers, pos_offsets=OFFS, grad=True)
        silog = O.silog_loss(pred, target.to(dtype), target > 1e-3, interpolate=True)
        zl = R.torch_loss(pred, rect, mask, raw, target.shape[-2], target.shape[-1], 1e-3, 10.0, MAX_D, tof.AMBIENT_FLOOR)
        (silog + w * zl).backward()
    finally:
        O.BN_TRAIN = False
    grads = {k: v.grad.double() for k, v in sdg.items() if getattr(v, "grad", None) is not None}
    return float(silog.detach()), float(zl.detach()), grads


def test_weight_zero_is_the_step_without_the_argument():
    l_none, z_none, g_none, _ = _hip_step(None)
    l_zero, z_zero, g_zero, _ = _hip_step(0.0)
    assert z_none is None and z_zero is None                        # no launch, no value
    assert torch.equal(l_none, l_zero) and set(g_none) == set(g_zero)
    assert all(torch.equal(g_none[k], g_zero[k]) for k in g_none)


def test_step_with_the_term_matches_autograd_of_the_oracle():
    """Ground truth = float64 autograd of the oracle with 0.5 x the restatement's loss added; the HIP step must be as close to it as the
    float32 autograd of the same objective is (the comparative form and constants of the chamfer step test)."""
    s64, z64, g64 = _oracle_step(W, torch.float64)
    s32, z32, g32 = _oracle_step(W, torch.float32)
    loss, zl, gh, table = _hip_step(W)
    gh = {k: v.double().cpu() for k, v in gh.items()}
    compared = int(np.isfinite(table[..., R.R]).sum())
    print(f"silog f64 {s64:.7f} f32 {s32:.7f} hip {float(loss):.7f} | zone f64 {z64:.7f} f32 {z32:.7f} hip {zl:.7f} | compared zones {compared} of {table.shape[0] * table.shape[1]}")
    assert compared >= table.shape[0] * 3 and z64 > 0                            # the term is alive on this batch
    assert abs(float(loss) - s64) <= 2e-6 * abs(s64) + abs(s32 - s64)            # the returned loss stays the SILog scalar
    assert abs(zl - z64) <= 1e-4 * abs(z64) + abs(z32 - z64)                     # on the network's own float32 prediction
    live = {k for k, g in g64.items() if float(g.abs().max()) > 0}
    assert not sorted(live - set(gh)) and not [k for k in gh if k not in g64]
    gmax = max(float(g.abs().max()) for g in g64.values())
    names = sorted(live)
    den = {k: max(float(g64[k].abs().max()), 1e-5 * gmax) for k in names}
    e_hip = np.array([float((gh[k] - g64[k]).abs().max()) / den[k] for k in names])
    e_ref = np.array([float((g32[k] - g64[k]).abs().max()) / den[k] for k in names])
    order = np.argsort(-e_hip)[:6]
    print(f"gradient error vs f64: median hip {np.median(e_hip):.2e} / f32 autograd {np.median(e_ref):.2e}; "
          f"worst hip {[(names[i], f'{e_hip[i]:.1e}', f'{e_ref[i]:.1e}') for i in order]}")
    # a silently ignored term fails here: the weight moves this gradient by more than the step's own tolerance for it
    g0 = _hip_step(0.0)[2][BIAS].double().cpu()
    moved = float((gh[BIAS] - g0).abs().max()) / den[BIAS]
    print(f"{BIAS}: |g(w=0.5) - g(w=0)| / max|g64| = {moved:.3e}; its error vs f64 {e_hip[names.index(BIAS)]:.2e}")
    assert np.median(e_hip) <= 1.5 * np.median(e_ref) + 1e-4
    assert np.quantile(e_hip, 0.99) <= 3 * np.quantile(e_ref, 0.99) + 1e-3
    assert e_hip.max() < 0.15
    assert moved > 0.15


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, "f32x3"], ids=["bf16", "f16", "f32x3"])
def test_the_term_runs_in_every_training_numerics(dtype):
    """The loss maths is float32 / float64 in every mode: the zone value stays within 1 % of the float32 step's (the rule for the loss of
    the mixed-precision step), the SILog scalar is the one of the step without the term, and the head's bias gradient is finite and moved."""
    _, z32, _, _ = _hip_step(W)
    l0, _, g0, _ = _hip_step(None, dtype)
    l1, zl, g1, _ = _hip_step(W, dtype)
    print(f"{dtype}: zone {zl:.6f} vs float32 step {z32:.6f}")
    assert torch.equal(l0, l1)
    assert abs(zl - z32) < 1e-2 * z32
    assert bool(torch.isfinite(g1[BIAS]).all()) and not torch.equal(g0[BIAS], g1[BIAS])


def _batches(n, zero_target=False):
    out = []
    for s in range(n):
        i2 = synthetic.make_inputs(2, 256, 320, 3, 64, seed=70 + s, drop_hist=0.25 * (s % 2))
        t2 = torch.from_numpy(np.stack([synthetic.make_depth(256, 320, seed=90 + 2 * s + i, holes=0.1) for i in range(2)]))[:, None]
        zt = _measure(t2, offsets=[3 * s - 4, 5 - 2 * s])               # the rectangles move from batch to batch, as with --train_zone_random_offset
        i2 = synthetic.to_device(i2, DEV)
        i2["additional"].update(raw_data=zt["raw_data"], rect_data=zt["rect_data"], zone_mask=zt["mask"])
        o2 = {"cross_atten3": (s, 2 * s), "cross_atten2": (3 * s, s), "cross_atten1": (5 * s, 7 * s)}
        out.append((i2, torch.zeros_like(t2).cuda() if zero_target else t2.cuda(), o2))
    return out


@pytest.mark.parametrize("form", ["one_graph", "split", "segments"])
def test_captured_trainer_with_the_term_equals_the_eager_one(form):
    """Trainer(w_zone=0.5).capture() as one graph, split where the encoder's backward begins, and in segments with the parameter
    gradients beside them: three steps on changing inputs, targets and zone rectangles follow the eager trainer -- the rule of the
    captured-step test: losses within 1e-6, bit-identical parameters; and the zone value follows too."""
    from cfpnet_amd.trainer import Trainer
    layers, sd, _, _ = _case()
    batches = _batches(3)
    kw = dict(lr=3e-4, total_steps=20, w_zone=W, zone_max_distance=MAX_D)
    eager = Trainer(sd, layers, **kw)
    graph = Trainer(sd, layers, comm="off" if form == "split" else "overlap", **kw)
    graph.capture(*batches[0][:2], split=form == "split", wgrad_beside=form == "segments")
    assert (graph._graph2 is not None) == (form == "split") and (graph._segments is not None) == (form == "segments")
    zones = []
    for inp_b, tgt_b, offs_b in batches:
        l0, _, _ = eager.step(inp_b, tgt_b, pos_offsets=offs_b)
        l1, _, _ = graph.step(inp_b, tgt_b, pos_offsets=offs_b)
        torch.cuda.synchronize()
        z0, z1 = float(eager.last_zone), float(graph.last_zone)
        zones.append(z0)
        assert abs(float(l0) - float(l1)) <= 1e-6 * abs(float(l0)), (float(l0), float(l1))
        assert abs(z0 - z1) <= 1e-6 * abs(z0), (z0, z1)
        assert torch.equal(eager.net._zone.zone[..., 4:7], graph.net._zone.zone[..., 4:7])          # the same runs on the moved rectangles
    assert torch.equal(eager.flat.param, graph.flat.param)
    assert len(set(zones)) == 3 and all(np.isfinite(zones)) and min(zones) > 0          # it followed the changing targets


def test_zone_only_trains_without_ground_truth():
    """`zone_only` on a batch whose depth target is all zeros (SILog would be NaN): every gradient is finite, the returned loss is
    w_zone * L, and six captured steps on that fixed batch bring `last_zone` down."""
    from cfpnet_amd.trainer import Trainer
    layers, sd, _, _ = _case()
    inp, tgt, offs = _batches(1, zero_target=True)[0]
    assert not bool(tgt.any())
    tr = Trainer(sd, layers, lr=1e-3, total_steps=20, w_zone=W, zone_only=True, zone_max_distance=MAX_D)
    loss = tr._grads_to_flat(inp, tgt, offs)                          # the eager step up to the optimizer: look at the gradients
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.flat.grad).all()) and float(tr.flat.grad.abs().max()) > 0
    assert float(loss) == W * float(tr.last_zone) and np.isfinite(float(loss))
    tr.capture(inp, tgt)
    vals = []
    for _ in range(6):
        l, _, _ = tr.step(inp, tgt, pos_offsets=offs)
        torch.cuda.synchronize()
        vals.append(float(tr.last_zone))
        assert abs(float(l) - W * vals[-1]) <= 1e-6 * abs(vals[-1])
    print(f"zone_only: last_zone over six steps {[f'{v:.5f}' for v in vals]}")
    assert all(np.isfinite(vals)) and vals[-1] < vals[0]
    assert bool(torch.isfinite(tr.flat.param).all())
    with pytest.raises(ValueError, match="raw_data"):                 # a batch without the measurement is refused, not trained on SILog alone
        tr._zone_kw({"rgb": inp["rgb"], "additional": {k: v for k, v in inp["additional"].items() if k != "raw_data"}})


def test_train_cli_logs_the_term_and_refuses_a_resume_with_another_weight(tmp_path, capsys):
    """`train.py --w_zone 0.1 --simu_max_distance 10`: the step line shows `zone=` with a positive finite value, the checkpoint's optimizer
    entry carries the weight, and a resume without it is refused."""
    import train as train_cli
    common = ["@" + os.path.join(ROOT, "configs", "cfpnet_combine1.txt"), "--synthetic", "4", "--bs", "2", "--epochs", "2", "--log_every", "1", "--seed", "7",
              "--simu_max_distance", "10"]
    a, b = tmp_path / "a" / "w.pt", tmp_path / "b" / "w.pt"
    train_cli.main(common + ["--save", str(a), "--w_zone", "0.1", "--stop_after", "2"])
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("epoch ")]
    assert len(lines) == 2 and all(" zone=" in l and " loss " in l for l in lines), out[-600:]
    vals = [float(l.split("zone=")[1].split()[0]) for l in lines]
    assert all(np.isfinite(vals)) and min(vals) > 0, vals
    ck = str(a)[:-3] + ".ckpt.pt"
    opt = torch.load(ck, map_location="cpu", weights_only=False)["optimizer"]
    assert opt["w_zone"] == 0.1 and opt["zone_only"] is False
    with pytest.raises(ValueError, match="w_zone"):
        train_cli.main(common + ["--save", str(b), "--resume", ck])
