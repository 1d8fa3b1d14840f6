"""The training step in the f16x3 numerics (Trainer(dtype="f32x3"), TrainNet(dtype="f32x3"), Deltar(train_dtype="f32x3"),
train.py --dtype f32x3): float32 storage, every dense conv / Linear GEMM of the forward and of both gradients in split precision.
It must hold the FLOAT32 tape's bounds against float32 autograd of the oracle on the benched shard."""
import os
import sys

import numpy as np
import pytest
import torch

from cfpnet_amd import spec, synthetic, weights
from oracle import cfpnet_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from test_train_step_gpu import _SHARD_BOUNDS, _case, _flat, _shard_case  # noqa: E402  (the module pytest loaded: its shard cache is shared)


def test_config2_shard_b16_416x544_f32x3_training_step_vs_oracle():
    """16 crops of 416x544, 6x6 zones: loss, prediction and the gradient of every live tensor against float32 autograd of the oracle,
    within the float32 tape's bounds."""
    from cfpnet_amd.train_model import TrainNet
    c = _shard_case()
    net = TrainNet(c["sd"], c["layers"], "cuda:0", dtype="f32x3")
    loss, pred, _ = net.forward_backward(c["inp"], c["target"], c["target"] > 1e-3, pos_offsets=c["offs"])
    torch.cuda.synchronize()
    g = net.grads()
    ref = c["grads"]
    live = sorted(k for k, v in ref.items() if float(v.abs().max()) > 0)
    assert len(live) >= 413 and not sorted(set(live) - set(g))[:5] and not [k for k in g if k not in ref]
    a, b = _flat(g, live), _flat(ref, live)
    cos = float((a * b).sum() / (a.norm() * b.norm()))
    rms_max = max(float(ref[k].double().pow(2).mean().sqrt()) for k in live)
    rms_ok, worst = 0, []
    for k in live:
        r0 = float(ref[k].double().pow(2).mean().sqrt())
        r1 = float(g[k].double().pow(2).mean().sqrt())
        ok = abs(r1 - r0) <= 0.1 * r0 + 1e-6 * rms_max
        rms_ok += ok
        if not ok:
            worst.append((k, r0, r1))
    dl = abs(float(loss) - c["loss"]) / abs(c["loss"])
    dp = float((pred.double().cpu() - c["pred"]).abs().sum() / c["pred"].abs().sum())
    print(f"shard B=16 416x544 f32x3: loss {float(loss):.6f} vs oracle {c['loss']:.6f} (rel {dl:.2e}); pred relL1 {dp:.2e}; "
          f"full-gradient cosine {cos:.6f}; tensors with rms within 10 %: {rms_ok}/{len(live)}; off: {worst[:4]}")
    bl, bp, bc, br = _SHARD_BOUNDS[torch.float32]
    assert dl < bl and dp < bp and cos > bc and rms_ok >= br * len(live)
    del net
    torch.cuda.empty_cache()


def test_captured_f32x3_step_equals_the_eager_one():
    """Trainer(dtype="f32x3").capture(): the step with its batched operand packing and the device-side gradient scales, replayed as a
    graph with new inputs and windows per step, follows the eager f32x3 trainer bit for bit."""
    from cfpnet_amd.trainer import Trainer
    layers, sd, inp, target, offs = _case()
    batches = []
    for s in range(3):
        i2 = synthetic.make_inputs(2, 256, 320, 3, 64, seed=70 + s, drop_hist=0.25 * (s % 2))
        t2 = torch.from_numpy(np.stack([synthetic.make_depth(256, 320, seed=90 + 2 * s + i, holes=0.1) for i in range(2)]))[:, None]
        o2 = {"cross_atten3": (s, 2 * s), "cross_atten2": (3 * s, s), "cross_atten1": (5 * s, 7 * s)}
        batches.append((synthetic.to_device(i2, "cuda:0"), t2.cuda(), o2))
    eager = Trainer(sd, layers, lr=3e-4, total_steps=20, dtype="f32x3")
    graph = Trainer(sd, layers, lr=3e-4, total_steps=20, dtype="f32x3")
    graph.capture(*batches[0][:2])
    assert graph.net.packed and graph.net.packed_t            # the step's operands come from the one packing launch
    for inp_b, tgt_b, offs_b in batches:
        l0, _, _ = eager.step(inp_b, tgt_b, pos_offsets=offs_b)
        l1, _, _ = graph.step(inp_b, tgt_b, pos_offsets=offs_b)
        torch.cuda.synchronize()
        assert float(l0) == float(l1), (float(l0), float(l1))
    assert torch.equal(eager.flat.param, graph.flat.param)


def test_deltar_module_trains_in_f32x3_through_torch_autograd():
    """Deltar(train_dtype="f32x3"): `model(input)` in train mode + a torch loss + `loss.backward()` runs the f16x3 tape and gives the
    gradients of Trainer(dtype="f32x3") on the same batch; a default model keeps the float32 tape."""
    import types
    from cfpnet_amd.deltar import Deltar
    from cfpnet_amd.trainer import Trainer
    layers, sd, inp, target, offs = _case()
    args = types.SimpleNamespace(attention_layer=layers, zone_sample_num=16, change_embedding=True, no_skip_inside=False, hist_encoder_10x=True)
    model = Deltar(n_bins=256, min_val=1e-3, max_val=10.0, norm="linear", args=args, train_dtype="f32x3")
    assert Deltar(n_bins=256, min_val=1e-3, max_val=10.0, norm="linear", args=args).train_dtype is None
    model.load_state_dict(sd)
    model = model.to("cuda:0").train()
    dinp = synthetic.to_device(inp, "cuda:0")
    edges, pred = model(dinp, pos_offsets=offs)
    tgt = target.to("cuda:0")
    loss = O.silog_loss(torch.clip(pred, 1e-3), tgt, tgt > 1e-3, interpolate=True)
    loss.backward()
    torch.cuda.synchronize()
    tr = Trainer(sd, layers, lr=3e-4, total_steps=10, dtype="f32x3")
    assert tr.net.x3 and tr.dtype == torch.float32
    loss1 = tr._grads_to_flat(dinp, tgt, offs)
    torch.cuda.synchronize()
    assert abs(float(loss) - float(loss1)) < 1e-5 * float(loss1)
    named = dict(model.named_parameters())
    ref = {k: tr._to_torch[k](tr.flat.view(k, "grad")).cpu() for k in tr._to_torch}
    ref = {k: v for k, v in ref.items() if named[k].grad is not None}
    assert len(ref) >= 0.9 * len([p for p in named.values() if p.grad is not None])
    gmax = max(float(g.abs().max()) for g in ref.values())
    errs = [float((named[k].grad.cpu() - ref[k]).abs().max()) / max(float(ref[k].abs().max()), 1e-5 * gmax) for k in ref]
    # the same split-precision tape; the loss gradient comes from torch ops on one side and the SILog kernel on the other
    assert np.median(errs) < 2e-3 and max(errs) < 0.15, (np.median(errs), max(errs))
    # against the float32 tape of the default model: close, not equal
    a = torch.cat([named[k].grad.reshape(-1).double().cpu() for k in sorted(ref)])
    model32 = Deltar(n_bins=256, min_val=1e-3, max_val=10.0, norm="linear", args=args)
    model32.load_state_dict(sd)
    model32 = model32.to("cuda:0").train()
    _, pred32 = model32(dinp, pos_offsets=offs)
    O.silog_loss(torch.clip(pred32, 1e-3), tgt, tgt > 1e-3, interpolate=True).backward()
    n32 = dict(model32.named_parameters())
    b = torch.cat([n32[k].grad.reshape(-1).double().cpu() for k in sorted(ref)])
    cos = float((a * b).sum() / (a.norm() * b.norm()))
    assert cos > 0.9995 and not torch.equal(a, b), cos


def test_train_cli_f32x3_runs_and_its_loss_goes_down(capsys):
    import train as train_cli
    loss = train_cli.main(["@" + os.path.join(ROOT, "configs", "cfpnet_combine1.txt"), "--synthetic", "32", "--max_steps", "5", "--bs", "2",
                           "--dtype", "f32x3", "--log_every", "1", "--seed", "3"])
    out = capsys.readouterr().out
    losses = [float(line.split(" loss ")[1].split()[0]) for line in out.splitlines() if " loss " in line and line.startswith("epoch")]
    print(out)
    assert np.isfinite(loss) and len(losses) == 5, losses
    assert losses[-1] < losses[0], losses
