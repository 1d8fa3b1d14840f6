"""The bin-centre chamfer term in the training step (`w_chamfer`): TrainNet, Trainer (eager and captured), the module boundary
(`bin_edges` differentiable, `train_ops.bins_chamfer`) and data-parallel training with the global-batch SILog.  Geometry of the
training-step tests: 2 images of 256 x 320."""
import os
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import chamfer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cfpnet_amd import spec, synthetic, weights  # noqa: E402
from oracle import cfpnet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OFFS = {"cross_atten3": (3, 5), "cross_atten2": (7, 2), "cross_atten1": (11, 30)}
BIAS = "depth_head.regressor.4.bias"
_HIP = {}


def _case(B=2, H=256, W=320, zn=3, zpx=64, seed=11):
    layers = spec.COMBINE1_LAYERS
    sd = weights.make_torch_state_dict(spec.model_manifest(layers))
    inp = synthetic.make_inputs(B, H, W, zn, zpx, seed=seed, drop_hist=0.25)
    target = torch.from_numpy(np.stack([synthetic.make_depth(H, W, seed=seed + 5 + i, holes=0.1) for i in range(B)]))[:, None]
    return layers, sd, inp, target


def _hip_step(w):
    """(loss, chamfer or None, gradients) of TrainNet.forward_backward with weight `w` (None: the call without the argument), once."""
    if w not in _HIP:
        from cfpnet_amd.train_model import TrainNet
        layers, sd, inp, target = _case()
        net = TrainNet(sd, layers, DEV)
        kw = {} if w is None else {"w_chamfer": w}
        loss, _, edges = net.forward_backward(inp, target, target > 1e-3, pos_offsets=OFFS, **kw)
        torch.cuda.synchronize()
        cham = None if net.last_chamfer is None else float(net.last_chamfer)
        _HIP[w] = (loss.clone(), cham, {k: v.clone() for k, v in net.grads().items()}, edges.clone())
    return _HIP[w]


def _oracle_step(w, dtype):
    """float autograd of the oracle: SILog + w * brute-force chamfer on its own bin edges."""
    layers, sd, inp, target = _case()
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
        edges, pred, _ = O.forward(sdg, i2, layer_names=layers, pos_offsets=OFFS, grad=True)
        silog = O.silog_loss(pred, target.to(dtype), target > 1e-3, interpolate=True)
        cham, _ = R.chamfer_of_centers(0.5 * (edges[:, :-1] + edges[:, 1:]), target, target > 1e-3)
        (silog + w * cham).backward()
    finally:
        O.BN_TRAIN = False
    grads = {k: v.grad.double() for k, v in sdg.items() if getattr(v, "grad", None) is not None}
    return float(silog.detach()), float(cham.detach()), grads


def test_weight_zero_is_the_step_without_the_argument():
    l_none, c_none, g_none, _ = _hip_step(None)
    l_zero, c_zero, g_zero, _ = _hip_step(0.0)
    assert c_none is None and c_zero is None                        # no launch, no value
    assert torch.equal(l_none, l_zero) and set(g_none) == set(g_zero)
    assert all(torch.equal(g_none[k], g_zero[k]) for k in g_none)


def test_step_with_the_term_matches_autograd_of_the_oracle():
    """Ground truth = float64 autograd of the oracle with 0.5 x the brute-force chamfer added; the HIP step must be as close to it as
    the float32 autograd of the same objective is (the comparative form and constants of the SILog-only step test)."""
    w = 0.5
    s64, c64, g64 = _oracle_step(w, torch.float64)
    s32, c32, g32 = _oracle_step(w, torch.float32)
    loss, cham, gh, _ = _hip_step(w)
    gh = {k: v.double().cpu() for k, v in gh.items()}
    print(f"silog f64 {s64:.7f} f32 {s32:.7f} hip {float(loss):.7f} | chamfer f64 {c64:.7f} f32 {c32:.7f} hip {cham:.7f}")
    assert abs(float(loss) - s64) <= 2e-6 * abs(s64) + abs(s32 - s64)          # the returned loss stays the SILog scalar
    assert abs(cham - c64) <= 1e-4 * abs(c64) + abs(c32 - c64)      # on the network's own float32 edges (pred: 1e-4 in the step test)
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
    """The bin maths is float32 in every mode: the chamfer value stays within 1 % of the float32 step's (the rule for the loss of the
    mixed-precision step), the SILog scalar is the one of the step without the term, and the head's bias gradient is finite and moved."""
    from cfpnet_amd.train_model import TrainNet
    layers, sd, inp, target = _case()
    _, c32, _, _ = _hip_step(0.5)
    grads, losses = [], []
    for kw in ({}, {"w_chamfer": 0.5}):
        net = TrainNet(sd, layers, DEV, dtype=dtype)
        loss, _, _ = net.forward_backward(inp, target, target > 1e-3, pos_offsets=OFFS, **kw)
        torch.cuda.synchronize()
        grads.append(net.grads()[BIAS].clone()); losses.append(loss.clone())
        cham = net.last_chamfer
    print(f"{dtype}: chamfer {float(cham):.6f} vs float32 step {c32:.6f}")
    assert torch.equal(losses[0], losses[1])
    assert abs(float(cham) - c32) < 1e-2 * c32
    assert bool(torch.isfinite(grads[1]).all()) and not torch.equal(grads[0], grads[1])


@pytest.mark.parametrize("form", ["one_graph", "split", "segments"])
def test_captured_trainer_with_the_term_equals_the_eager_one(form):
    """Trainer(w_chamfer=0.1).capture() as one graph, split where the encoder's backward begins, and in segments with the parameter
    gradients beside them: three steps on changing inputs and targets follow the eager trainer -- the rule of the captured-step test:
    losses within 1e-6, bit-identical parameters; and the chamfer value follows too."""
    from cfpnet_amd.trainer import Trainer
    layers, sd, _, _ = _case()
    batches = []
    for s in range(3):
        i2 = synthetic.make_inputs(2, 256, 320, 3, 64, seed=70 + s, drop_hist=0.25 * (s % 2))
        t2 = torch.from_numpy(np.stack([synthetic.make_depth(256, 320, seed=90 + 2 * s + i, holes=0.1) for i in range(2)]))[:, None]
        o2 = {"cross_atten3": (s, 2 * s), "cross_atten2": (3 * s, s), "cross_atten1": (5 * s, 7 * s)}
        batches.append((synthetic.to_device(i2, DEV), t2.cuda(), o2))
    eager = Trainer(sd, layers, lr=3e-4, total_steps=20, w_chamfer=0.1)
    graph = Trainer(sd, layers, lr=3e-4, total_steps=20, w_chamfer=0.1, comm="off" if form == "split" else "overlap")
    plain = Trainer(sd, layers, lr=3e-4, total_steps=20)
    graph.capture(*batches[0][:2], split=form == "split", wgrad_beside=form == "segments")
    assert (graph._graph2 is not None) == (form == "split") and (graph._segments is not None) == (form == "segments")
    chams = []
    for inp_b, tgt_b, offs_b in batches:
        l0, _, _ = eager.step(inp_b, tgt_b, pos_offsets=offs_b)
        l1, _, _ = graph.step(inp_b, tgt_b, pos_offsets=offs_b)
        plain.step(inp_b, tgt_b, pos_offsets=offs_b)
        torch.cuda.synchronize()
        c0, c1 = float(eager.last_chamfer), float(graph.last_chamfer)
        chams.append(c0)
        assert abs(float(l0) - float(l1)) <= 1e-6 * abs(float(l0)), (float(l0), float(l1))
        assert abs(c0 - c1) <= 1e-6 * abs(c0), (c0, c1)
    assert torch.equal(eager.flat.param, graph.flat.param)
    assert len(set(chams)) == 3 and all(np.isfinite(chams))          # it followed the changing targets
    assert plain.last_chamfer is None and not torch.equal(plain.flat.param, eager.flat.param)      # and the term trained something


@pytest.mark.parametrize("graphs", [False, True], ids=["eager_tape", "train_graphs"])
def test_module_path_bin_edges_are_differentiable(graphs):
    """The reference-shaped loop: `edges, pred = model.train()(x)`, `loss = silog(pred) + 0.1 * bins_chamfer(edges, tgt, mask)`,
    `loss.backward()`: the parameter gradients are those of TrainNet.forward_backward(w_chamfer=0.1), within the bound of the
    module-path test of the SILog-only step."""
    from cfpnet_amd import train_ops
    from cfpnet_amd.deltar import Deltar
    layers, sd, inp, target = _case()
    args = types.SimpleNamespace(attention_layer=layers, zone_sample_num=16, change_embedding=True, no_skip_inside=False, hist_encoder_10x=True)
    model = Deltar(n_bins=256, min_val=1e-3, max_val=10.0, norm="linear", args=args, dtype=torch.float32)
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    model.train_graphs = graphs
    tgt = target.to(DEV)
    for rep in range(2 if graphs else 1):                            # captured: the second pass is a replay with the buffers in use
        model.zero_grad()
        edges, pred = model(synthetic.to_device(inp, DEV), pos_offsets=OFFS)
        assert edges.requires_grad and pred.requires_grad and edges.shape == (2, 257)
        cham = train_ops.bins_chamfer(edges, tgt, tgt > 1e-3)
        loss = O.silog_loss(torch.clip(pred, 1e-3), tgt, tgt > 1e-3, interpolate=True) + 0.1 * cham
        loss.backward()
    torch.cuda.synchronize()
    assert graphs == bool(model._train_captures)
    l_ref, c_ref, ref, _ = _hip_step(0.1)
    assert abs(float(cham.detach()) - c_ref) <= 1e-6 * c_ref
    assert abs(float(loss.detach()) - (float(l_ref) + 0.1 * c_ref)) < 1e-5 * float(l_ref)
    named = dict(model.named_parameters())
    assert {k for k, p in named.items() if p.grad is not None} == set(ref)
    gmax = max(float(g.abs().max()) for g in ref.values())
    errs = {k: float((named[k].grad - ref[k]).abs().max()) / max(float(ref[k].abs().max()), 1e-5 * gmax) for k in ref}
    print(f"median {np.median(list(errs.values())):.2e} max {max(errs.values()):.2e} {BIAS} {errs[BIAS]:.2e}")
    assert np.median(list(errs.values())) < 2e-3 and max(errs.values()) < 0.15
    # a dropped edge gradient would leave the SILog-only gradient: farther from the reference than the bound
    g0 = _hip_step(0.0)[2]
    assert float((g0[BIAS] - ref[BIAS]).abs().max()) / max(float(ref[BIAS].abs().max()), 1e-5 * gmax) > 0.15
    # a loss on the edges alone also runs (no gradient reaches `pred`)
    model.zero_grad()
    edges, pred = model(synthetic.to_device(inp, DEV), pos_offsets=OFFS)
    train_ops.bins_chamfer(edges, tgt, tgt > 1e-3).backward()
    assert named[BIAS].grad is not None and bool(torch.isfinite(named[BIAS].grad).all()) and float(named[BIAS].grad.abs().max()) > 0


def test_train_cli_logs_the_term_and_refuses_a_resume_with_another_weight(tmp_path, capsys):
    """`train.py --w_chamfer 0.1`: the step line shows `chamfer=`, the checkpoint's optimizer entry carries the weight, a resume with the
    same weight runs on and one with another weight is refused."""
    import train as train_cli
    common = ["@" + os.path.join(ROOT, "configs", "cfpnet_combine1.txt"), "--synthetic", "4", "--bs", "2", "--epochs", "2", "--log_every", "1", "--seed", "7"]
    a, b = tmp_path / "a" / "w.pt", tmp_path / "b" / "w.pt"
    train_cli.main(common + ["--save", str(a), "--w_chamfer", "0.1", "--stop_after", "2"])
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("epoch ")]
    assert len(lines) == 2 and all(" chamfer=" in l and " loss " in l for l in lines), out[-600:]
    assert all(np.isfinite(float(l.split("chamfer=")[1].split()[0])) for l in lines)
    ck = str(a)[:-3] + ".ckpt.pt"
    assert torch.load(ck, map_location="cpu", weights_only=False)["optimizer"]["w_chamfer"] == 0.1
    with pytest.raises(ValueError, match="w_chamfer"):
        train_cli.main(common + ["--save", str(b), "--resume", ck])
    train_cli.main(common + ["--save", str(b), "--resume", ck, "--w_chamfer", "0.1"])
    assert "chamfer=" in capsys.readouterr().out


# ---------------------------------------------------------------- two ranks, global-batch SILog, the chamfer term on

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard(rank, B=2, H=256, W=320):
    inp = synthetic.make_inputs(B, H, W, 3, 64, seed=300 + rank, drop_hist=0.25)
    target = torch.from_numpy(np.stack([synthetic.make_depth(H, W, seed=400 + 10 * rank + i, holes=0.1) for i in range(B)]))[:, None]
    return inp, target


def _worker(rank, world, port, out, w):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from cfpnet_amd.trainer import Trainer
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    layers = spec.COMBINE1_LAYERS
    sd = weights.make_torch_state_dict(spec.model_manifest(layers))
    inp, target = _shard(rank)
    tr = Trainer(sd, layers, lr=3e-4, total_steps=20, device=DEV, dist=dist, world=world, comm="sequential", sync_loss=True, w_chamfer=w,
                 kernel_layout=False)
    loss = tr._grads_to_flat(synthetic.to_device(inp, DEV), target.cuda(), OFFS)          # the eager step up to the optimizer
    tr._reduce_group(None)
    torch.cuda.synchronize()
    torch.save({"loss": float(loss), "chamfer": float(tr.last_chamfer),
                "grads": {sg.name: tr.flat.view(sg.name, "grad").detach().cpu().clone() for sg in tr.flat.segments if sg.group != 2}}, f"{out}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_global_silog_and_chamfer_equal_the_concatenated_batch(tmp_path):
    """Two gloo ranks on one GPU, `sync_loss` and w_chamfer = 0.5, started as fresh child processes.  The gradient both ranks end up
    with must be the single-process gradient of the concatenated batch: ONE SILog over all four images, the chamfer mean over all four
    (so the per-rank chamfer gradient is NOT multiplied by the world size), each shard run through the network on its own, as a replica
    does (BatchNorm statistics are per replica in this trainer).  Bound: 1e-5 of the largest gradient entry, as for the global-batch
    SILog gradient over two ranks."""
    from cfpnet_amd import train_ops
    from cfpnet_amd.train_model import TrainNet
    world, w, out = 2, 0.5, str(tmp_path / "cham")
    mp.spawn(_worker, args=(world, _free_port(), out, w), nprocs=world, join=True)
    r = [torch.load(f"{out}.{k}", weights_only=False) for k in range(world)]
    assert all(torch.equal(r[0]["grads"][k], r[1]["grads"][k]) for k in r[0]["grads"])
    layers = spec.COMBINE1_LAYERS
    sd = weights.make_torch_state_dict(spec.model_manifest(layers))
    nets, tapes, preds, edges, tgts = [], [], [], [], []
    for k in range(world):
        inp, target = _shard(k)
        net = TrainNet(sd, layers, DEV)
        tape = net.new_tape()
        pred, e, (B, h, wd) = net.forward(tape, inp, OFFS)
        nets.append(net); tapes.append(tape); preds.append(pred); edges.append(e); tgts.append(target.to(DEV))
    tgt = torch.cat(tgts)
    crit, cham = train_ops.SILogLoss(), train_ops.BinsChamferLoss()
    loss = crit.forward(torch.cat([p.t.reshape(B, 1, h, wd) for p in preds]), tgt, tgt > 1e-3, interpolate=True)
    gp = crit.backward(1.0)
    c = cham.forward(torch.cat(edges), tgt, tgt > 1e-3, grad_scale=w)
    want = {}
    for k in range(world):
        preds[k].g = gp[k * B:(k + 1) * B].reshape(-1, 1).contiguous()
        tapes[k].acc(nets[k].centers, cham.grad_centers[k * B:(k + 1) * B].contiguous())
        tapes[k].backward()
        for n, g in nets[k].grads().items():
            want[n] = want[n] + g.cpu() if n in want else g.cpu().clone()
    torch.cuda.synchronize()
    assert abs(r[0]["loss"] - float(loss)) <= 2e-6 * abs(float(loss)) and r[0]["loss"] == r[1]["loss"]
    assert abs(0.5 * (r[0]["chamfer"] + r[1]["chamfer"]) - float(c)) <= 2e-6 * float(c)          # the mean over ranks is the global mean
    assert set(want) == set(r[0]["grads"])
    gmax = max(float(g.abs().max()) for g in want.values())
    worst = max(float((r[0]["grads"][n].reshape(want[n].shape) - want[n]).abs().max()) for n in want)
    print(f"two ranks vs concatenated batch: worst |diff| {worst:.3e}, largest gradient entry {gmax:.3e}")
    assert worst <= 1e-5 * gmax
