#!/usr/bin/env python3
"""Graph-timed cost of one `cfp_unc_sparsification` call (B x 240x320 -> 480x640, K removal fractions) next to `cfp_eval_metrics` on
the same tensors and to one forward step of the default numerics mode (single-graph replay, uncertainty map on, no prob output):

    python tools/unc_metrics_bench.py [--batch 8] [--steps 20] [--no-forward]

Prints one JSON line.  Measured on one MI355X (B = 8, K = 20): DESIGN.md section 4.13."""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cfpnet_amd import metrics, synthetic
from _gtime import graph_time_us

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--no-forward", action="store_true")
a = ap.parse_args()
B, H, W, K = a.batch, 480, 640, a.steps
gt = torch.from_numpy(np.stack([synthetic.make_depth(H, W, seed=900 + i, holes=0.1 * (i % 3)) for i in range(B)])).cuda()
res = dict(batch=B, steps=K)
if a.no_forward:
    pred = torch.from_numpy(np.stack([synthetic.make_eval_pair(H, W, 240, 320, 700 + i, 0.1, 0.1)[1] for i in range(B)])).cuda()
    g = torch.Generator().manual_seed(3)
    unc = torch.rand(B, 3, 240, 320, generator=g).cuda()
else:
    from cfpnet_amd import spec, weights
    from cfpnet_amd.engine import Engine
    layers = spec.COMBINE1_LAYERS
    eng = Engine(weights.make_torch_state_dict(spec.model_manifest(layers)), layer_names=layers, device="cuda:0")
    inp = synthetic.to_device(synthetic.make_inputs(B), "cuda:0")
    eng.capture(inp, return_prob=False, uncertainty=True)
    out = eng.replay(inp)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        out = eng.replay(inp)
    torch.cuda.synchronize()
    res["forward_ms"] = (time.perf_counter() - t0) / 10 * 1e3
    pred, unc = out[1].clone(), out[3].clone()
rows = torch.empty(B, 10, dtype=torch.float64, device="cuda:0")
metrics.eval_metrics(pred, gt, 1e-3, 10.0, out=rows)
res["eval_metrics_us"] = graph_time_us(lambda: metrics.eval_metrics(pred, gt, 1e-3, 10.0, out=rows), calls=8, replays=6)
sp = metrics.sparsification(pred, unc, gt, 1e-3, 10.0, steps=K)
res["sparsification_us"] = graph_time_us(lambda: metrics.sparsification(pred, unc, gt, 1e-3, 10.0, steps=K, out=sp), calls=4, replays=5)
for k in (1, 100):
    spk = metrics.sparsification(pred, unc, gt, 1e-3, 10.0, steps=k)
    res[f"sparsification_us_K{k}"] = graph_time_us(lambda: metrics.sparsification(pred, unc, gt, 1e-3, 10.0, steps=k, out=spk), calls=4, replays=5)
noise = torch.rand(B, 3, 240, 320, generator=torch.Generator().manual_seed(3)).cuda()      # white-noise planes: no two lanes share a bin
res["sparsification_us_noise_planes"] = graph_time_us(lambda: metrics.sparsification(pred, noise, gt, 1e-3, 10.0, steps=K, out=sp), calls=4, replays=5)
sp = metrics.sparsification(pred, unc, gt, 1e-3, 10.0, steps=K, out=sp)
torch.cuda.synchronize()
res["ause_rmse_mean"] = [float(v) for v in sp["ause"][:, :, 0].nanmean(0)]
print(json.dumps(res))
