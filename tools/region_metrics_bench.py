#!/usr/bin/env python3
"""Graph-timed cost of one `cfp_eval_metrics_regions` call (B x 240x320 -> 480x640, the 8x8 zone grid with a third of the zones dropped)
without range edges (E = 0) and with two (E = 2), next to `cfp_eval_metrics` on the same tensors, in the same process:

    python tools/region_metrics_bench.py [--batch 8]

Prints one JSON line.  Measured on one MI355X (B = 8): DESIGN.md section 4.14."""
import argparse, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cfpnet_amd import metrics, synthetic
from cfpnet_amd.geometry import centered_zone_rects
from _gtime import graph_time_us

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
a = ap.parse_args()
B, H, W = a.batch, 480, 640
pairs = [synthetic.make_eval_pair(H, W, 240, 320, 700 + i, 0.1 * (i % 3), 0.15) for i in range(B)]
gt = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
pred = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
rect = torch.from_numpy(np.stack([centered_zone_rects(H, W, 8, 56)] * B)).cuda()
mask = torch.from_numpy(np.stack([np.random.default_rng(700 + i).random(64) >= 0.34 for i in range(B)])).cuda()
res = dict(batch=B, height=H, width=W)
rows = torch.empty(B, 10, dtype=torch.float64, device="cuda:0")
metrics.eval_metrics(pred, gt, 1e-3, 10.0, out=rows)
res["eval_metrics_us"] = graph_time_us(lambda: metrics.eval_metrics(pred, gt, 1e-3, 10.0, out=rows), calls=8, replays=6)
for name, edges in (("E0", ()), ("E2", (2.0, 4.0)), ("E7", (0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0))):
    out = metrics.region_metrics(pred, gt, 1e-3, 10.0, rect, mask, edges)
    res[f"region_metrics_us_{name}"] = graph_time_us(lambda: metrics.region_metrics(pred, gt, 1e-3, 10.0, rect, mask, edges, out=out), calls=8, replays=6)
    res[f"ratio_{name}"] = res[f"region_metrics_us_{name}"] / res["eval_metrics_us"]
# rectangles that are no integer grid take the loop over the rectangles (the definition); same pixels, same mask
rect_q = rect + 0.25
out = metrics.region_metrics(pred, gt, 1e-3, 10.0, rect_q, mask, (2.0, 4.0))
res["region_metrics_us_E2_rect_loop"] = graph_time_us(lambda: metrics.region_metrics(pred, gt, 1e-3, 10.0, rect_q, mask, (2.0, 4.0), out=out), calls=8, replays=6)
torch.cuda.synchronize()
full = metrics.region_metrics(pred, gt, 1e-3, 10.0, rect, mask, (2.0, 4.0)).cpu()
res["all_row_equals_eval_metrics_rel"] = float(((full[:, 0, 0, :9] - rows.cpu()[:, :9]).abs() / rows.cpu()[:, :9].abs()).max())
res["pixels_per_region"] = [float(v) for v in full[:, :, 0, 9].mean(0)]
print(json.dumps(res))
