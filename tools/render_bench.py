#!/usr/bin/env python3
"""Graph-timed cost of `render.demo_panel` (B x 240x320 prediction -> B x 960x1280 panel: five launches into one canvas) next to the host
restatement of the same panel -- numpy with matplotlib's tables, tests/render_ref.py -- which starts with the device-to-host copy of the
float32 prediction, as the reference's `colorize` path does:

    python tools/render_bench.py [--batch 8] [--host_images 2]

The kernels move about 1 MB per image and piece, so they are bound by their launches, not by HBM; the point of the pair is that the
prediction no longer crosses to the host as float32 and comes back as a picture.  The host side is timed on `--host_images` images and
scaled to the batch.  Prints one JSON line.  Measured on one MI355X (B = 8): DESIGN.md section 4.18."""
import argparse, json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cfpnet_amd import render, synthetic
from _gtime import graph_time_us
import render_ref as R

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--host_images", type=int, default=2)
a = ap.parse_args()
B, h, w, H, W = a.batch, 240, 320, 480, 640
DEV = "cuda:0"
pairs = [synthetic.make_eval_pair(H, W, h, w, 700 + i, 0.1, 0.15) for i in range(B)]
pred = torch.from_numpy(np.stack([p[1] for p in pairs])).to(DEV)
gt = torch.from_numpy(np.stack([p[0] for p in pairs])).to(DEV)
inp = synthetic.to_device(synthetic.make_inputs(B, seed=9, drop_hist=0.2), DEV)
add = inp["additional"]
canvas = torch.empty(B, 2 * H, 2 * W, 3, dtype=torch.uint8, device=DEV)


def panel():
    render.demo_panel(inp["rgb"], pred, add["hist_data"], add["rect_data"], add["mask"], gt, out=canvas)


def piece(fn):
    return graph_time_us(fn, calls=12, replays=5)


res = dict(batch=B, height=H, width=W, panel_us=piece(panel))
small = torch.empty(B, H, W, 3, dtype=torch.uint8, device=DEV)
res["depth_us"] = piece(lambda: render.depth_image(pred, (H, W), out=small))
res["error_us"] = piece(lambda: render.error_image(pred, gt, out=small))
res["rgb_us"] = piece(lambda: render.rgb_image(inp["rgb"], out=small))
res["zones_us"] = piece(lambda: render.zones_overlay(small, add["hist_data"], add["rect_data"], add["mask"], 1e-3, 10.0))
torch.cuda.synchronize()

# the host restatement of the same panel, from the device-to-host copy of the float32 prediction on
try:
    import matplotlib
    table = lambda n: np.ascontiguousarray(matplotlib.colormaps[n](np.arange(256), bytes=True)[:, :3])
    res["host_tables"] = "matplotlib"
except ImportError:
    table = render.colormap_table
    res["host_tables"] = "cfpnet_amd/colormaps.py"
n = max(1, min(a.host_images, B))
t0 = time.perf_counter()
p_host = pred[:n].cpu().numpy()
torch.cuda.synchronize()
g_host, x_host = gt[:n].cpu().numpy(), inp["rgb"][:n].cpu().numpy()
hist, rect, mask = (add[k][:n].cpu().numpy() for k in ("hist_data", "rect_data", "mask"))
magma, jet = table("magma_r"), table("jet")
host = np.empty((n, 2 * H, 2 * W, 3), np.uint8)
for b in range(n):
    host[b, :H, :W] = R.render_rgb(x_host[b])
    host[b, :H, W:] = R.render_zones(host[b, :H, :W], hist[b], rect[b], mask[b], 1e-3, 10.0, magma, 160)
    host[b, H:, :W] = R.render_depth(p_host[b], None, H, W, 1, R.DEPTH, 1e-3, 10.0, magma)
    host[b, H:, W:] = R.render_depth(p_host[b], g_host[b], H, W, 1, R.ABS_ERR, 0.0, 1.0, jet)
res["host_us"] = (time.perf_counter() - t0) / n * B * 1e6
res["host_images_timed"] = n
panel()
res["panel_pixels_equal_to_host"] = float((canvas[:n].cpu().numpy() == host).all(-1).mean())
print(json.dumps(res))
