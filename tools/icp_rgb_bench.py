#!/usr/bin/env python3
"""Graph-timed cost of one `cfp_icp_rgb_step` next to one `cfp_icp_step` on the same inputs in the same run (a 240x320 prediction and its
std seen at 480x640, against a 480x640 raycast of the coloured 256^3 room of tools/icp_bench.py with normals and std, and for the
photometric half the frame's luminance and the luminance of the shaded raycast) at strides 1, 2 and 4, and of the two `cfp_luma`
layouts that feed it:

    python tools/icp_rgb_bench.py [--batch 1] [--dim 256]

The protocol is tools/icp_bench.py's: six sets of inputs rotate, so that back-to-back launches do not find their data in the 256 MiB
Infinity Cache; every figure is taken three times (each a graph of 12 calls replayed 20 times), the median is reported and the three are
listed.  The step with the image reads 4 more bytes per pixel of the stride grid for the frame's luminance and the four taps of the
model's (neighbours of the depth gather: the same lines), and carries 60 double accumulators instead of 30.  Prints one JSON line.
Measured on one MI355X: DESIGN.md section 4.33."""
import argparse, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cfpnet_amd import hip, pointcloud, render, synthetic, tracking, tsdf
from _gtime import graph_time_us

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--dim", type=int, default=256)
a = ap.parse_args()
B, D, h, w, H, W, NB = a.batch, a.dim, 240, 320, 480, 640, 6
DEV = "cuda:0"
VOXEL = 0.02
pred = torch.from_numpy(np.stack([synthetic.make_eval_pair(H, W, h, w, 700 + i, 0.0, 0.02)[1] for i in range(B)])).to(DEV)
unc = torch.rand(B, 3, h, w, device=DEV) * 0.05 + 0.02
K = torch.tensor([pointcloud.ZJUL5_INTRINSICS] * B, dtype=torch.float32, device=DEV)
# the camera and the start pose of tools/icp_bench.py: a degree and a centimetre apart
T = torch.tensor([[0.99997, -0.003, -0.006, 0.012, 0.003, 0.99999, -0.004, -0.006, 0.006, 0.004, 0.99997, 0.009]] * B, dtype=torch.float32,
                 device=DEV).reshape(B, 3, 4)
T0 = torch.tensor([[0.99985, -0.004, 0.017, 0.010, 0.004, 0.99999, 0.002, -0.005, -0.017, -0.002, 0.99985, 0.008]] * B, dtype=torch.float32,
                  device=DEV).reshape(B, 3, 4)
# a smooth picture, periods of 40 to 90 pixels, normalised like the model's input
yy, xx = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float32), torch.arange(W, device=DEV, dtype=torch.float32), indexing="ij")
c = torch.stack([0.5 + 0.2 * torch.sin(xx / 9.0 + 0.3 * k) + 0.15 * torch.sin(yy / 7.0 + xx / 14.0 + k) for k in range(3)])
mean, std = (torch.tensor(v, device=DEV).view(3, 1, 1) for v in (render.IMAGENET_MEAN, render.IMAGENET_STD))
rgb = ((c - mean) / std).expand(B, 3, H, W).contiguous()
origin = (-0.5 * D * VOXEL, -0.5 * D * VOXEL, 0.3)
res = dict(batch=B, dims=[D, D, D], voxel=VOXEL, height=H, width=W)
k = [0]


def timed(fn):
    runs = sorted(graph_time_us(fn, calls=12, replays=20) for _ in range(3))
    return runs[1], runs


vols = [tsdf.TsdfVolume((D, D, D), VOXEL, origin, K, size=(H, W)) for _ in range(NB)]
preds, uncs, rgbs = [pred.clone() for _ in range(NB)], [unc.clone() for _ in range(NB)], [rgb.clone() for _ in range(NB)]
for v in vols:
    v.integrate_rgb(pred, rgb, unc, T)
models = [tuple(t.clone() for t in v.raycast(T, normals=True)) for v in vols]
shades = [v.shade(m[0], T).clone() for v, m in zip(vols, models)]
torch.cuda.synchronize()
res["model_hit"] = float((~torch.isnan(models[0][0])).float().mean())
res["model_coloured"] = float((~torch.isnan(shades[0][..., 0])).float().mean())

lumas = [torch.empty(B, H, W, device=DEV) for _ in range(NB)]
m3, s3 = render._three(render.IMAGENET_MEAN, "mean"), render._three(render.IMAGENET_STD, "std")
for name, layout, srcs in (("luma_planar", 0, rgbs), ("luma_interleaved", 1, shades)):
    def run_luma():
        i = k[0] % NB; k[0] += 1
        hip.call("cfp_luma", srcs[i].data_ptr(), layout, m3 if layout == 0 else None, s3 if layout == 0 else None, H, W, B,
                 lumas[i].data_ptr(), hip.current_stream())

    t, ts = timed(run_luma)
    nbytes = 16.0 * B * H * W                            # 12 read, 4 written
    res[name] = dict(us=t, runs_us=ts, mbytes=nbytes / 1e6, gb_per_s=nbytes / t / 1e3)

for stride in (1, 2, 4):
    args = lambda i: (preds[i], K, models[i][0], models[i][2], T0, uncs[i], models[i][1], None, (H, W))
    geo = [tracking.icp(*args(i), iters=1, stride=stride) for i in range(NB)]
    col = [tracking.icp_rgb(*args(i), iters=1, stride=stride, rgb=rgbs[i], model_rgb=shades[i]) for i in range(NB)]
    # the step alone: the luminance planes are computed once per `icp_rgb` call, not per step, and are timed above
    planes = [(o.src_luma.clone(), o.mdl_luma.clone()) for o in col]
    col = [tracking.icp_rgb(*args(i), iters=1, stride=stride, rgb=planes[i][0], model_rgb=planes[i][1]) for i in range(NB)]
    torch.cuda.synchronize()
    sg, sc = geo[0].stats[0].cpu().numpy(), col[0].stats[0].cpu().numpy()

    def run_geo():
        i = k[0] % NB; k[0] += 1
        tracking.icp(*args(i), iters=1, stride=stride, out=geo[i])

    def run_col():
        i = k[0] % NB; k[0] += 1
        tracking.icp_rgb(*args(i), iters=1, stride=stride, rgb=planes[i][0], model_rgb=planes[i][1], out=col[i])

    (tg, tgs), (tc, tcs) = timed(run_geo), timed(run_col)
    ns = -(-H // stride) * -(-W // stride)
    res[f"step_stride{stride}"] = dict(icp_us=tg, icp_runs_us=tgs, icp_rgb_us=tc, icp_rgb_runs_us=tcs, rgb_over_geometry=tc / tg, pixels=B * ns,
                                       pairs=float(sg[:, 0].sum()), photo_pairs=float(sc[:, 6].sum()), accepted=float(sc[:, 5].min()),
                                       same_geometric_pairs=bool((sg[:, 0] == sc[:, 0]).all()))
torch.cuda.synchronize()
print(json.dumps(res))
