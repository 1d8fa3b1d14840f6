#!/usr/bin/env python3
"""Graph-timed cost of one `cfp_icp_step` (a 240x320 prediction and its std seen at 480x640, against a 480x640 raycast of the 256^3
room of tools/tsdf_bench.py with normals and std) at strides 1, 2 and 4, of the `cfp_tsdf_raycast` that feeds it, and of one full
`Tracker.update` (raycast, ten steps, pose copy, integrate), next to a device copy that moves the same number of bytes under the same
protocol:

    python tools/icp_bench.py [--batch 1] [--dim 256]

Bytes counted for a step (read, the algorithmic minimum; it writes one row of 240 bytes per workgroup): the prediction and its std plane
once (8 bytes per prediction pixel; at a stride the taps of the pixels used, at most that), and 20 bytes per pixel of the stride grid
(model depth, normal, std at the pixel it projects to).  The step is a gather and a reduction, not a stream: the copy is the yardstick
for "what would these bytes cost", not a target.  Six sets of inputs rotate, so that back-to-back launches do not find their data in the
256 MiB Infinity Cache.  Every figure is taken three times (each a graph of 12 calls replayed 20 times); the median is reported and the
three are listed.  Prints one JSON line.  Measured on one MI355X: DESIGN.md section 4.30."""
import argparse, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cfpnet_amd import pointcloud, synthetic, tracking, tsdf
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
# the camera of tools/tsdf_bench.py, and the pose the tracked frame starts from: a degree and a centimetre away
T = torch.tensor([[0.99997, -0.003, -0.006, 0.012, 0.003, 0.99999, -0.004, -0.006, 0.006, 0.004, 0.99997, 0.009]] * B, dtype=torch.float32,
                 device=DEV).reshape(B, 3, 4)
T0 = torch.tensor([[0.99985, -0.004, 0.017, 0.010, 0.004, 0.99999, 0.002, -0.005, -0.017, -0.002, 0.99985, 0.008]] * B, dtype=torch.float32,
                  device=DEV).reshape(B, 3, 4)
origin = (-0.5 * D * VOXEL, -0.5 * D * VOXEL, 0.3)
res = dict(batch=B, dims=[D, D, D], voxel=VOXEL, height=H, width=W)
k = [0]


def timed(fn):
    runs = sorted(graph_time_us(fn, calls=12, replays=20) for _ in range(3))
    return runs[1], runs


def copy_us(nbytes):
    n = max(int(nbytes // 8), 1)                         # float32 elements: n read + n written = nbytes
    src = [torch.empty(n, device=DEV) for _ in range(NB)]
    dst = [torch.empty(n, device=DEV) for _ in range(NB)]

    def cp():
        i = k[0] % NB; k[0] += 1
        dst[i].copy_(src[i])
    return timed(cp)


vols = [tsdf.TsdfVolume((D, D, D), VOXEL, origin, K, size=(H, W)) for _ in range(NB)]
preds, uncs = [pred.clone() for _ in range(NB)], [unc.clone() for _ in range(NB)]
for v in vols:
    v.integrate(pred, unc, T)
models = [tuple(t.clone() for t in v.raycast(T, normals=True)) for v in vols]
torch.cuda.synchronize()
res["model_hit"] = float((~torch.isnan(models[0][0])).float().mean())


def run_raycast():
    i = k[0] % NB; k[0] += 1
    vols[i].raycast(T, normals=True)


t, ts = timed(run_raycast)
res["raycast_normals"] = dict(us=t, runs_us=ts)

for stride in (1, 2, 4):
    outs = [tracking.icp(preds[i], K, models[i][0], models[i][2], T0, uncs[i], models[i][1], None, (H, W), iters=1, stride=stride)
            for i in range(NB)]
    torch.cuda.synchronize()
    st = outs[0].stats[0].cpu().numpy()

    def run_step():
        i = k[0] % NB; k[0] += 1
        tracking.icp(preds[i], K, models[i][0], models[i][2], T0, uncs[i], models[i][1], None, (H, W), iters=1, stride=stride, out=outs[i])

    ns = -(-H // stride) * -(-W // stride)
    nbytes = B * (8.0 * min(h * w, 4 * ns) + 20.0 * ns)
    (t, ts), (tc, tcs) = timed(run_step), copy_us(nbytes)
    res[f"step_stride{stride}"] = dict(us=t, runs_us=ts, pixels=B * ns, pairs=float(st[:, 0].sum()), accepted=float(st[:, 5].min()),
                                       pixels_per_us=B * ns / t, mbytes=nbytes / 1e6, gb_per_s=nbytes / t / 1e3, copy_us=tc,
                                       copy_runs_us=tcs, kernel_over_copy=t / tc)

trackers = [tracking.Tracker(v, T) for v in vols]
for tr in trackers:
    tr.update(pred, unc)                                 # the first frame, integrated at T (the volumes hold it already: no harm)
    tr.update(pred, unc)                                 # the first tracked frame: every buffer exists afterwards
torch.cuda.synchronize()
res["update_accepted"] = float(trackers[0].stats[-1, :, 5].min())


def run_update():
    i = k[0] % NB; k[0] += 1
    trackers[i].update(preds[i], uncs[i])


t, ts = timed(run_update)
res["tracker_update"] = dict(us=t, runs_us=ts, iters=trackers[0].options["iters"])
torch.cuda.synchronize()
print(json.dumps(res))
