#!/usr/bin/env python3
"""Graph-timed cost of `cfp_tsdf_integrate` and `cfp_tsdf_raycast` (a 256^3 volume of 2 cm voxels per image, a 240x320 prediction seen
at 480x640, raycast into 480x640 with normals) next to a device copy that moves the same number of bytes under the same protocol -- the
project's yardstick for kernels bound by HBM:

    python tools/tsdf_bench.py [--batch 1] [--dim 256]

Bytes counted (read + written, the algorithmic minimum):
  integrate  16 bytes per UPDATED voxel ((F, Wt) read and written once; a skipped voxel is neither), the prediction and its std plane
             once (8 bytes per prediction pixel).  Every voxel is still projected: `voxels_per_us` counts all of them.
  raycast    20 bytes per target pixel written (depth, std, normal), and the observed part of the volume read once (8 bytes per voxel
             with Wt > 0) -- what a march over the whole surface cannot avoid; the 8-corner gathers of neighbouring samples re-read the
             same lines from cache.
Nothing here tunes the kernels beyond their launch shapes (one thread per voxel, x along the lanes; 16 x 16 pixel tiles).  Six volumes
and output sets rotate, so that back-to-back launches do not find their data in the 256 MiB Infinity Cache.  Every figure is taken three
times (each a graph of 12 calls replayed 20 times); the median is reported and the three are listed.  Prints one JSON line.
Measured on one MI355X: DESIGN.md section 4.28."""
import argparse, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cfpnet_amd import pointcloud, synthetic, tsdf
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
# the camera a little off the volume's axis, and a second view a hand's width away for the raycast
T = torch.tensor([[0.99997, -0.003, -0.006, 0.012, 0.003, 0.99999, -0.004, -0.006, 0.006, 0.004, 0.99997, 0.009]] * B, dtype=torch.float32,
                 device=DEV).reshape(B, 3, 4)
Tv = torch.tensor([[0.9988, -0.003, -0.049, 0.10, 0.003, 0.99999, -0.004, -0.03, 0.049, 0.004, 0.9988, 0.02]] * B, dtype=torch.float32,
                  device=DEV).reshape(B, 3, 4)
origin = (-0.5 * D * VOXEL, -0.5 * D * VOXEL, 0.3)
res = dict(batch=B, dims=[D, D, D], voxel=VOXEL, height=H, width=W)
k = [0]


def timed(fn):
    runs = sorted(graph_time_us(fn, calls=12, replays=20) for _ in range(3))
    return runs[1], runs


def copy_us(nbytes):
    n = int(nbytes // 8)                                 # float32 elements: n read + n written = nbytes
    src = [torch.empty(n, device=DEV) for _ in range(NB)]
    dst = [torch.empty(n, device=DEV) for _ in range(NB)]

    def cp():
        i = k[0] % NB; k[0] += 1
        dst[i].copy_(src[i])
    return timed(cp)


vols = [tsdf.TsdfVolume((D, D, D), VOXEL, origin, K, size=(H, W)) for _ in range(NB)]
for v in vols:
    counts = v.integrate(pred, unc, T)
torch.cuda.synchronize()
seen, updated, behind = (int(c) for c in counts.sum(0).tolist())


def run_integrate():
    i = k[0] % NB; k[0] += 1
    vols[i].integrate(pred, unc, T)


nbytes = 16.0 * updated + 8.0 * B * h * w
(t, ts), (tc, tcs) = timed(run_integrate), copy_us(nbytes)
res["integrate"] = dict(us=t, runs_us=ts, counts=dict(seen=seen, updated=updated, behind=behind), voxels=B * D ** 3,
                        voxels_per_us=B * D ** 3 / t, mbytes=nbytes / 1e6, tb_per_s=nbytes / t / 1e6, copy_us=tc, copy_runs_us=tcs,
                        kernel_over_copy=t / tc)

observed = int((vols[0].volume[..., 1] > 0).sum())
for normals in (True, False):
    def run_raycast():
        i = k[0] % NB; k[0] += 1
        vols[i].raycast(Tv, normals=normals)
    out = vols[0].raycast(Tv, normals=normals)
    torch.cuda.synchronize()
    hit = float((~torch.isnan(out[0])).float().mean())
    step = 0.5 * vols[0].trunc
    nbytes = (20.0 if normals else 8.0) * B * H * W + 8.0 * observed
    (t, ts), (tc, tcs) = timed(run_raycast), copy_us(nbytes)
    res["raycast_normals" if normals else "raycast"] = dict(us=t, runs_us=ts, hit=hit, steps=int((vols[0].hi - vols[0].z_near) / step) + 1,
                                                           observed_voxels=observed, mbytes=nbytes / 1e6, tb_per_s=nbytes / t / 1e6,
                                                           copy_us=tc, copy_runs_us=tcs, kernel_over_copy=t / tc)
torch.cuda.synchronize()
print(json.dumps(res))
