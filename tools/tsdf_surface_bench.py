#!/usr/bin/env python3
"""Graph-timed cost of `cfp_tsdf_surface` on the room of tools/tsdf_bench.py (a 256^3 volume of 2 cm voxels per image with one 240x320
prediction seen at 480x640 integrated into it) next to a device copy that moves the same number of bytes under the same protocol -- the
project's yardstick for kernels bound by HBM:

    python tools/tsdf_surface_bench.py [--batch 1] [--dim 256]

Three calls: count only (`surface_count`: the count pass and the scan), points without normals and points with normals
(`surface_points(capacity=..., out=...)`: count, scan, scatter).  Bytes counted (read + written, the algorithmic minimum): the volume
read once (8 bytes per voxel) plus what leaves -- 4 bytes per image for the count, 20 bytes per kept edge (point, std, index), 32 with
the normal.  The +y and +z neighbour rows and the scatter pass's second look at the chunks that hold a crossing are re-reads the figure
does not count.  Six volumes and output sets rotate, so that back-to-back launches do not find their data in the 256 MiB Infinity Cache.
Every figure is taken three times (each a graph of 12 calls replayed 20 times); the median is reported and the three are listed.
Prints one JSON line.  Measured on one MI355X: DESIGN.md section 4.31."""
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
T = torch.tensor([[0.99997, -0.003, -0.006, 0.012, 0.003, 0.99999, -0.004, -0.006, 0.006, 0.004, 0.99997, 0.009]] * B, dtype=torch.float32,
                 device=DEV).reshape(B, 3, 4)
origin = (-0.5 * D * VOXEL, -0.5 * D * VOXEL, 0.3)
res = dict(batch=B, dims=[D, D, D], voxel=VOXEL)
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
    v.integrate(pred, unc, T)
counts = vols[0].surface_count()
torch.cuda.synchronize()
kept = int(counts.sum())
cap = max(int(counts.max()), 1)
chunks = vols[0].surface_points(capacity=cap).index[0, :int(counts[0])] // (3 * 256)
res.update(kept=kept, capacity=cap, voxels=B * D ** 3, chunks_with_a_crossing=int(torch.unique(chunks).numel()), chunks=(D ** 3 + 255) // 256)


def run_count():
    i = k[0] % NB; k[0] += 1
    vols[i].surface_count()


volume_bytes = 8.0 * B * D ** 3
nbytes = volume_bytes + 4.0 * B
(t, ts), (tc, tcs) = timed(run_count), copy_us(nbytes)
res["count"] = dict(us=t, runs_us=ts, mbytes=nbytes / 1e6, tb_per_s=nbytes / t / 1e6, copy_us=tc, copy_runs_us=tcs, kernel_over_copy=t / tc)

for normals in (False, True):
    outs = [v.surface_points(capacity=cap, normals=normals) for v in vols]

    def run_points():
        i = k[0] % NB; k[0] += 1
        vols[i].surface_points(capacity=cap, normals=normals, out=outs[i])
    nbytes = volume_bytes + 4.0 * B + (32.0 if normals else 20.0) * kept
    (t, ts), (tc, tcs) = timed(run_points), copy_us(nbytes)
    res["points_normals" if normals else "points"] = dict(us=t, runs_us=ts, mbytes=nbytes / 1e6, tb_per_s=nbytes / t / 1e6, copy_us=tc,
                                                        copy_runs_us=tcs, kernel_over_copy=t / tc)
torch.cuda.synchronize()
print(json.dumps(res))
