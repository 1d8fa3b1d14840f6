#!/usr/bin/env python3
"""Graph-timed cost of colour in the TSDF map -- `cfp_tsdf_integrate_rgb` next to `cfp_tsdf_integrate`, `cfp_tsdf_shade` after one
raycast and `cfp_tsdf_surface_rgb` for the room's points -- under the protocol of tools/tsdf_bench.py and tools/tsdf_surface_bench.py: a
256^3 volume of 2 cm voxels per image, a 240x320 prediction seen at 480x640, each figure next to a device copy that moves the same
number of bytes:

    python tools/tsdf_color_bench.py [--batch 1] [--dim 256]

Bytes counted (read + written, the algorithmic minimum):
  integrate       16 bytes per UPDATED voxel, the prediction and its std plane once (8 bytes per prediction pixel) -- tsdf_bench.py's.
  integrate_rgb   that, plus 32 bytes per COLOURED voxel ((R, G, B, Wc) read and written once) and the image once (12 bytes per grid
                  pixel).  Every voxel is still projected.
  shade           16 bytes per target pixel (the depth read, three floats written) and 16 bytes per corner gathered, counted as
                  min(8 * hits, coloured voxels): neighbouring pixels share corners, and no corner need be read twice.
  surface_colors  64 bytes per row: the index, (F, Wt) and (R, G, B, Wc) of both ends, three floats written.
Six volumes and output sets rotate, so that back-to-back launches do not find their data in the 256 MiB Infinity Cache.  The two
integrate figures are taken alternately, three times each, so that a drift of the machine shows in both.  Every figure is the median of
three runs (each a graph of 12 calls replayed 20 times); the three are listed.  Prints one JSON line.  DESIGN.md section 4.32."""
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
rgb = torch.randn(B, 3, H, W, device=DEV)
K = torch.tensor([pointcloud.ZJUL5_INTRINSICS] * B, dtype=torch.float32, device=DEV)
T = torch.tensor([[0.99997, -0.003, -0.006, 0.012, 0.003, 0.99999, -0.004, -0.006, 0.006, 0.004, 0.99997, 0.009]] * B, dtype=torch.float32,
                 device=DEV).reshape(B, 3, 4)
Tv = torch.tensor([[0.9988, -0.003, -0.049, 0.10, 0.003, 0.99999, -0.004, -0.03, 0.049, 0.004, 0.9988, 0.02]] * B, dtype=torch.float32,
                  device=DEV).reshape(B, 3, 4)
origin = (-0.5 * D * VOXEL, -0.5 * D * VOXEL, 0.3)
res = dict(batch=B, dims=[D, D, D], voxel=VOXEL, height=H, width=W)
k = [0]


def once(fn):
    return graph_time_us(fn, calls=12, replays=20)


def median3(runs):
    runs = sorted(runs)
    return runs[1], runs


def copy_us(nbytes):
    n = int(nbytes // 8)                                 # float32 elements: n read + n written = nbytes
    src = [torch.empty(n, device=DEV) for _ in range(NB)]
    dst = [torch.empty(n, device=DEV) for _ in range(NB)]

    def cp():
        i = k[0] % NB; k[0] += 1
        dst[i].copy_(src[i])
    return median3(once(cp) for _ in range(3))


def entry(t, ts, nbytes, **more):
    tc, tcs = copy_us(nbytes)
    return dict(us=t, runs_us=ts, mbytes=nbytes / 1e6, tb_per_s=nbytes / t / 1e6, copy_us=tc, copy_runs_us=tcs, kernel_over_copy=t / tc, **more)


vols = [tsdf.TsdfVolume((D, D, D), VOXEL, origin, K, size=(H, W)) for _ in range(NB)]
for v in vols:
    counts = v.integrate_rgb(pred, rgb, unc, T)
torch.cuda.synchronize()
seen, updated, behind, coloured = (int(c) for c in counts.sum(0).tolist())
res["counts"] = dict(seen=seen, updated=updated, behind=behind, coloured=coloured, voxels=B * D ** 3)


def run_integrate():
    i = k[0] % NB; k[0] += 1
    vols[i].integrate(pred, unc, T)


def run_integrate_rgb():
    i = k[0] % NB; k[0] += 1
    vols[i].integrate_rgb(pred, rgb, unc, T)


plain, colour = [], []
for _ in range(3):                                       # alternately
    plain.append(once(run_integrate))
    colour.append(once(run_integrate_rgb))
(tp, tps), (tc_, tcs_) = median3(plain), median3(colour)
res["integrate"] = entry(tp, tps, 16.0 * updated + 8.0 * B * h * w, voxels_per_us=B * D ** 3 / tp)
res["integrate_rgb"] = entry(tc_, tcs_, 16.0 * updated + 32.0 * coloured + 8.0 * B * h * w + 12.0 * B * H * W, voxels_per_us=B * D ** 3 / tc_,
                             over_integrate=tc_ / tp)

rays = [v.raycast(Tv, normals=False) for v in vols]
outs = [torch.empty(B, H, W, 3, device=DEV) for _ in vols]
torch.cuda.synchronize()
hits = int((~torch.isnan(rays[0][0])).sum())
have = int((vols[0].color[..., 3] > 0).sum())


def run_shade():
    i = k[0] % NB; k[0] += 1
    vols[i].shade(rays[i][0], Tv, out=outs[i])


t, ts = median3(once(run_shade) for _ in range(3))
torch.cuda.synchronize()
res["shade"] = entry(t, ts, 16.0 * B * H * W + 16.0 * min(8 * hits, have), hits=hits, coloured_voxels=have,
                     shaded=int((~torch.isnan(outs[0][..., 0])).sum()))

cnt = vols[0].surface_count()
torch.cuda.synchronize()
kept, cap = int(cnt.sum()), max(int(cnt.max()), 1)
sps = [v.surface_points(capacity=cap, normals=False) for v in vols]
for v, sp in zip(vols, sps):
    v.surface_colors(sp)


def run_surface_colors():
    i = k[0] % NB; k[0] += 1
    vols[i].surface_colors(sps[i])


t, ts = median3(once(run_surface_colors) for _ in range(3))
torch.cuda.synchronize()
res["surface_colors"] = entry(t, ts, 64.0 * kept, rows=kept, with_a_colour=int((~torch.isnan(sps[0].colors[0, :int(cnt[0]), 0])).sum()))
print(json.dumps(res))
