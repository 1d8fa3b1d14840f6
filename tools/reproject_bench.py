#!/usr/bin/env python3
"""Graph-timed cost of `cfp_depth_reproject` (splat 1 and 2, with a variance plane) and `cfp_depth_fuse` (B x 480x640 state, 240x320
prediction) next to a device copy that moves the same number of bytes under the same protocol -- the project's yardstick for kernels
bound by HBM:

    python tools/reproject_bench.py [--batch 8]

Bytes counted (read + written, the algorithmic minimum):
  reproject  the state's depth once (4 bytes per source pixel), the z-buffer written, hit and read (8 bytes per target pixel, three
             times: fill, one atomic per hit counted once, resolve), depth, index and plane written (12 bytes per target pixel), the
             plane gathered at the winner (4 bytes per target pixel)
  fuse       the prediction and its std plane (8 bytes per prediction pixel), prior depth and variance read, depth and variance written
             (16 bytes per pixel)
The splat's atomics are scattered 8-byte ones, a lane per address, one per hit with splat 1 and four with splat 2; nothing here tunes
them.  Six sets of buffers rotate, so that back-to-back launches do not find their data in the 256 MiB Infinity Cache.  Every figure is
taken three times (each a graph of 12 calls replayed 20 times); the median is reported and the three are listed.  Prints one JSON line.
Measured on one MI355X (B = 8): DESIGN.md section 4.27."""
import argparse, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cfpnet_amd import hip, pointcloud, synthetic, temporal
from _gtime import graph_time_us

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
a = ap.parse_args()
B, h, w, H, W, NB = a.batch, 240, 320, 480, 640, 6
DEV = "cuda:0"
pred = torch.from_numpy(np.stack([synthetic.make_eval_pair(H, W, h, w, 700 + i, 0.0, 0.02)[1] for i in range(B)])).to(DEV)
unc = torch.rand(B, 3, h, w, device=DEV) * 0.05 + 0.02
K = torch.tensor([pointcloud.ZJUL5_INTRINSICS] * B, dtype=torch.float32, device=DEV)
# a hand-held camera between two frames: a few milliradians and a centimetre
T = torch.tensor([[0.99997, -0.003, -0.006, 0.012, 0.003, 0.99999, -0.004, -0.006, 0.006, 0.004, 0.99997, 0.009]] * B, dtype=torch.float32,
                 device=DEV).reshape(B, 3, 4)
res = dict(batch=B, height=H, width=W)
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


# the state the filter would hold after its first frame, NB copies of it and of every output
first = temporal.TemporalFilter(pointcloud.ZJUL5_INTRINSICS, size=(H, W))
first.update(pred, unc)
state = [(first.depth.clone(), first.var.clone()) for _ in range(NB)]
warped = [(torch.empty(B, H, W, device=DEV), torch.empty(B, H, W, dtype=torch.int32, device=DEV), torch.empty(B, H, W, device=DEV))
          for _ in range(NB)]
lib = hip.load()
ws_warp = torch.empty(lib.cfp_depth_reproject_ws_bytes(B, H, W) // 8, dtype=torch.int64, device=DEV)
ws_fuse = torch.empty(lib.cfp_depth_fuse_ws_bytes(B, H, W) // 8, dtype=torch.int64, device=DEV)
Tf = temporal._pose(T, B, DEV)
inf = float("inf")
for splat in (1, 2):
    def run():
        i = k[0] % NB; k[0] += 1
        temporal._reproject(state[i][0], K, Tf, K, H, W, H, W, -inf, inf, splat, 1e-3, state[i][1], warped[i], ws_warp)
    run()
    torch.cuda.synchronize()
    covered = float((warped[(k[0] - 1) % NB][1] >= 0).float().mean())
    nbytes = B * H * W * (4.0 + 3 * 8.0 + 12.0 + 4.0)
    (t, ts), (tc, tcs) = timed(run), copy_us(nbytes)
    res[f"reproject_splat{splat}"] = dict(us=t, runs_us=ts, covered=covered, atomics_per_source=splat * splat, mbytes=nbytes / 1e6,
                                          tb_per_s=nbytes / t / 1e6, copy_us=tc, copy_runs_us=tcs, kernel_over_copy=t / tc)

outs = [(torch.empty(B, H, W, device=DEV), torch.empty(B, H, W, device=DEV), torch.empty(B, 4, dtype=torch.int32, device=DEV),
         torch.empty(B, 2, dtype=torch.float64, device=DEV)) for _ in range(NB)]


def run_fuse():
    i = k[0] % NB; k[0] += 1
    temporal.fuse(pred, unc, warped[i][0], warped[i][2], out=outs[i], ws=ws_fuse)


run_fuse()
torch.cuda.synchronize()
nbytes = 8.0 * B * h * w + 16.0 * B * H * W
(t, ts), (tc, tcs) = timed(run_fuse), copy_us(nbytes)
res["fuse"] = dict(us=t, runs_us=ts, counts=outs[(k[0] - 1) % NB][2][0].tolist(), mbytes=nbytes / 1e6, tb_per_s=nbytes / t / 1e6, copy_us=tc,
                   copy_runs_us=tcs, kernel_over_copy=t / tc)
torch.cuda.synchronize()
print(json.dumps(res))
