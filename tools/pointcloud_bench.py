#!/usr/bin/env python3
"""Graph-timed cost of `cfp_depth_unproject` and `cfp_points_compact` (B x 240x320 -> 480x640) next to a device copy that moves the same
number of bytes under the same protocol -- the project's yardstick for kernels bound by HBM:

    python tools/pointcloud_bench.py [--batch 8]

Bytes counted (read + written, the algorithmic minimum):
  unproject  the prediction once, 12 bytes per pixel and output map
  compact    Z of every candidate twice (count and scatter pass, 4 bytes each; at stride 1 these reads drag the whole 12-byte rows in),
             the uncertainty plane twice, and per kept pixel the rows read (12 or 24 bytes) and written (16 or 28 bytes)
Six sets of buffers rotate, so that back-to-back launches do not find their data in the 256 MiB Infinity Cache.
Prints one JSON line.  Measured on one MI355X (B = 8): DESIGN.md section 4.15."""
import argparse, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cfpnet_amd import hip, pointcloud, synthetic
from _gtime import graph_time_us

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
a = ap.parse_args()
B, h, w, H, W, NB = a.batch, 240, 320, 480, 640, 6
DEV = "cuda:0"
pred = torch.from_numpy(np.stack([synthetic.make_eval_pair(H, W, h, w, 700 + i, 0.1, 0.15)[1] for i in range(B)])).to(DEV)
unc = torch.rand(B, 3, h, w, device=DEV) * 0.4
K = torch.tensor([pointcloud.ZJUL5_INTRINSICS] * B, dtype=torch.float32, device=DEV)
res = dict(batch=B, height=H, width=W)
k = [0]


def copy_us(nbytes):
    n = int(nbytes // 8)                                 # float32 elements: n read + n written = nbytes
    src = [torch.empty(n, device=DEV) for _ in range(NB)]
    dst = [torch.empty(n, device=DEV) for _ in range(NB)]

    def cp():
        i = k[0] % NB; k[0] += 1
        dst[i].copy_(src[i])
    return graph_time_us(cp, calls=12, replays=5)


dense = [(torch.empty(B, H, W, 3, device=DEV), torch.empty(B, H, W, 3, device=DEV)) for _ in range(NB)]
for name, normals in (("unproject", False), ("unproject_normals", True)):
    def run():
        i = k[0] % NB; k[0] += 1
        pointcloud.unproject(pred, K, (H, W), normals=normals, out=dense[i] if normals else dense[i][0])
    nbytes = 4.0 * B * h * w + 12.0 * B * H * W * (2 if normals else 1)
    t, tc = graph_time_us(run, calls=12, replays=5), copy_us(nbytes)
    res[name] = dict(us=t, mbytes=nbytes / 1e6, tb_per_s=nbytes / t / 1e6, copy_us=tc, copy_over_kernel=tc / t)

# the compaction alone, on the dense maps above: the C entry point with preallocated outputs
lib = hip.load()
for name, stride, with_unc in (("compact_s1", 1, False), ("compact_s2_unc", 2, True), ("compact_s1_unc", 1, True)):
    cap = -(-H // stride) * -(-W // stride)
    outs = [(torch.empty(B, cap, 3, device=DEV), torch.empty(B, cap, 3, device=DEV), torch.empty(B, cap, dtype=torch.int32, device=DEV)) for _ in range(NB)]
    counts = torch.empty(B, dtype=torch.int32, device=DEV)
    nws = lib.cfp_points_compact_ws_bytes(B, H, W, stride)
    ws = torch.empty(nws // 8, dtype=torch.int64, device=DEV)
    plane = unc[:, 0]

    def run():
        i = k[0] % NB; k[0] += 1
        hip.call("cfp_points_compact", dense[i][0].data_ptr(), dense[i][1].data_ptr(), H, W, B, stride, 0.5, 3.0,
                 plane.data_ptr() if with_unc else 0, h, w, unc.stride(0), 0.0, 0.2, cap, outs[i][0].data_ptr(), outs[i][1].data_ptr(),
                 outs[i][2].data_ptr(), counts.data_ptr(), ws.data_ptr(), nws, hip.current_stream())
    run()
    kept = float(counts.sum())
    nbytes = 2 * 4.0 * B * cap + (2 * 4.0 * B * h * w if with_unc else 0.0) + kept * (24 + 28)
    t, tc = graph_time_us(run, calls=12, replays=5), copy_us(nbytes)
    res[name] = dict(us=t, kept_fraction=kept / (B * cap), mbytes=nbytes / 1e6, tb_per_s=nbytes / t / 1e6, copy_us=tc, copy_over_kernel=tc / t)
torch.cuda.synchronize()
print(json.dumps(res))
