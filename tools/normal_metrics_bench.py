#!/usr/bin/env python3
"""Graph-timed cost of `cfp_normal_metrics` (B x 240x320 -> 480x640) next to a device copy that moves the same number of bytes under the
same protocol -- the project's yardstick for kernels bound by HBM (tools/pointcloud_bench.py):

    python tools/normal_metrics_bench.py [--batch 8]

Bytes counted (read + written, the algorithmic minimum): the prediction and the ground truth once, 4 bytes per pixel each, plus 4 bytes
per pixel of the angle map when it is asked for; the histogram, the partial sums and `out` are a few KB per image and are not counted.
24 sets of inputs (and maps) rotate, 12.3 MB each at B = 8, so that back-to-back launches do not find their data in the 256 MiB Infinity
Cache.  Prints one JSON line.  Measured on one MI355X (B = 8): DESIGN.md section 4.21."""
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
B, h, w, H, W, NB = a.batch, 240, 320, 480, 640, 24
DEV = "cuda:0"
pairs = [synthetic.make_eval_pair(H, W, h, w, 700 + i, 0.1, 0.15) for i in range(B)]
pred0 = torch.from_numpy(np.stack([p[1] for p in pairs])).to(DEV)
gt0 = torch.from_numpy(np.stack([p[0] for p in pairs])).to(DEV)
sets = [(pred0.clone(), gt0.clone(), torch.empty(B, H, W, device=DEV)) for _ in range(NB)]
K = torch.tensor([pointcloud.ZJUL5_INTRINSICS] * B, dtype=torch.float32, device=DEV)
lib = hip.load()
nws = lib.cfp_normal_metrics_ws_bytes(B, H, W)
ws = torch.empty(nws // 8, dtype=torch.int64, device=DEV)
out = torch.empty(B, 7, dtype=torch.float64, device=DEV)
hist = torch.empty(B, 1800, dtype=torch.int32, device=DEV)
res = dict(batch=B, height=H, width=W, sets=NB)
k = [0]


def copy_us(nbytes):
    n = int(nbytes // 8)                                 # float32 elements: n read + n written = nbytes
    src = [torch.empty(n, device=DEV) for _ in range(NB)]
    dst = [torch.empty(n, device=DEV) for _ in range(NB)]

    def cp():
        i = k[0] % NB; k[0] += 1
        dst[i].copy_(src[i])
    return graph_time_us(cp, calls=NB, replays=5)


for name, with_map in (("metrics", False), ("metrics_angle_map", True)):
    def run():
        i = k[0] % NB; k[0] += 1
        p, g, m = sets[i]
        hip.call("cfp_normal_metrics", p.data_ptr(), h, w, g.data_ptr(), H, W, B, 1, 1e-3, 10.0, K.data_ptr(), ws.data_ptr(), nws,
                 out.data_ptr(), hist.data_ptr(), m.data_ptr() if with_map else 0, hip.current_stream())
    nbytes = 4.0 * B * h * w + 4.0 * B * H * W * (2 if with_map else 1)
    t, tc = graph_time_us(run, calls=NB, replays=5), copy_us(nbytes)
    res[name] = dict(us=t, mbytes=nbytes / 1e6, tb_per_s=nbytes / t / 1e6, copy_us=tc, copy_over_kernel=tc / t)
torch.cuda.synchronize()
res["n_valid"] = out[:, 6].tolist()
print(json.dumps(res))
