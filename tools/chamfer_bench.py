#!/usr/bin/env python3
"""Graph-timed cost of `cfp_bins_chamfer` (value + gradient) on the benched training shard, 16 crops of 416x544 with 256 bins, next to a
device copy that moves the same bytes (target 4 B + mask 1 B per pixel) under the same protocol:

    python tools/chamfer_bench.py [--batch 16] [--bins 256]
    python tools/chamfer_bench.py --step [--dtype bf16]      # also the captured training step with w_chamfer = 0 and 0.1, alternating

24 sets of (target, mask) rotate, 18 MB each at B = 16, so that back-to-back launches do not find their pixels in the 256 MiB Infinity
Cache.  Prints one JSON line.  Measured on one MI355X: DESIGN.md section 4.23."""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cfpnet_amd import hip, spec, synthetic, train_ops, weights
from _gtime import graph_time_us

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--bins", type=int, default=256)
ap.add_argument("--step", action="store_true", help="also time the captured training step with the term off and on")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--dtype", default="bf16", choices=("f32", "bf16", "f16", "f32x3"))
a = ap.parse_args()
B, H, W, P, NB = a.batch, 416, 544, a.bins, 24
DEV = "cuda:0"
target0 = torch.from_numpy(np.stack([synthetic.make_depth(H, W, seed=50 + i, holes=0.1) for i in range(B)]))[:, None].to(DEV)
sets = [(target0.clone(), (target0 > 1e-3).to(torch.uint8)) for _ in range(NB)]
g = torch.Generator().manual_seed(1)
w = torch.rand(B, P, generator=g) + 0.1
edges, _ = train_ops.bin_centers((w / w.sum(1, keepdim=True)).to(DEV), 1e-3, 10.0)
lib = hip.load()
nws = int(lib.cfp_bins_chamfer_ws_bytes(B, H, W, P))
ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
out = torch.empty(1 + B, dtype=torch.float32, device=DEV)
grad = torch.empty(B, P, dtype=torch.float32, device=DEV)
k = [0]


def run():
    i = k[0] % NB; k[0] += 1
    t, m = sets[i]
    hip.call("cfp_bins_chamfer", edges.data_ptr(), t.data_ptr(), m.data_ptr(), B, H, W, P, 1.0, ws.data_ptr(), nws, out.data_ptr(), grad.data_ptr(),
             hip.current_stream())


def copy_us(nbytes):
    n = int(nbytes // 2)                                 # bytes: n read + n written = nbytes
    src = [torch.empty(n, dtype=torch.uint8, device=DEV) for _ in range(NB)]
    dst = [torch.empty(n, dtype=torch.uint8, device=DEV) for _ in range(NB)]

    def cp():
        i = k[0] % NB; k[0] += 1
        dst[i].copy_(src[i])
    return graph_time_us(cp, calls=NB, replays=5)


nbytes = 5.0 * B * H * W
t, tc = graph_time_us(run, calls=NB, replays=5), copy_us(nbytes)
torch.cuda.synchronize()
res = dict(batch=B, height=H, width=W, bins=P, sets=NB, ws_mbytes=nws / 1e6,
           chamfer=dict(us=t, mbytes=nbytes / 1e6, tb_per_s=nbytes / t / 1e6, copy_us=tc, copy_over_kernel=tc / t), loss=float(out[0]))

if a.step:
    from cfpnet_amd.trainer import Trainer
    layers = spec.COMBINE1_LAYERS
    sd = weights.make_torch_state_dict(spec.model_manifest(layers))
    inp = synthetic.to_device(synthetic.make_inputs(B, H, W, 6, 64, seed=5, drop_hist=0.34), DEV)
    DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f32x3": "f32x3"}[a.dtype]
    trs = {}
    for wc in (0.0, 0.1):
        trs[wc] = Trainer(sd, layers, lr=3e-4, total_steps=100000, dtype=DT, w_chamfer=wc)
        trs[wc].capture(inp, target0)
        for _ in range(3):
            trs[wc].step(inp, target0)
    ms = {0.0: [], 0.1: []}
    for _ in range(a.rounds):                            # alternate the two, so that drift of the machine hits both
        for wc in (0.0, 0.1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.steps):
                trs[wc].step(inp, target0)
            torch.cuda.synchronize()
            ms[wc].append((time.perf_counter() - t0) / a.steps * 1e3)
    res["step"] = dict(dtype=a.dtype, steps=a.steps, ms_w0=ms[0.0], ms_w01=ms[0.1], median_w0=float(np.median(ms[0.0])),
                       median_w01=float(np.median(ms[0.1])), chamfer=float(trs[0.1].last_chamfer))
print(json.dumps(res))
