#!/usr/bin/env python3
"""Graph-timed cost of `cfp_tof_zone_loss` (value + gradient, added into an existing gradient) on the benched training shard, 16
predictions of 208x272 against an 8x8 grid of 52 x 68 pixel zones that covers the 416x544 crop (measured by the sensor model on the ground
truth), next to a device copy that moves the same bytes (the prediction read, the gradient read and written: 12 B per prediction pixel) under the same
protocol, and to the value-only call:

    python tools/zone_loss_bench.py [--batch 16]
    python tools/zone_loss_bench.py --step [--dtype bf16]      # also the captured training step with w_zone = 0 and 0.1, alternating

24 sets of (prediction, gradient) rotate so that back-to-back launches do not find their data in the Infinity Cache.  The step uses the
model's own 6x6 grid of 64 px zones (the zone size is the model's geometry) measured by `TofSimulator` on the target.  Prints one JSON
line.  Measured on one MI355X: DESIGN.md section 4.26."""
import argparse, json, os, sys, time, types
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cfpnet_amd import hip, metrics, spec, synthetic, tof, weights
from _gtime import graph_time_us

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--step", action="store_true", help="also time the captured training step with the term off and on")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--dtype", default="bf16", choices=("f32", "bf16", "f16", "f32x3"))
a = ap.parse_args()
B, h, w, H, W, NB = a.batch, 208, 272, 416, 544, 24
DEV = "cuda:0"
pairs = [synthetic.make_eval_pair(H, W, h, w, 700 + i, 0.1, 0.15) for i in range(B)]
pred0 = torch.from_numpy(np.stack([p[1] for p in pairs])).to(DEV)
gt0 = torch.from_numpy(np.stack([p[0] for p in pairs])).to(DEV)
ZN, ZH, ZW = 8, H // 8, W // 8                           # the 8x8 grid over the whole crop: rectangles of 52 x 68 pixels
rect = torch.tensor([[zy * ZH, zx * ZW, (zy + 1) * ZH, (zx + 1) * ZW] for zy in range(ZN) for zx in range(ZN)], dtype=torch.float32)
rect = rect[None].repeat(B, 1, 1).to(DEV).contiguous()
Z, bins = rect.shape[1], int(4.0 / tof.BIN_WIDTH)
# what the sensor measures there: the sensor model on the ground truth (the metric with the ground truth as its prediction)
_, zt = metrics.zone_consistency(gt0, torch.zeros(B, Z, 2, dtype=torch.float64, device=DEV), rect, torch.ones(B, Z, dtype=torch.bool, device=DEV),
                                 1e-3, 10.0, size=(H, W), max_distance=4.0)
fh, mask = zt[..., :2].contiguous(), (zt[..., 2] > 0).contiguous()
sets = [(pred0.clone(), torch.zeros(B, h, w, device=DEV)) for _ in range(NB)]
lib = hip.load()
nws = int(lib.cfp_tof_zone_loss_ws_bytes(B, Z, bins))
ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
zone = torch.empty(B, Z, 8, dtype=torch.float64, device=DEV)
out = torch.empty(1 + B, dtype=torch.float32, device=DEV)
k = [0]


def make_run(with_grad):
    def run():
        i = k[0] % NB; k[0] += 1
        p, g = sets[i]
        hip.call("cfp_tof_zone_loss", p.data_ptr(), h, w, H, W, B, 1, 1e-3, 10.0, rect.data_ptr(), mask.data_ptr(), fh.data_ptr(), Z, 4.0, bins,
                 tof.BIN_WIDTH, tof.AMBIENT_FLOOR, tof.BIN_WIDTH, 1.0, 1, ws.data_ptr(), nws, zone.data_ptr(), out.data_ptr(),
                 g.data_ptr() if with_grad else 0, hip.current_stream())
    return run


def copy_us(nbytes):
    n = int(nbytes // 2)                                 # bytes: n read + n written = nbytes
    src = [torch.empty(n, dtype=torch.uint8, device=DEV) for _ in range(NB)]
    dst = [torch.empty(n, dtype=torch.uint8, device=DEV) for _ in range(NB)]

    def cp():
        i = k[0] % NB; k[0] += 1
        dst[i].copy_(src[i])
    return graph_time_us(cp, calls=NB, replays=5)


nbytes = 12.0 * B * h * w
t, tv, tc = graph_time_us(make_run(True), calls=NB, replays=5), graph_time_us(make_run(False), calls=NB, replays=5), copy_us(nbytes)
torch.cuda.synchronize()
res = dict(batch=B, pred=[h, w], grid=[H, W], zones=Z, zone_hw=[ZH, ZW], bins=bins, sets=NB, ws_mbytes=nws / 1e6,
           zone_loss=dict(us=t, value_only_us=tv, mbytes=nbytes / 1e6, copy_us=tc, copy_over_kernel=tc / t), loss=float(out[0]),
           n_compared=int(torch.isfinite(zone[..., 2]).sum()))

if a.step:
    from cfpnet_amd.trainer import Trainer
    layers = spec.COMBINE1_LAYERS
    sd = weights.make_torch_state_dict(spec.model_manifest(layers))
    target0 = torch.from_numpy(np.stack([synthetic.make_depth(H, W, seed=50 + i, holes=0.1) for i in range(B)]))[:, None].to(DEV)
    inp = synthetic.to_device(synthetic.make_inputs(B, H, W, 6, 64, seed=5, drop_hist=0.34), DEV)
    tcfg = types.SimpleNamespace(mode="train", train_zone_num=6, train_zone_random_offset=0, simu_max_distance=10.0, zone_sample_num=16)
    m6 = tof.TofSimulator(tcfg, DEV).simulate(target0)                # 10 m: the untrained network predicts about 5 m
    inp["additional"].update(raw_data=m6["fh"], rect_data=m6["rect_data"], zone_mask=m6["mask"])
    DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f32x3": "f32x3"}[a.dtype]
    trs = {}
    for wz in (0.0, 0.1):
        trs[wz] = Trainer(sd, layers, lr=3e-4, total_steps=100000, dtype=DT, w_zone=wz, zone_max_distance=10.0)
        trs[wz].capture(inp, target0)
        for _ in range(3):
            trs[wz].step(inp, target0)
    ms = {0.0: [], 0.1: []}
    for _ in range(a.rounds):                            # alternate the two, so that drift of the machine hits both
        for wz in (0.0, 0.1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.steps):
                trs[wz].step(inp, target0)
            torch.cuda.synchronize()
            ms[wz].append((time.perf_counter() - t0) / a.steps * 1e3)
    res["step"] = dict(dtype=a.dtype, steps=a.steps, ms_w0=ms[0.0], ms_w01=ms[0.1], median_w0=float(np.median(ms[0.0])),
                       median_w01=float(np.median(ms[0.1])), zone=float(trs[0.1].last_zone))
print(json.dumps(res))
