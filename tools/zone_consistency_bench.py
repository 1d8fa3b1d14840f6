#!/usr/bin/env python3
"""Graph-timed cost of one `cfp_tof_zone_consistency` call (B x 240x320 -> 480x640, the 8x8 grid of 56 px zones) next to
`cfp_tof_hist_sim` on the same zone grid, from the same run:

    python tools/zone_consistency_bench.py [--batch 8]

Both launches are latency bound (64 workgroups per image over 3136 pixels each; the re-simulation forms every depth from four taps of
the prediction where the simulation reads one float).  24 sets of inputs rotate so that back-to-back launches do not find their data in
the Infinity Cache.  Prints one JSON line.  Measured on one MI355X (B = 8): DESIGN.md section 4.24."""
import argparse, json, os, sys, types
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cfpnet_amd import hip, synthetic, tof
from _gtime import graph_time_us

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
a = ap.parse_args()
B, h, w, H, W, NB = a.batch, 240, 320, 480, 640, 24
DEV = "cuda:0"
pairs = [synthetic.make_eval_pair(H, W, h, w, 700 + i, 0.1, 0.15) for i in range(B)]
pred0 = torch.from_numpy(np.stack([p[1] for p in pairs])).to(DEV)
gt0 = torch.from_numpy(np.stack([p[0] for p in pairs])).to(DEV)
cfg = types.SimpleNamespace(mode="online_eval", simu_max_distance=4.0, zone_sample_num=16, sample_uniform=False)
sim = tof.TofSimulator(cfg, DEV)
sets = [(pred0.clone(), gt0.clone(), torch.empty(B, H, W, device=DEV)) for _ in range(NB)]
meas = sim.simulate(gt0)
fh, rect, mask = meas["fh"], meas["rect_data"], meas["mask"]
Z = rect.shape[1]
zone = torch.empty(B, Z, 6, dtype=torch.float64, device=DEV)
summ = torch.empty(B, 10, dtype=torch.float64, device=DEV)
res = dict(batch=B, height=H, width=W, zones=Z, zone_px=56, sets=NB)
k = [0]


def hist_sim():
    i = k[0] % NB; k[0] += 1
    sim.simulate(sets[i][1], out=meas)


res["tof_hist_sim_us"] = graph_time_us(hist_sim, calls=NB, replays=5)
for name, with_map in (("zone_consistency_us", False), ("zone_consistency_dev_map_us", True)):
    def run():
        i = k[0] % NB; k[0] += 1
        p, _, m = sets[i]
        hip.call("cfp_tof_zone_consistency", p.data_ptr(), h, w, H, W, B, 1, 1e-3, 10.0, rect.data_ptr(), mask.data_ptr(), fh.data_ptr(), Z, 4.0,
                 100, tof.BIN_WIDTH, tof.AMBIENT_FLOOR, zone.data_ptr(), summ.data_ptr(), m.data_ptr() if with_map else 0, hip.current_stream())
    res[name] = graph_time_us(run, calls=NB, replays=5)
torch.cuda.synchronize()
res["n_compared"] = summ[:, 0].tolist()
res["mae_mu"] = summ[:, 1].tolist()
print(json.dumps(res))
