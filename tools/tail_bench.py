#!/usr/bin/env python3
"""cfp_loftr_tail at the three fusion scales of the benched batch (graph-timed, back-to-back launches).
--dtype picks the storage mode (default bf16), --batch the images per launch, --lkpm adds cfp_lkpm_tail at D = 32 / 64 / 128 with the rows of the same three scales."""
import argparse, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cfpnet_amd import hip, ops
from _gtime import graph_time_us
ap = argparse.ArgumentParser()
ap.add_argument("--dtype", choices=["bf16", "f16", "f32x3"], default="bf16")
ap.add_argument("--lkpm", action="store_true", help="also time the LKPM tail")
ap.add_argument("--batch", type=int, default=8, help="images per launch (1: the row counts of a single image, which run the 1- and 2-wave kernels)")
ap.add_argument("--fine", action="store_true", help="best of 5 graphs of 20 replays each, printed to 0.01 us")
args = ap.parse_args()
DEV = "cuda:0"
x3 = args.dtype == "f32x3"
dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32x3": torch.float32}[args.dtype]
g = torch.Generator().manual_seed(1)
mk = lambda n, k: ops.pack_w_x3((torch.randn(n, k, generator=g) / k ** 0.5).to(DEV)) if x3 else (torch.randn(n, k, generator=g) / k ** 0.5).to(dt).to(DEV)
ln = lambda D: (torch.ones(D, device=DEV), torch.zeros(D, device=DEV), 1e-5)
best = lambda fn: min(graph_time_us(fn, calls=16, replays=20 if args.fine else 5) for _ in range(5 if args.fine else 2))
us = lambda t: f"{t:7.2f}" if args.fine else f"{t:6.1f}"
B = args.batch
for D, heads, NB, Hq, Wq, qt in [(128, 8, B, 30, 40, 4), (128, 4, B, 30, 40, 4), (64, 8, B, 60, 80, 8), (64, 4, B, 60, 80, 8), (32, 8, B, 120, 160, 15), (32, 4, B, 120, 160, 15)]:
    rows = NB * Hq * Wq
    d = D // heads
    G = NB * ((Hq + qt - 1) // qt) * ((Wq + qt - 1) // qt)
    x = ops.new_act(rows, D, dt, DEV); x.buf.copy_(torch.randn(rows, D, generator=g).to(dt))
    out = ops.new_act(rows, D, dt, DEV)
    kv = torch.randn(G * heads, d, d, generator=g).to(DEV); ks = torch.rand(G * heads, d, generator=g).to(DEV) + 0.5
    wq, wm, w0, w2 = mk(D, D), mk(D, D), mk(2 * D, 2 * D), mk(D, 2 * D)
    ln1, ln2 = ln(D), ln(D)
    fn = lambda: ops.loftr_tail(None, kv, ks, x, out, wq, wm, w0, w2, ln1, ln2, NB, Hq, Wq, qt, qt, float(qt * qt), heads)
    fn(); torch.cuda.synchronize()
    print(f"D={D:3d} heads={heads} rows={rows:6d}: {us(best(fn))} us per launch")
for D, rows in [(128, B * 30 * 40), (64, B * 60 * 80), (32, B * 120 * 160)] if args.lkpm else []:
    t = ops.new_act(rows, D, dt, DEV); t.buf.copy_(torch.randn(rows, D, generator=g).to(dt))
    xin = ops.new_act(rows, D, dt, DEV); xin.buf.copy_(torch.randn(rows, D, generator=g).to(dt))
    out = ops.new_act(rows, D, dt, DEV)
    w1, w2 = mk(4 * D, D), mk(D, 4 * D)
    b1, b2 = torch.randn(4 * D, generator=g).to(DEV) * 0.1, torch.randn(D, generator=g).to(DEV) * 0.1
    lg, lb, _ = ln(D)
    fn = lambda: ops.lkpm_tail(t, xin, out, w1, b1, w2, b2, lg, lb, rows)
    fn(); torch.cuda.synchronize()
    print(f"lkpm D={D:3d} rows={rows:6d}: {us(best(fn))} us per launch")
