#!/usr/bin/env python3
"""us per launch at batch 8: cfp_pw_rows against the cfp_conv2d_nhwc launch it replaces on the expand convolutions of the inverted-residual
blocks (and, with --qkv, the six DAPM qkv GEMMs), alone and with --inflight N copies side by side (the plan's in-flight kernel then), inside
replayed HIP graphs (tools/_gtime.py).  Each figure is the median of --runs timings.  --groups 1,2,8 adds forced column-group counts."""
import argparse, json, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cfpnet_amd import hip, ops
from cfpnet_amd.engine import concurrent_streams
from _gtime import graph_time_us, graph_time_us_concurrent

ap = argparse.ArgumentParser()
ap.add_argument("--inflight", type=int, default=1)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--dtype", choices=("bf16", "f16"), default="bf16")
ap.add_argument("--qkv", action="store_true")
ap.add_argument("--groups", default="", help="comma-separated forced column-group counts to time beside the automatic one")
ap.add_argument("--tm", type=int, default=0, help="force the 16-row fragments per wave (cfp_debug_set key 41: 1 / 2; 0 = the kernel's rule)")
ap.add_argument("--out", default=None, help="also write the rows as JSON to this file")
a = ap.parse_args()

# (layers, M, K, N, launches per forward, activation)
SHAPES = [("conv3.0.0", 38400, 56, 224, 1, hip.ACT_SILU), ("conv3.0.1-4", 9600, 112, 448, 4, hip.ACT_SILU), ("conv3.1.0", 9600, 112, 672, 1, hip.ACT_SILU),
          ("conv3.1.1-6, conv4.0", 9600, 136, 816, 7, hip.ACT_SILU), ("conv4.1-11", 2400, 232, 1392, 11, hip.ACT_SILU)]
if a.qkv:
    SHAPES += [("dapm32 qkv", 153600, 32, 96, 2, hip.ACT_NONE), ("dapm64 qkv", 38400, 64, 192, 2, hip.ACT_NONE), ("dapm128 qkv", 9600, 128, 384, 2, hip.ACT_NONE)]
dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
dev = "cuda:0"
hip.load().cfp_debug_set(41, a.tm)
streams = concurrent_streams(dev, want=a.inflight) if a.inflight > 1 else None
ops.PLAN_IN_FLIGHT = a.inflight > 1


def t_us(fn):
    ts = [graph_time_us_concurrent(fn, streams, calls=a.calls, replays=3) if streams else graph_time_us(fn, calls=a.calls, replays=4) for _ in range(a.runs)]
    return statistics.median(ts)


rows = []
forced = [int(g) for g in a.groups.split(",") if g]
print(f"{'layers':22s} {'M':>7} {'K':>4} {'N':>5}  x  {'roof':>6} {'conv2d':>7} {'pw_rows':>8} grp" + "".join(f" {'g=' + str(g):>7}" for g in forced))
tot_c = tot_p = 0.0
for name, M, K, N, cnt, act in SHAPES:
    g = torch.Generator().manual_seed(M + K + N)
    x = ops.Act(torch.randn(M, K, generator=g).to(dtype).to(dev), 0, K)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dtype).to(dev)
    s, t = (torch.rand(N, generator=g) + 0.5).to(dev), torch.randn(N, generator=g).to(dev)
    o1, o2 = ops.new_act(M, N, dtype, dev), ops.new_act(M, N, dtype, dev)
    conv = lambda: ops.conv2d(x, w, s, t, o1, 1, 1, M, 1, 1, 1, 0, 0, 1, M, act)
    rows_fn = lambda gr=0: ops.pw_rows(x, w, s, t, o2, M, act, gr)
    conv(); rows_fn(); torch.cuda.synchronize()
    assert torch.equal(o1.buf.view(torch.int16), o2.buf.view(torch.int16)), name
    roof = 2.0 * (M * K + M * N + N * K) / 4.7e12 * 1e6      # bytes over the copy rate at this size
    tc, tp = t_us(conv), t_us(rows_fn)
    tf = {gr: t_us(lambda: rows_fn(gr)) for gr in forced}
    auto = ops.pw_rows_groups(M, K, N)[0]
    print(f"{name:22s} {M:7d} {K:4d} {N:5d} {cnt:2d} {roof:7.1f} {tc:7.1f} {tp:8.1f} {auto:3d}" + "".join(f" {tf[g]:7.1f}" for g in forced))
    rows.append(dict(layers=name, M=M, K=K, N=N, count=cnt, roof_us=roof, conv2d_us=tc, pw_rows_us=tp, groups=auto, forced=tf))
    tot_c += cnt * tc; tot_p += cnt * tp
print(f"per forward: conv2d {tot_c:.1f} us, pw_rows {tot_p:.1f} us   ({a.dtype}, {a.inflight} in flight, tm {a.tm})")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rows, open(a.out, "w"))
