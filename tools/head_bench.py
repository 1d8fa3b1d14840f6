#!/usr/bin/env python3
"""The adaptive-bins head at the bench shape (batch 8, 240x320 half-resolution map): separate kernels (3x3 conv -> ram -> fused
conv_out + softmax) against the one-kernel head (csrc/head_fused.hip) with its exactness islands on / off; back-to-back inside a
replayed HIP graph, alone and with 4 copies side by side (the throughput mode of bench.py).  Every head also with the per-pixel
uncertainty planes (`stats`: std, entropy, pmax -- 3 float32 planes) on, with and without `prob`; a block for the default numerics
(f32x3: conv_out + softmax in bin_head_x3_kernel) and, for context, the torch post-processing of a float32 `prob` that the planes replace.
`--conv0`: instead, decoder.conv0 + head in one kernel (csrc/head_conv0.hip) against the conv0 launch + depth_head_fused, with its phase probes."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cfpnet_amd import hip, ops
from cfpnet_amd.engine import concurrent_streams
from _gtime import graph_time_us, graph_time_us_concurrent
DEV = "cuda:0"
CONV0 = "--conv0" in sys.argv      # only the block that sets cfp_depth_head_conv0_fused against the pair it replaces
if CONV0:
    sys.argv.remove("--conv0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
H, W = 240, 320
M = B * H * W


def conv0_block():
    """decoder.conv0 + head in one kernel (csrc/head_conv0.hip) against the pair: the conv0 launch (halo kernel, 32 -> 128) + depth_head_fused.
    Probes of the one-kernel form: 8 = phase 0 only (t halo + conv0 into LDS), 2 = ... + GEMM1, 4 = ... + GEMM2, 1 = zero-record descriptors."""
    streams = concurrent_streams(DEV, 4)
    fl0 = 2.0 * M * 128 * 9 * 32
    for dt in (torch.bfloat16, torch.float16):
        t = ops.Act(torch.randn(M, 32, device=DEV).to(dt), 0, 32)
        w0 = (torch.randn(128, 9 * 32, device=DEV) * 0.06).to(dt)
        b0 = torch.randn(128, device=DEV) * 0.5
        w3 = (torch.randn(128, 9 * 128, device=DEV) * 0.03).to(dt)
        sh = torch.zeros(128, device=DEV)
        wp0 = ops.permute_wout(torch.randn(256, 128) * 0.3, dt, hilo=False).to(DEV)
        bo = torch.zeros(256, device=DEV)
        cen = torch.sort(torch.rand(B, 256, device=DEV) * 10, dim=1)[0].contiguous()
        unet = ops.new_act(M, 128, dt, DEV)
        prob = torch.empty(B, 256, H * W, dtype=dt, device=DEV)
        pred = torch.empty(M, device=DEV)

        def conv0():
            ops.conv2d(t, w0, None, b0, unet, B, H, W, 3, 3, 1, 1, 1, H, W)

        def head():
            ops.depth_head_fused(unet, w3, None, sh, wp0, bo, cen, prob, pred, B, H, W, ram_hilo=False)

        def pair():
            conv0()
            head()

        def one(probe=0, pr=prob):
            ops.depth_head_conv0_fused(t, w0, None, b0, w3, None, sh, wp0, bo, cen, pr, pred, B, H, W, probe=probe)
        rows = [("conv0 launch (3x3, 32 -> 128)", conv0), ("depth_head_fused", head), ("the pair: conv0 + depth_head_fused", pair),
                ("one kernel: depth_head_conv0_fused", one), ("one kernel, no prob output", lambda: one(pr=None)),
                ("probe: phase 0 only", lambda: one(8)), ("probe: phase 0 + GEMM1", lambda: one(2)), ("probe: phase 0 + GEMM1 + GEMM2", lambda: one(4)),
                ("probe: no fetch (zero-record descriptors)", lambda: one(1))]
        for name, fn in rows:
            a = graph_time_us(fn, calls=6, replays=5)
            a4 = graph_time_us_concurrent(fn, streams, calls=6, replays=5)
            print(f"{str(dt):16s} {name:52s} alone {a:7.1f} us   4 side by side {a4:7.1f} us per call", flush=True)


if CONV0:
    conv0_block()
    sys.exit(0)
FL = 2.0 * M * 128 * (9 * 128 + 256)
for dt in (torch.bfloat16, torch.float16):
    x = ops.Act((torch.randn(M, 128, device=DEV)).to(dt), 0, 128)
    w3 = (torch.randn(128, 9 * 128, device=DEV) * 0.03).to(dt)
    wo = torch.randn(256, 128) * 0.3
    wo16 = wo.to(dt).to(DEV)
    sc, sh = torch.ones(128, device=DEV), torch.zeros(128, device=DEV)
    bo = torch.zeros(256, device=DEV)
    cen = torch.sort(torch.rand(B, 256, device=DEV) * 10, dim=1)[0].contiguous()
    ram = ops.new_act(M, 128, dt, DEV)
    prob = torch.empty(B, 256, H * W, dtype=dt, device=DEV)
    pred = torch.empty(M, device=DEV)

    def unfused():
        ops.conv2d(x, w3, sc, sh, ram, B, H, W, 3, 3, 1, 1, 1, H, W)
        ops.bin_head_fused(ram, wo16, bo, cen, prob, pred, B, H * W)
    rows = [("separate kernels (conv3x3 + bin_head_fused)", unfused)]
    for hl in ((False, False), (True, False), (True, True)):
        wp = ops.permute_wout(wo, dt, hilo=hl[0]).to(DEV)
        rows.append((f"one kernel, Wout hi+lo={hl[0]}, ram hi+lo={hl[1]}",
                     lambda wp=wp, hl=hl: ops.depth_head_fused(x, w3, sc, sh, wp, bo, cen, prob, pred, B, H, W, ram_hilo=hl[1])))
    wp0 = ops.permute_wout(wo, dt, hilo=False).to(DEV)
    for probe, what in ((1, "probe: no fetch (zero-record descriptors)"), (2, "probe: GEMM1 only"), (3, "probe: GEMM1 only, no fetch"), (4, "probe: GEMM1 + GEMM2"),
                        (5, "probe: GEMM1 + GEMM2, no fetch")):
        rows.append((what, lambda probe=probe: ops.depth_head_fused(x, w3, sc, sh, wp0, bo, cen, prob, pred, B, H, W, ram_hilo=False, probe=probe)))
    rows.append(("no prob output", lambda: ops.depth_head_fused(x, w3, sc, sh, wp0, bo, cen, None, pred, B, H, W, ram_hilo=False)))
    unc = torch.empty(B, 3, H * W, device=DEV)
    rows.append(("one kernel, prob + stats", lambda: ops.depth_head_fused(x, w3, sc, sh, wp0, bo, cen, prob, pred, B, H, W, ram_hilo=False, stats=unc)))
    rows.append(("one kernel, stats, no prob output", lambda: ops.depth_head_fused(x, w3, sc, sh, wp0, bo, cen, None, pred, B, H, W, ram_hilo=False, stats=unc)))
    streams = concurrent_streams(DEV, 4)
    for name, fn in rows:
        t = graph_time_us(fn, calls=6, replays=5)
        t4 = graph_time_us_concurrent(fn, streams, calls=6, replays=5)
        print(f"{str(dt):16s} {name:52s} alone {t:7.1f} us ({FL / t / 1e6:5.0f} TFLOP/s)   4 side by side {t4:7.1f} us per call")

# the default numerics: float32 tensors, conv_out (f16x3 matrix math) + softmax + expectation in bin_head_x3_kernel, float32 prob
x32 = ops.Act(torch.randn(M, 128, device=DEV), 0, 128)
wx = ops.pack_w_x3((torch.randn(256, 128, device=DEV) * 0.3).contiguous())
bo = torch.zeros(256, device=DEV)
cen = torch.sort(torch.rand(B, 256, device=DEV) * 10, dim=1)[0].contiguous()
prob32 = torch.empty(B, 256, H * W, device=DEV)
pred = torch.empty(M, device=DEV)
unc = torch.empty(B, 3, H * W, device=DEV)
FL3 = 2.0 * M * 128 * 256
for name, pr, st in (("prob", prob32, None), ("prob + stats", prob32, unc), ("no prob output", None, None), ("stats, no prob output", None, unc)):
    fn = lambda pr=pr, st=st: ops.bin_head_fused(x32, wx, bo, cen, pr, pred, B, H * W, stats=st)
    t = graph_time_us(fn, calls=6, replays=5)
    t4 = graph_time_us_concurrent(fn, streams, calls=6, replays=5)
    print(f"{'f32x3':16s} {'conv_out + softmax, ' + name:52s} alone {t:7.1f} us ({FL3 / t / 1e6:5.0f} TFLOP/s)   4 side by side {t4:7.1f} us per call")


def torch_post():      # what a caller needs today for the same three maps: entropy, centred variance, max over a float32 prob
    c = cen[:, :, None]
    mu = (prob32 * c).sum(1, keepdim=True)
    return torch.stack([(prob32 * (c - mu) ** 2).sum(1).sqrt(), -torch.xlogy(prob32, prob32).sum(1), prob32.max(1)[0]], 1)


ops.bin_head_fused(x32, wx, bo, cen, prob32, pred, B, H * W)
print(f"{'float32':16s} {'torch post-processing of prob (std, entropy, max)':52s} alone {graph_time_us(torch_post, calls=3, replays=3):7.1f} us")
