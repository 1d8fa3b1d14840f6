"""us per launch at batch 8, kernels alone: cfp_conv3x3_pw_fused against the 3x3 launch and the 1x1 launch it replaces, on the model's five
3x3 -> 1x1 pairs (in-flight plan hint on, as bench.py runs them).  Run from the repository root."""
import os, sys, math
import torch
sys.path.insert(0, os.getcwd())
from cfpnet_amd import hip, ops
ops.PLAN_IN_FLIGHT = True
DEV = "cuda:0"; dt = torch.bfloat16
def t_us(fn, n=60):
    for _ in range(10): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(3):
        a.record()
        for _ in range(n): fn()
        b.record(); torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / n * 1e3)
    return best
for (B, H, W, Cin, mid, Cout, s, pads, skip, act) in [(8, 240, 320, 16, 64, 40, 2, (0, 0), False, hip.ACT_SILU), (8, 120, 160, 40, 160, 40, 1, (1, 1), True, hip.ACT_SILU),
                                                      (8, 120, 160, 40, 160, 56, 2, (0, 0), False, hip.ACT_SILU), (8, 60, 80, 56, 224, 56, 1, (1, 1), True, hip.ACT_SILU),
                                                      (8, 120, 160, 64, 64, 32, 1, (1, 1), False, hip.ACT_LRELU)]:
    Ho, Wo = -(-H // s), -(-W // s); M = B * Ho * Wo
    x = ops.Act(torch.randn(B * H * W, Cin, device=DEV).to(dt), 0, Cin)
    w1 = (torch.randn(mid, 9 * Cin, device=DEV) / math.sqrt(9 * Cin)).to(dt)
    w2 = (torch.randn(Cout, mid, device=DEV) / math.sqrt(mid)).to(dt)
    s1, t1, s2, t2 = [torch.rand(n, device=DEV) + 0.5 for n in (mid, mid, Cout, Cout)]
    wp = ops.pad_pw_w(w2)
    midb, out = ops.new_act(M, mid, dt, DEV), ops.new_act(M, Cout, dt, DEV)
    res = ops.Act(torch.randn(M, Cout, device=DEV).to(dt), 0, Cout) if skip else None
    f = t_us(lambda: ops.conv3x3_pw_fused(x, w1, s1, t1, act, wp, s2, t2, out, B, H, W, s, pads[0], pads[1], Ho, Wo, hip.ACT_NONE, res))
    e = t_us(lambda: ops.conv2d(x, w1, s1, t1, midb, B, H, W, 3, 3, s, pads[0], pads[1], Ho, Wo, act, None, None))
    p = t_us(lambda: ops.conv2d(midb, w2, s2, t2, out, B, Ho, Wo, 1, 1, 1, 0, 0, Ho, Wo, hip.ACT_NONE, res, None))
    print(f"{Cin:3d} -> {mid:3d} -> {Cout:2d} stride {s} px {M:6d}: fused {f:6.1f} us | expand {e:6.1f} + 1x1 {p:5.1f} = {e + p:6.1f} us")
