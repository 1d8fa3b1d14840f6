#!/usr/bin/env python3
"""Outputs of the whole-depth-halo 3x3 convolutions as .npy files, for an A/B of two builds of the library (CFP_HIP_LIB), at the small
shapes of the test suite's case lists: every forced 16-bit halo variant (bf16 / f16, stride 1 and 2), the UP form, cfp_conv3x3_pw_fused,
every forced f16x3 whole-depth and chunk-pipelined variant, the two-source f16x3 variants 40-42.  Run it once per build into two
directories, then `halo_dump.py --compare DIR_A DIR_B` compares them byte for byte and prints the table."""
import hashlib, math, os, sys
import numpy as np


def compare(a, b):
    """One line per group (form, dtype): files compared, files identical, a hash over the group's files of run A."""
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and names, "the two runs wrote different file sets"
    groups = {}
    for n in names:
        da, db = open(os.path.join(a, n), "rb").read(), open(os.path.join(b, n), "rb").read()
        g = groups.setdefault("_".join(n.split("_")[:2]), [0, 0, hashlib.sha256()])
        g[0] += 1; g[1] += da == db; g[2].update(da)
        if da != db:
            print(f"DIFFERENT: {n}")
    for k, (n, same, h) in groups.items():
        print(f"{k:20s} {same:3d} of {n:3d} files identical  sha256 {h.hexdigest()[:16]}")
    same = sum(g[1] for g in groups.values())
    print(f"{same} of {len(names)} files identical")
    return 0 if same == len(names) else 1


if len(sys.argv) == 4 and sys.argv[1] == "--compare":
    sys.exit(compare(sys.argv[2], sys.argv[3]))

import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cfpnet_amd import hip, ops
import test_ops_gpu as T                       # the case lists and operand builders of the suite
import test_conv3x3_pw_fused_gpu as TP
out_dir = sys.argv[1]
os.makedirs(out_dir, exist_ok=True)
DEV = "cuda:0"
lib = hip.load()
save = lambda name, t: np.save(os.path.join(out_dir, name), (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy())
S2_CASES = [(1, 34, 46, 8, 40, 3, 2, (0, 0, 1, 1)), (2, 24, 32, 16, 64, 3, 2, (0, 0, 1, 1)), (1, 21, 35, 40, 160, 3, 2, (1, 1, 1, 1)),
            (1, 66, 20, 24, 16, 3, 2, (0, 0, 1, 1)), (1, 10, 130, 64, 32, 3, 2, (1, 0, 0, 1))]
UP_CASES = [(1, 13, 17, 26, 34, 64, 24, 16), (2, 15, 20, 45, 50, 64, 8, 64), (1, 9, 11, 20, 33, 64, 64, 40), (1, 30, 40, 60, 80, 64, 16, 24)]
UPX3_CASES = [(2, 15, 20, 30, 40, 64, 16, 32), (1, 8, 10, 16, 20, 128, 40, 64), (2, 5, 7, 10, 14, 256, 56, 128), (1, 7, 9, 13, 21, 32, 8, 16),
              (1, 3, 3, 9, 33, 64, 4, 96), (3, 6, 6, 12, 12, 32, 36, 32)]


def conv(tag, variant, ci, case, args, dtype):
    """One forced launch of cfp_conv2d_nhwc; a variant that cannot run the problem writes no file (the same in both builds)."""
    B, H, W, Cin, Cout, k, s, pads = case
    xa, wa, scale, shift, ra, Ho, Wo = args
    out = ops.new_act(B * Ho * Wo, Cout, dtype, DEV, ld=Cout + 24, zero=True)
    try:
        ops.conv2d(xa, wa, scale, shift, ops.Act(out.buf, 16, Cout), B, H, W, k, k, s, pads[0], pads[1], Ho, Wo, hip.ACT_SILU, ra, None)
    except RuntimeError as e:
        assert "cannot run this problem" in str(e), e
        return
    save(f"{tag}_v{variant}_c{ci}.npy", out.buf)


try:
    for dtype, dname in ((torch.bfloat16, "bf16"), (torch.float16, "f16")):
        for stride, cases in ((1, T.HALO_CASES), (2, S2_CASES)):
            for ci, case in enumerate(cases):
                args = T._conv_ref_and_args(case, dtype)[1:]
                for variant in range(8):
                    if case[4] > 4 * T.HALO_CAP[variant]:
                        continue
                    lib.cfp_debug_set(0, 300 + variant)
                    conv(f"halo{stride}_{dname}", variant, ci, case, args, dtype)
        lib.cfp_debug_set(14, 2)
        for ci, (B, Hs, Ws, H, W, Cup, Cskip, Cout) in enumerate(UP_CASES):
            low, skip = T.q(T.rnd(B, Cup, Hs, Ws, seed=31), dtype), T.q(T.rnd(B, Cskip, H, W, seed=32), dtype)
            Cin = Cup + Cskip
            w = T.rnd(Cout, Cin, 3, 3, seed=33, scale=1.0 / math.sqrt(9 * Cin))
            scale, shift = (T.rnd(Cout, seed=34).abs() + 0.5).to(DEV), T.rnd(Cout, seed=35, scale=0.1).to(DEV)
            wp = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous().to(dtype).to(DEV)
            a_low = T.to_act(T.nhwc(low), dtype)
            cat = ops.new_act(B * H * W, Cin, dtype, DEV)
            cat.buf[:, Cup:] = T.nhwc(skip).to(dtype).to(DEV)
            for variant in (0, 1, 2, 3, 7):
                lib.cfp_debug_set(0, 300 + variant)
                out = ops.new_act(B * H * W, Cout, dtype, DEV, zero=True)
                ops.upsample_cat_conv3x3(a_low, Hs, Ws, cat.slice(Cup, Cskip), wp, scale, shift, out, B, H, W, hip.ACT_LRELU)
                save(f"up_{dname}_v{variant}_c{ci}.npy", out.buf)
        lib.cfp_debug_set(0, -1); lib.cfp_debug_set(14, 1)
        for ci, case in enumerate(TP.RAGGED_CASES):
            B, H, W, Cin, mid, Cout, s, (pt, pl, pb, pr), skip, act1, extra = case
            x, w1 = T.q(T.rnd(B, Cin, H, W, seed=1), dtype), T.q(T.rnd(mid, Cin, 3, 3, seed=2, scale=1.0 / math.sqrt(9 * Cin)), dtype)
            w2 = T.q(T.rnd(Cout, mid, seed=3, scale=1.0 / math.sqrt(mid)), dtype)
            s1, t1, s2, t2 = T.rnd(mid, seed=4).abs() + 0.5, T.rnd(mid, seed=5), T.rnd(Cout, seed=6).abs() + 0.5, T.rnd(Cout, seed=7)
            Ho, Wo = (H + pt + pb - 3) // s + 1, (W + pl + pr - 3) // s + 1
            res = T.q(T.rnd(B, Cout, Ho, Wo, seed=8), dtype)
            for act2 in (hip.ACT_NONE, hip.ACT_LRELU):
                fused, _, _ = TP._run_pair(case, dtype, x, w1, s1, t1, w2, s2, t2, res, act2)
                save(f"pw_{dname}_a{act2}_c{ci}.npy", fused)
        torch.cuda.synchronize()
        print(f"{dname}: done", flush=True)
    for tag, variants, cases in (("x3halo_f32", list(range(10)) + [99], T.X3_HALO_CASES),
                                 ("x3chunk_f32", [20, 21, 22, 23, 24, 25, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 43, 44, 45, 46], T.X3_CHUNK_CASES)):
        for ci, case in enumerate(cases):
            _, xa, _, wx, scale, shift, ra, Ho, Wo = T._x3_problem(case)
            for variant in variants:
                lib.cfp_debug_set(0, 500 + variant)
                conv(tag, variant, ci, case, (xa, wx, scale, shift, ra, Ho, Wo), torch.float32)
    for ci, (B, Hs, Ws, H, W, Cup, Csk, Cout) in enumerate(UPX3_CASES):
        low, skip = T.rnd(B, Cup, Hs, Ws, seed=1), T.rnd(B, Csk, H, W, seed=2)
        w = T.rnd(Cout, Cup + Csk, 3, 3, seed=3, scale=1.0 / math.sqrt(9 * (Cup + Csk)))
        scale, shift = T.rnd(Cout, seed=4).abs() + 0.5, T.rnd(Cout, seed=5)
        la = T.to_act(T.nhwc(low), torch.float32, ld=Cup + 8, c0=4)
        cat = ops.new_act(B * H * W, Cup + Csk, torch.float32, DEV, zero=True)
        cat.buf[:, Cup:] = T.nhwc(skip).to(DEV)
        wcat = ops.pack_w_x3_cat(w.permute(0, 2, 3, 1).contiguous().to(DEV), Cup)
        for variant in (40, 41, 42):
            lib.cfp_debug_set(0, 500 + variant)
            out = ops.new_act(B * H * W, Cout, torch.float32, DEV, ld=Cout + 4, zero=True)
            ops.upsample_cat_conv3x3(la, Hs, Ws, cat.slice(Cup, Csk), wcat, scale.to(DEV), shift.to(DEV), out, B, H, W, hip.ACT_LRELU, x3=True)
            save(f"x3up_f32_v{variant}_c{ci}.npy", out.buf)
    torch.cuda.synchronize()
    print("f32x3: done", flush=True)
finally:
    lib.cfp_debug_set(0, -1); lib.cfp_debug_set(14, 1)
print(f"wrote {len(os.listdir(out_dir))} files to {out_dir}")
