#!/usr/bin/env python3
"""Outputs of the LDS-DMA implicit GEMMs (conv_igemm2.hip, conv_igemm_x3.hip) as .npy files, for an A/B of two builds of the library
(CFP_HIP_LIB): every forced 16-bit tile 0-21 (bf16 / f16) and every forced f16x3 tile 0-36 on the suite's CONV_CASES, un-split and with 4
K-splits where the tile allows; then the call forms at the planned tile: per-image weights, two-term weights, the fused LayerNorm with
and without residual, the moments output, cfp_bin_head_fused (f16x3), ticketed split-K.  Run it once per build into two directories, then
`igemm_dump.py --compare DIR_A DIR_B` compares them byte for byte and prints the table."""
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
        print(f"{k:20s} {same:4d} of {n:4d} files identical  sha256 {h.hexdigest()[:16]}")
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
out_dir = sys.argv[1]
os.makedirs(out_dir, exist_ok=True)
DEV = "cuda:0"
lib = hip.load()
HALF = ((torch.bfloat16, "bf16"), (torch.float16, "f16"))
save = lambda name, t: np.save(os.path.join(out_dir, name), (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy())
NO_SPLIT = set(T.GEN2_KGROUPS) | set(ops.X3_ADIRECT) | set(ops.X3_OCC)


def forced(tag, key, variant, dtype, problems):
    """Every CONV_CASE through one forced tile; a tile that refuses a problem writes no file (the same in both builds)."""
    lib.cfp_debug_set(0, key)
    for ci, (case, (xa, wa, scale, shift, ra, Ho, Wo)) in enumerate(zip(T.CONV_CASES, problems)):
        B, H, W, Cin, Cout, k, s, pads = case
        for splits in ((1,) if variant in NO_SPLIT else (1, 4)):
            lib.cfp_debug_set(1, splits)
            out = ops.new_act(B * Ho * Wo, Cout, dtype, DEV, ld=Cout + 24, zero=True)
            ws = torch.empty(splits * B * Ho * Wo * Cout, device=DEV)
            try:
                ops.conv2d(xa, wa, scale, shift, ops.Act(out.buf, 16, Cout), B, H, W, k, k, s, pads[0], pads[1], Ho, Wo, hip.ACT_SILU, ra, ws)
            except RuntimeError as e:
                assert "launch failed" in str(e), e
                print(f"refused: {tag} v{variant} case {ci} splits {splits}", flush=True)
                continue
            save(f"{tag}_v{variant}_c{ci}_s{splits}.npy", out.buf)


def rows_problem(rows, Cin, Cout, dtype, seed):
    x = T.rnd(rows, Cin, seed=seed)
    w = T.rnd(Cout, Cin, seed=seed + 1, scale=1.0 / math.sqrt(Cin))
    sc, sh = (T.rnd(Cout, seed=seed + 2).abs() + 0.5).to(DEV), T.rnd(Cout, seed=seed + 3).to(DEV)
    res = T.to_act(T.rnd(rows, Cout, seed=seed + 4), dtype)
    return T.to_act(x, dtype), w, sc, sh, res


try:
    # ---- every forced tile -------------------------------------------------------------------------------------------------------
    for dtype, dname in HALF:
        problems = [T._conv_ref_and_args(case, dtype)[1:] for case in T.CONV_CASES]
        for v in T.GEN2_VARIANTS:
            forced(f"g2_{dname}", v, v, dtype, problems)
        torch.cuda.synchronize()
        print(f"forced {dname}: done", flush=True)
    problems = []
    for case in T.CONV_CASES:
        _, xa, _, wx, scale, shift, ra, Ho, Wo = T._x3_problem(case)
        problems.append((xa, wx, scale, shift, ra, Ho, Wo))
    for v in range(37):
        forced("x3_f32", 400 + v, v, torch.float32, problems)
    torch.cuda.synchronize()
    print("forced f32x3: done", flush=True)
    lib.cfp_debug_set(0, -1); lib.cfp_debug_set(1, -1)

    # ---- call forms at the planned tile ------------------------------------------------------------------------------------------
    for dtype, dname in HALF + ((torch.float32, "f32x3"),):
        x3 = dtype == torch.float32
        pack = (lambda w: ops.pack_w_x3(w.contiguous().to(DEV))) if x3 else (lambda w: w.to(dtype).to(DEV).contiguous())
        # per-image weights
        for ci, (B, HW, Cin, Cout) in enumerate([(3, 300, 1392, 232), (2, 1200, 816, 136), (2, 70, 64, 24), (3, 70, 72, 40)]):
            xa, _, sc, sh, res = rows_problem(B * HW, Cin, Cout, dtype, 10)
            w = T.rnd(B, Cout, Cin, seed=2, scale=1.0 / math.sqrt(Cin))
            wp = pack(w.reshape(B * Cout, Cin)).reshape(B, Cout, -1)
            out = ops.new_act(B * HW, Cout, dtype, DEV, zero=True)
            ops.conv2d(xa, wp, sc, sh, out, B, 1, HW, 1, 1, 1, 0, 0, 1, HW, hip.ACT_NONE, res, None, per_image_weights=True)
            save(f"piw_{dname}_c{ci}.npy", out.buf)
        # fused LayerNorm (the tile spans the output channels), with and without residual
        for ci, (rows, Cin, Cout) in enumerate([(300, 256, 128), (4800, 128, 64), (1000, 64, 32), (77, 64, 16), (777, 232, 128)]):
            xa, w, sc, sh, res = rows_problem(rows, Cin, Cout, dtype, 20)
            g, bt = (T.rnd(Cout, seed=5).abs() + 0.5).to(DEV), T.rnd(Cout, seed=6).to(DEV)
            for r in (res, None):
                out = ops.new_act(rows, Cout, dtype, DEV, ld=Cout + 8, zero=True)
                ops.linear(xa, pack(w), sc, sh, out, rows, hip.ACT_RELU, r, None, ln=(g, bt, 1e-5))
                save(f"ln_{dname}_c{ci}_res{int(r is not None)}.npy", out.buf)
        if x3:
            continue
        # two-term weights (16-bit pointwise)
        for ci, (rows, Cin, Cout) in enumerate([(700, 136, 816), (9600, 56, 224), (300, 1392, 232), (5000, 64, 64), (210, 72, 40)]):
            xa, w, sc, sh, _ = rows_problem(rows, Cin, Cout, dtype, 30)
            ws_b = ops.conv2d_ws_bytes(rows, Cout, 2 * ((Cin + 63) // 64) * 64, ops.DT[dtype])
            ws = torch.empty(max(ws_b // 4, 1), dtype=torch.float32, device=DEV) if ws_b else None
            out = ops.new_act(rows, Cout, dtype, DEV, zero=True)
            ops.linear(xa, ops.pack_w2(w, dtype).to(DEV).contiguous(), sc, sh, out, rows, ws=ws)
            save(f"w2_{dname}_c{ci}.npy", out.buf)
        # the moments output
        for ci, (B, H, W, Cin, Cout, k, s, pd) in enumerate([(2, 13, 17, 32, 64, 3, 1, 1), (1, 30, 40, 136, 128, 1, 1, 0), (2, 9, 11, 72, 40, 3, 2, 1)]):
            Ho, Wo = (H + 2 * pd - k) // s + 1, (W + 2 * pd - k) // s + 1
            x = (T.rnd(B * H * W, Cin, seed=1) + 3.0).to(dtype).to(DEV)
            w = (T.rnd(Cout, k * k * Cin, seed=2) / math.sqrt(k * k * Cin)).to(dtype).to(DEV)
            y = torch.zeros(B * Ho * Wo, Cout, dtype=dtype, device=DEV)
            mom, ns, rps = ops.conv2d_moments(ops.Act(x, 0, Cin), w, (T.rnd(Cout, seed=3) * 4.0).to(DEV), ops.Act(y, 0, Cout), B, H, W, k, k, s, pd, pd, Ho, Wo)
            save(f"mom_{dname}_c{ci}_y_ns{ns}_rps{rps}.npy", y)
            save(f"mom_{dname}_c{ci}_m_ns{ns}_rps{rps}.npy", mom[: ns * 2 * Cout])
    # cfp_bin_head_fused (f16x3), with and without the probability volume
    for ci, HW in enumerate([8 * 8, 30 * 40 + 4, 120 * 160]):
        B, Cin, nb = 2, 128, 256
        xa = T.to_act(T.rnd(B * HW, Cin, seed=1), torch.float32)
        wx = ops.pack_w_x3(T.rnd(nb, Cin, seed=2, scale=0.25).contiguous().to(DEV))
        centers = torch.sort(torch.rand(B, nb, generator=torch.Generator().manual_seed(2)) * 10, dim=1)[0].to(DEV)
        prob, pred = torch.zeros(B, nb, HW, device=DEV), torch.zeros(B, HW, device=DEV)
        ops.bin_head_fused(xa, wx, T.rnd(nb, seed=3).to(DEV), centers, prob, pred, B, HW)
        save(f"binhead_f32x3_c{ci}_prob.npy", prob)
        save(f"binhead_f32x3_c{ci}_pred.npy", pred)
    # ticketed split-K (what CFP_SPLITK_TICKETS=1 makes the engine ask for: a workspace with the ticket area in front)
    for ci, case in enumerate([(1, 15, 20, 1824, 304, 1, 1, (0, 0, 0, 0)), (2, 8, 8, 136, 816, 1, 1, (0, 0, 0, 0)), (1, 9, 11, 72, 40, 3, 1, (1, 1, 1, 1)),
                               (3, 7, 9, 96, 64, 3, 1, (1, 1, 1, 1))]):
        B, H, W, Cin, Cout, k, s, pads = case
        _, xa, _, wx, scale, shift, ra, Ho, Wo = T._x3_problem(case)
        for variant in (-1, 4, 13, 12, 17, 0):
            lib.cfp_debug_set(0, 400 + variant if variant >= 0 else -1)
            for splits in ((-1,) if variant < 0 else (2, 3, 8)):
                lib.cfp_debug_set(1, splits)
                out = ops.new_act(B * Ho * Wo, Cout, torch.float32, DEV, ld=Cout + 24, zero=True)
                tws = ops.ticket_ws(8 * B * Ho * Wo * Cout * 4, DEV)
                ops.conv2d(xa, wx, scale, shift, ops.Act(out.buf, 16, Cout), B, H, W, k, k, s, pads[0], pads[1], Ho, Wo, hip.ACT_SILU, ra, tws)
                save(f"ticket_f32x3_c{ci}_v{variant}_s{splits}.npy", out.buf)
    torch.cuda.synchronize()
    print("call forms: done", flush=True)
finally:
    lib.cfp_debug_set(0, -1); lib.cfp_debug_set(1, -1)
print(f"wrote {len(os.listdir(out_dir))} files to {out_dir}")
