#!/usr/bin/env python3
"""Outputs of cfp_loftr_tail and cfp_lkpm_tail as .npy files, for an A/B of two builds of the library (CFP_HIP_LIB): the three storage
modes, D = 32 / 64 / 128, 4 / 8 heads, both q paths, 1 / 2 / 4 waves per workgroup forced (cfp_debug_set 35 / 39) and by the row count,
70 / 1073 / 9600 rows.  Run it once per build into two directories, then `tail_dump.py --compare DIR_A DIR_B` compares them byte for
byte and prints the table."""
import hashlib, os, sys
import numpy as np


def compare(a, b):
    """One line per (tail, dtype, D): files compared, files identical, a hash over the group's files of run A."""
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and names, "the two runs wrote different file sets"
    groups = {}
    for n in names:
        da, db = open(os.path.join(a, n), "rb").read(), open(os.path.join(b, n), "rb").read()
        g = groups.setdefault("_".join(n.split("_")[:3]), [0, 0, hashlib.sha256()])
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
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cfpnet_amd import hip, ops
out_dir = sys.argv[1]
os.makedirs(out_dir, exist_ok=True)
DEV = "cuda:0"
lib = hip.load()
save = lambda name, t: np.save(os.path.join(out_dir, name), (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy())
try:
    for dname, dt in (("f32x3", torch.float32), ("bf16", torch.bfloat16), ("f16", torch.float16)):
        x3 = dname == "f32x3"
        key = 35 if x3 else 39
        for D in (32, 64, 128):
            g = torch.Generator().manual_seed(D)
            mk = lambda n, k: ops.pack_w_x3((torch.randn(n, k, generator=g) / k ** 0.5).to(DEV)) if x3 else (torch.randn(n, k, generator=g) / k ** 0.5).to(dt).to(DEV)
            wq, wm, w0, w2 = mk(D, D), mk(D, D), mk(2 * D, 2 * D), mk(D, 2 * D)
            w1l, w2l = mk(4 * D, D), mk(D, 4 * D)
            b1l, b2l = torch.randn(4 * D, generator=g).to(DEV) * 0.1, torch.randn(D, generator=g).to(DEV) * 0.1
            ln1 = (torch.rand(D, generator=g).to(DEV) + 0.5, torch.randn(D, generator=g).to(DEV))
            ln2 = (torch.rand(D, generator=g).to(DEV) + 0.5, torch.randn(D, generator=g).to(DEV))
            for NB, Hq, Wq, qt in ((2, 5, 7, 3), (1, 37, 29, 6), (8, 30, 40, 4)):
                rows = NB * Hq * Wq
                G = NB * (-(-Hq // qt)) * (-(-Wq // qt))
                x = ops.new_act(rows, D, dt, DEV); x.buf.copy_(torch.randn(rows, D, generator=g).to(dt))
                qa = ops.new_act(rows, D, dt, DEV); qa.buf.copy_(torch.randn(rows, D, generator=g).to(dt))
                for waves in (1, 2, 4, 0):
                    lib.cfp_debug_set(key, waves)
                    for heads in (4, 8):
                        d = D // heads
                        gh = torch.Generator().manual_seed(1000 * D + heads)
                        kv = (torch.randn(G * heads, d, d, generator=gh) * 0.3).to(DEV); ks = (torch.rand(G * heads, d, generator=gh) + 0.5).to(DEV)
                        for own_q in (True, False):
                            out = ops.new_act(rows, D, dt, DEV, zero=True)
                            ops.loftr_tail(None if own_q else qa, kv, ks, x, out, wq if own_q else None, wm, w0, w2, ln1, ln2, NB, Hq, Wq, qt, qt,
                                           float(qt * qt), heads)
                            save(f"loftr_{dname}_D{D}_h{heads}_{'ownq' if own_q else 'q'}_w{waves}_r{rows}.npy", out.buf)
                    out = ops.new_act(rows, D, dt, DEV, zero=True)
                    ops.lkpm_tail(x, qa, out, w1l, b1l, w2l, b2l, ln1[0], ln1[1], rows)
                    save(f"lkpm_{dname}_D{D}_w{waves}_r{rows}.npy", out.buf)
            torch.cuda.synchronize()
        print(f"{dname}: done", flush=True)
finally:
    lib.cfp_debug_set(35, 0); lib.cfp_debug_set(39, 0)
print(f"wrote {len(os.listdir(out_dir))} files to {out_dir}")
