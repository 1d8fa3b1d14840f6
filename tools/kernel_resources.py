#!/usr/bin/env python3
"""Per-kernel compiled resources of two builds, read from the code-object metadata of their object files -- no GPU needed.

    kernel_resources.py PARENT_CSRC HEAD_CSRC conv_igemm2 conv_igemm_x3 ...

For every kernel symbol of the named objects: SGPR, VGPR (the unified file: arch + accumulation registers), scratch (private segment)
bytes, static LDS bytes and the register-limited waves per SIMD (512 / VGPRs in steps of 8, at most 8), parent -> head.  Exit status 1 if
the symbol sets differ, or a kernel gains scratch or drops a step of the occupancy ladder."""
import os, re, subprocess, sys, tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--" + os.environ.get("ARCH", "gfx950")
KEYS = (".sgpr_count", ".vgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(obj):
    """{symbol: (sgpr, vgpr, scratch, lds)} of the device code embedded in a host object."""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat"), os.path.join(d, "co")
        subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj, os.path.join(d, "unused")])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}"])
        notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", co], text=True)
    out, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r"\s*(?:- )?(\.[a-z_]+):\s*(\S+)\s*$", line)
        if not m:
            continue
        if line.lstrip().startswith("- ") and cur.get(".name"):      # a new entry of amdhsa.kernels
            out[cur[".name"]] = tuple(int(cur.get(k, 0)) for k in KEYS)
            cur = {}
        cur[m.group(1)] = m.group(2)
    if cur.get(".name"):
        out[cur[".name"]] = tuple(int(cur.get(k, 0)) for k in KEYS)
    return {k: v for k, v in out.items() if k.startswith("_Z")}


def waves(vgpr):
    return max(1, min(8, 512 // (max(vgpr, 1) + 7 & ~7)))


bad = 0
parent, head, names = sys.argv[1], sys.argv[2], sys.argv[3:]
for n in names:
    a, b = kernels(os.path.join(parent, n + ".o")), kernels(os.path.join(head, n + ".o"))
    if set(a) != set(b):
        bad = 1
        print(f"{n}: SYMBOL SETS DIFFER: only parent {sorted(set(a) - set(b))}, only head {sorted(set(b) - set(a))}")
    same = moved = 0
    print(f"{n}: {len(a)} kernels      SGPR      VGPR   scratch       LDS  waves")
    for k in sorted(set(a) & set(b)):
        x, y = a[k], b[k]
        worse = y[2] > x[2] or waves(y[1]) < waves(x[1])
        bad |= worse
        same += x == y
        moved += x != y
        short = re.sub(r"^_ZN\d+_GLOBAL__N_1", "", k)
        print(f"{short:72s} " + " ".join(f"{p:4d}->{q:<4d}" for p, q in zip(x, y)) + f" {waves(x[1])}->{waves(y[1])}" +
              ("  WORSE" if worse else "  moved" if x != y else ""))
    print(f"{n}: identical figures {same}, moved {moved}")
sys.exit(bad)
