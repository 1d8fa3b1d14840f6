#!/usr/bin/env python3
"""cfp_conv2d_plan over a grid of problems and debug states, as text rows or as one SHA-256 per (debug state, dtype) block.

Needs no GPU and only the exported ABI (cfp_conv2d_plan, cfp_debug_set), so the same file runs in any checkout of this repository:
copy it into the other checkout's tools/ and diff the two outputs to see what a change to the routing policy (csrc/conv_route.hip) moved.

    python tools/conv_plan_table.py                  every row: state dtype B KH stride rpb Cin Cout M variant splits [launch: ...]
    python tools/conv_plan_table.py --model          the model's own layer shapes (tests/golden/conv_plan_shapes.json) at batch 1 and 8
    python tools/conv_plan_table.py --write FILE     the fixture of tests/test_conv_plan_table.py: block digests + the model rows

The digests are taken after launch_wins(), which maps the rows on which an earlier library's query disagreed with its own launch to what
the launch ran; the text rows show such a row as "launch: variant splits" behind the query's answer.
"""
import argparse, array, ctypes, hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = os.path.join(ROOT, "tests", "golden", "conv_plan_shapes.json")

F32, BF16, F16, F32X3 = 0, 1, 2, 3
DTYPES = (F32, BF16, F16, F32X3)
BATCHES = (1, 8)
FILTERS = ((1, 1), (3, 1), (3, 2))          # (KH, stride)
CINS = (8, 16, 32, 40, 56, 64, 72, 128, 168, 256, 312, 392, 512, 1392)
COUTS = (8, 16, 24, 32, 40, 64, 72, 128, 136, 160, 224, 232, 256, 512, 1024, 1392)
# every threshold the rules use and one below each
MS = (30, 130, 160, 161, 300, 512, 513, 1100, 1101, 1200, 1201, 2400, 2401, 4800, 4801, 7999, 8000, 8999, 9000, 9600, 11999, 12000, 14999,
      15000, 19200, 20000, 20001, 29999, 30000, 38400, 76800, 99999, 100000, 153600, 199999, 200000, 299999, 300000, 614400)
# the debug states planning reads: ((key, value), ...) and the value that resets each key
RESET = {0: -1, 1: -1, 2: 0, 12: 1, 15: 1, 17: 0, 18: 1, 24: 1, 29: 0, 32: 1, 33: 4800, 40: 1}
STATES = ((), ((17, 1),), ((2, 1),), ((12, 0),), ((12, 2),), ((18, 0),), ((24, 0),), ((40, 0),), ((40, 2),), ((15, 0),), ((29, 1),),
          ((32, 0), (17, 1)), ((33, 0),), ((1, 4),)) + tuple(((0, v),) for v in (4, 13, 19, 204, 300, 303, 413, 500, 601))


def state_name(state):
    return "default" if not state else "+".join(f"k{k}={v}" for k, v in state)


def launch_wins(state, dtype, pr, vs, base):
    """What the LAUNCH does for the rows on which the query used to disagree with it (the query was a second, hand-kept copy of the rules), and
    `vs` = (variant, splits) unchanged for every other row.  The digests are taken over launch_wins(row): a library whose query follows its
    launch leaves every row unchanged (tests/test_conv_plan_table.py asserts that), the earlier library's differing rows are mapped to what
    its launch ran.  `base` = the same library's answer for the same problem with no debug key set.  The classes:
      halo_s2          16-bit 3x3 stride-2 layers that halo_wins_s2 / conv3x3_halo_takes send to the whole-depth halo kernel (the stem)
      x3_split_tile    f16x3 under a forced split count / forced K-group tile: a split K never runs on a two-K-group tile (>= 19): tile 4
      forced           cfp_debug_set(0, v): the query applied the force where its copy of the rules happened to, the launch where it says:
                       300+ = the halo kernel for every 3x3 problem it takes (up to 128 input channels, stride 2 included), 400 + v =
                       that f16x3 tile, 500+ = the f16x3 halo kernel for every problem it takes, 600 + v = that chunk tile for every problem
                       it takes; 200 + v only where the direct kernel is a candidate (shared weights).  (Where the launch refuses a forced
                       variant with CFP_EHIP the row is the route as it stands after the refusal.)
    Only halo_s2 exists without a forced variant or split count.  Two answers deliberately stay the earlier query's although the launch
    differs: per-image weights through the first-generation kernels are planned on the whole batch (the launch plans each image), and a
    forced split count is reported for 16-bit per-image weights (the launch runs them un-split) -- callers size memory from `splits`.
    """
    B, KH, stride, rpb, Cin, Cout, M = pr
    st = dict(state)
    force, half, v1 = st.get(0, -1), dtype in (BF16, F16), bool(st.get(2))
    if dtype == F32 or (half and v1):
        return vs
    if dtype == F32X3:
        if KH == 3 and stride == 1 and rpb == 0 and force >= 500:
            return 500, 1
        if 400 <= force < 500:
            return force, vs[1]
        return (404, vs[1]) if vs[1] > 1 and vs[0] >= 419 else vs
    if rpb > 0:
        return base if force == 204 and KH == 3 and stride == 1 else vs
    if KH == 3 and force >= 300:
        if 600 <= force < 700 and stride == 1 and Cin > 64:
            return force, 1
        return (300, 1) if Cin <= 128 and Cout <= 512 else vs
    if KH == 3 and stride == 2 and force < 0:
        halo, halo_s2 = st.get(12, 1), st.get(18, 1)
        if Cin <= 64 and Cout <= 512 and (halo == 2 or (halo == 1 and halo_s2 and M >= 30000 and Cout <= 160)):
            return 300, 1
    return vs


def problems():
    for B in BATCHES:
        for KH, stride in FILTERS:
            for per_image in (0, 1):
                for Cin in CINS:
                    for Cout in COUTS:
                        for M in MS:
                            yield B, KH, stride, (M // B if per_image else 0), Cin, Cout, M


def model_problems():
    """(B, KH, stride, rpb, Cin, Cout, M) of the network's conv / linear launches at batch 1 and 8 (recorded at batch 8 by tools/conv_bench.py)."""
    for M8, Cout, K, KH, stride, piw in json.load(open(SHAPES))["batch8"]:
        for B in (1, 8):
            M = M8 // 8 * B
            yield B, KH, stride, (M // B if piw else 0), K // (KH * KH), Cout, M


class Planner:
    def __init__(self, lib):
        self.lib, self.v, self.s = lib, ctypes.c_int(0), ctypes.c_int(0)
        self.pv, self.ps = ctypes.byref(self.v), ctypes.byref(self.s)

    def __call__(self, dtype, B, KH, stride, rpb, Cin, Cout, M):
        self.lib.cfp_conv2d_plan(M, Cout, KH * KH * Cin, KH, stride, dtype, rpb, B, self.pv, self.ps)
        return self.v.value, self.s.value


def with_state(lib, state, fn):
    try:
        for k, v in state:
            lib.cfp_debug_set(k, v)
        return fn()
    finally:
        for k, _ in state:
            lib.cfp_debug_set(k, RESET[k])


def block(lib, state, dtype, base=None, probs=None):
    """-> [(variant, splits)] of cfp_conv2d_plan over problems() (or probs) in this debug state; base: the same for the empty state."""
    plan = Planner(lib)
    rows = with_state(lib, state, lambda: [plan(dtype, *pr) for pr in (probs if probs is not None else problems())])
    return rows


def canonical(state, dtype, rows, base, probs=None):
    return [launch_wins(state, dtype, pr, vs, b) for pr, vs, b in zip(probs if probs is not None else problems(), rows, base)]


def digest(rows):
    flat = array.array("i", [x for vs in rows for x in vs])
    if sys.byteorder != "little":
        flat.byteswap()
    return hashlib.sha256(flat.tobytes()).hexdigest()


def model_rows(lib, mapped=True):
    """[state, dtype, B, KH, stride, rpb, Cin, Cout, M, variant, splits] of the model's layers, alone and in flight (mapped: after launch_wins)."""
    probs = list(model_problems())
    out = []
    for dtype in (BF16, F16, F32X3, F32):
        base = block(lib, (), dtype, probs=probs)
        for state in ((), ((17, 1),)):
            rows = block(lib, state, dtype, probs=probs)
            if mapped:
                rows = canonical(state, dtype, rows, base, probs)
            out += [[state_name(state), dtype, *pr, *vs] for pr, vs in zip(probs, rows)]
    return out


def digests(lib, states=STATES):
    """{state/dtype: SHA-256 of the block after launch_wins}."""
    out = {}
    for dt in DTYPES:
        base = block(lib, (), dt)
        for st in states:
            out[f"{state_name(st)}/{dt}"] = digest(canonical(st, dt, block(lib, st, dt) if st else base, base))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--write", default=None)
    a = ap.parse_args()
    from cfpnet_amd import hip
    lib = hip.load()
    if a.model:
        for r in model_rows(lib):
            print(*r)
    elif a.write:
        with open(a.write, "w") as f:
            json.dump({"digests": digests(lib), "model_rows": model_rows(lib)}, f, separators=(",", ":"))
            f.write("\n")
    else:
        for dt in DTYPES:
            base = block(lib, (), dt)
            for st in STATES:
                rows = block(lib, st, dt) if st else base
                for pr, vs, c in zip(problems(), rows, canonical(st, dt, rows, base)):
                    print(state_name(st), dt, *pr, *vs, "" if c == vs else f"launch: {c[0]} {c[1]}")


if __name__ == "__main__":
    main()
