#!/usr/bin/env python3
"""What the device-side ToF degradation costs and what it buys:

    python tools/tof_degrade_bench.py [--steps 60] [--child_timeout 420] [--out profiles/tof_degrade_bench.json]

1. the graph-timed launch time of `cfp_tof_degrade` at B = 16, Z = 36 (the training shard of configs/cfpnet_combine1.txt) and at
   B = 8, Z = 64 (the evaluation grid), next to `cfp_tof_sample_points` on the same zones -- the launch the host path repeats;
2. samples/s of `train.py @configs/cfpnet_combine1.txt --synthetic 256 --max_steps K` with `--tof_rng host`, with `--tof_rng device`
   and with `--tof_rng host` again, so that the run-to-run spread of the unchanged host path stands next to the difference.  The rate
   is taken between the log lines of step 20 and of the last step, timed by this process as the lines arrive: capture and warm-up
   stay out of it.

Every measurement runs in a fresh child process with a time limit; this process never opens the device.  A child that fails or runs
into its limit ends the run: nothing is started after it.  Prints one JSON line.  Measured on one MI355X: DESIGN.md section 4.25."""
import argparse, json, os, re, subprocess, sys, threading, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_times():
    """Child: the two launches inside a replayed graph, 24 rotating sets of zones."""
    import types
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from cfpnet_amd import tof
    from _gtime import graph_time_us
    DEV, NB = "cuda:0", 24
    sim = tof.TofSimulator(types.SimpleNamespace(zone_sample_num=16, sample_uniform=True), DEV)
    res = {}
    for B, Z in ((16, 36), (8, 64)):
        rng = np.random.default_rng(B)
        sets = [{"fh": torch.from_numpy(np.stack([0.4 + 3.2 * rng.random((B, Z)), 0.01 + 0.2 * rng.random((B, Z))], -1)).to(DEV),
                 "mask": torch.from_numpy(rng.random((B, Z)) < 0.85).to(DEV)} for _ in range(NB)]
        out = sim.degrade(sets[0], drop=0.34, seed=1, step=0)
        pts = torch.empty(B, Z, 16, device=DEV)
        k = [0]

        def degrade(noise):
            i = k[0] % NB; k[0] += 1
            sim.degrade(sets[i], drop=0.34, noise=noise, seed=4242, step=i, out=out)

        def sample_points():
            i = k[0] % NB; k[0] += 1
            s = sets[i]
            tof.hip.call("cfp_tof_sample_points", s["fh"].data_ptr(), s["mask"].data_ptr(), sim.w0.data_ptr(), tof.hip.ptr(sim.w1), B * Z, 16,
                         sim.sample_mode, pts.data_ptr(), tof.hip.current_stream())

        res[f"b{B}_z{Z}"] = {"degrade_drop_us": round(graph_time_us(lambda: degrade((0.0, 0.0, 0.0)), calls=NB, replays=20), 3),
                             "degrade_drop_noise_us": round(graph_time_us(lambda: degrade((0.5, 0.0, 0.03)), calls=NB, replays=20), 3),
                             "sample_points_us": round(graph_time_us(sample_points, calls=NB, replays=20), 3)}
    print(json.dumps(res))


def child(cmd, limit, on_line=None):
    """Run `cmd` with a time limit, handing each stdout line to `on_line` as it arrives.  -> (exit status or 'timeout', stdout, stderr tail)."""
    p = subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    timed_out = []
    timer = threading.Timer(limit, lambda: (timed_out.append(1), p.kill()))
    timer.start()
    err = []
    t_err = threading.Thread(target=lambda: err.append(p.stderr.read()), daemon=True)
    t_err.start()
    lines = []
    try:
        for line in p.stdout:
            lines.append(line)
            if on_line:
                on_line(line)
        p.wait()
    finally:
        timer.cancel()
    t_err.join(5)
    return ("timeout" if timed_out else p.returncode), "".join(lines), ("".join(err))[-2000:]


def train_rate(mode, steps, limit, batch=16):
    marks = []

    def on_line(line):
        m = re.search(r"step (\d+)/\d+ loss", line)
        if m:
            marks.append((int(m.group(1)), time.perf_counter()))

    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "@" + os.path.join(ROOT, "configs", "cfpnet_combine1.txt"), "--synthetic", "256",
           "--max_steps", str(steps), "--tof_rng", mode, "--log_every", "10"]
    status, out, err = child(cmd, limit, on_line)
    if status != 0:
        return {"mode": mode, "status": status, "stderr": err}
    cum = re.findall(r"([\d.]+) samples/s", out)
    at = dict(marks)
    first = 20 if 20 in at and steps > 20 else min(at)
    res = {"mode": mode, "status": 0, "steps": steps, "samples_per_s_whole_run": float(cum[-1]) if cum else None}
    if steps > first:
        res["samples_per_s"] = round(batch * (steps - first) / (at[steps] - at[first]), 2)
        res["ms_per_step"] = round(1e3 * (at[steps] - at[first]) / (steps - first), 3)
        res["from_step"] = first
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel_child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--child_timeout", type=float, default=420.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.kernel_child:
        return kernel_times()
    res = {"train": []}
    status, out, err = child([sys.executable, os.path.abspath(__file__), "--kernel_child"], a.child_timeout)
    ok = status == 0
    res["kernel"] = json.loads(out.strip().splitlines()[-1]) if ok else {"status": status, "stderr": err}
    print(f"kernel: {res['kernel']}", file=sys.stderr, flush=True)
    for mode in ("host", "device", "host"):
        if not ok:
            break
        r = train_rate(mode, a.steps, a.child_timeout)
        print(f"train --tof_rng {mode}: {r}", file=sys.stderr, flush=True)
        res["train"].append(r)
        ok = r["status"] == 0
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
