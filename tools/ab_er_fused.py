#!/usr/bin/env python3
"""ms per batch (bf16; AB_BATCH, default 8) with four batches in flight and as one graph, for the CFP_ER_FUSED of the environment: one JSON line.
Run it from the root of the tree under test, one fresh process per switch value, values interleaved (profiles/r6a_er_fused_ab.txt)."""
import os, sys, time, json
import torch
sys.path.insert(0, os.getcwd())
from cfpnet_amd import spec, synthetic, weights
from cfpnet_amd.engine import Engine
layers = spec.COMBINE1_LAYERS
sd = weights.make_torch_state_dict(spec.model_manifest(layers))
B = int(os.environ.get("AB_BATCH", "8"))
inp = synthetic.to_device(synthetic.make_inputs(B), "cuda:0")
out = {}
for mode in (4, 1):
    ts = []
    for rnd in range(2):
        eng = Engine(sd, layer_names=layers, dtype=torch.bfloat16)
        eng.capture(inp, inflight=mode) if mode > 1 else eng.capture(inp)
        run = eng.replay_async if mode > 1 else eng.replay
        for _ in range(16):
            run()
        torch.cuda.synchronize()
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(32):
                run()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / 32 * 1e3)
        del eng
    ts.sort()
    out["inflight4" if mode > 1 else "one_graph"] = {"min": round(ts[0], 4), "median": round(ts[len(ts) // 2], 4), "max": round(ts[-1], 4)}
print(json.dumps({"tree": os.path.basename(os.getcwd()), "CFP_ER_FUSED": os.environ.get("CFP_ER_FUSED", "(default)"), "batch": B, **out}))
