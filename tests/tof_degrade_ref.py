"""numpy / Python-integer mirror of `cfp_tof_degrade` (definition in include/cfpnet_hip.h): Philox4x32-10, zone dropout with
replacement, Box-Muller range noise, and the samples through the ToF oracle's sampling functions.  Checker only."""
import math

import numpy as np

from oracle import tof_oracle as TO

M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11; the constants of Random123) in Python integers: (c0..c3), (k0, k1) -> 4 words."""
    c0, c1, c2, c3 = (int(c) & M32 for c in ctr)
    k0, k1 = (int(k) & M32 for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def seed_key(seed):
    return int(seed) & M32, (int(seed) >> 32) & M32


def dropped_zones(mask_b, drop, key, step, b):
    """The draws of image b: -> (list of the k drawn zone indices, duplicates included)."""
    valid = np.flatnonzero(np.asarray(mask_b, dtype=bool))
    n = int(valid.size)
    k = int(float(n) * float(drop))
    return [int(valid[(philox4x32_10((j, b, step, 0), key)[0] * n) >> 32]) for j in range(k)]


def box_muller(words):
    """The two Box-Muller factors of one Philox block, in float64: sqrt(-2 ln((w1 + 1) 2^-32)) and cos(2 pi w2 2^-32)."""
    return math.sqrt(-2.0 * math.log((float(words[1]) + 1.0) * 2.0 ** -32)), math.cos(6.283185307179586 * (float(words[2]) * 2.0 ** -32))


def standard_normal(words):
    rad, c = box_muller(words)
    return rad * c


def degrade(fh, mask, drop=0.0, noise=(0.0, 0.0, 0.0), seed=0, step=0, w0=None, w1=None):
    """fh [B,Z,2] f64, mask [B,Z] bool -> dict(mask, fh, pts, counts [B,3], noised [B,Z] bool).  `w1` None = the icdf branch with
    table `w0`, otherwise the uniform branch with both tables (as `TofSimulator` holds them)."""
    fh = np.array(fh, dtype=np.float64)
    mask = np.array(mask, dtype=bool)
    B, Z = mask.shape
    key = seed_key(seed)
    prob, mean, sigma = (float(v) for v in noise)
    counts = np.zeros((B, 3), dtype=np.int32)
    noised = np.zeros((B, Z), dtype=bool)
    pts = []
    for b in range(B):
        before = mask[b].copy()
        for z in dropped_zones(before, drop, key, step, b):
            mask[b, z] = False
        for z in np.flatnonzero(mask[b]) if prob > 0.0 else ():
            w = philox4x32_10((int(z), b, step, 1), key)
            if float(w[0]) * 2.0 ** -32 < prob:
                rad, c = box_muller(w)
                fh[b, z, 0] += mean + sigma * rad * c
                noised[b, z] = True
        counts[b] = (before.sum(), (before & ~mask[b]).sum(), noised[b].sum())
        pts.append(TO.sample_points_icdf(fh[b], mask[b], w0) if w1 is None else TO.sample_points_uniform(fh[b], mask[b], w0, w1))
    return {"mask": mask, "fh": fh, "pts": np.stack(pts), "counts": counts, "noised": noised}
