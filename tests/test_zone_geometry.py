"""Zone-geometry records of the dynamic-geometry training step (geometry.zone_record / capacity): host integers that must
agree exactly with FusionGeometry, the batch reduction of fusion.py:70-84, for every per-sample grid offset."""
import itertools

import numpy as np
import pytest

from cfpnet_amd import geometry as G

CASES = [(256, 320, 3, 64), (416, 544, 6, 64)]


def _reference_record(H, W, zn, zp, offs, scale):
    pi = G.collate_patch_info([G.patch_info_from_rect_data(G.centered_zone_rects(H, W, zn, zp, o), (H, W)) for o in offs])
    g = G.FusionGeometry.from_patch_info(pi, scale)
    h, w = G.token_hw(H, W, scale)
    y0, y1, x0, x1 = g.clipped(h, w)
    return pi, [g.sy_wo, g.sx_wo, g.tzh, g.tzw, y0, y1, x0, x1, (y1 - y0) * (x1 - x0)]


@pytest.mark.parametrize("H,W,zn,zp", CASES)
def test_record_matches_fusion_geometry_over_every_offset_pair(H, W, zn, zp):
    k = 9
    layout = (zn, zp, int((H - zp * zn) / 2), int((W - zp * zn) / 2))
    for o in itertools.product(range(-k, k + 1), repeat=2):
        recs = G.zone_records_from_offsets(o, layout, (H, W))
        assert recs.dtype == np.int32 and recs.shape == (3, G.ZONE_REC_LEN)
        for i, s in enumerate(G.FUSION_SCALES):
            pi, ref = _reference_record(H, W, zn, zp, o, s)
            assert recs[i].tolist() == ref, (o, s)
            assert G.zone_record(pi, s, *G.token_hw(H, W, s)).tolist() == ref


def test_record_reads_the_reference_float_scale_key():
    pi, ref = _reference_record(256, 320, 3, 64, (5, -7), 8)
    assert G.zone_record(pi, 640 / 80, 32, 40).tolist() == ref


@pytest.mark.parametrize("H,W,zn,zp", CASES)
def test_capacity_bounds_every_draw_and_is_reached(H, W, zn, zp):
    k = 8
    layout = (zn, zp, int((H - zp * zn) / 2), int((W - zp * zn) / 2))
    cap = G.capacity(layout, H, W, k)
    seen = {s: [0, 0, 0] for s in G.FUSION_SCALES}
    rng = np.random.default_rng(3)
    draws = [tuple(rng.integers(-k, k + 1, size=4)) for _ in range(200)] + [(-k, k, 0, 0), (k, k, k, k), (-k, -k, -k, -k)]
    for o in draws:
        recs = G.zone_records_from_offsets(o, layout, (H, W))
        for i, s in enumerate(G.FUSION_SCALES):
            tzh, tzw, n = int(recs[i][2]), int(recs[i][3]), int(recs[i][8])
            assert tzh <= cap[s][0] and tzw <= cap[s][1] and n <= cap[s][2], (o, s, cap[s])
            seen[s] = [max(seen[s][0], tzh), max(seen[s][1], tzw), max(seen[s][2], n)]
    for s in G.FUSION_SCALES:
        assert tuple(seen[s]) == cap[s], (s, seen[s], cap[s])      # some draw reaches it (the widest union is among the draws)


def test_zero_bound_capacity_is_the_centred_grid():
    layout = (3, 64, 32, 64)
    cap = G.capacity(layout, 256, 320, 0)
    for i, s in enumerate(G.FUSION_SCALES):
        r = G.zone_records_from_offsets([0, 0], layout, (256, 320))[i]
        assert cap[s] == (int(r[2]), int(r[3]), int(r[8]))
