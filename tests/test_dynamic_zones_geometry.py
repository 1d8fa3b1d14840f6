"""Host side of the moving zone rectangle of the eval forward: the device records, the static key a record-reading
capture is specific to, and the validation a record-reading launch cannot do.  No GPU."""
import numpy as np
import pytest

from cfpnet_amd import geometry as G, synthetic

# (pitch, origin_y, origin_x) of an 8x8 grid: integer and fractional origins, overhang at the top (5), the left (8) and none at the
# bottom / right; resampled at scale 4 (tzh != 8 * 14 = 112: frames 3, 4, 5, 6, 8) and not (1, 2, 7)
FRAMES = [(56, 16, 96), (56, 23, 101), (54, 20, 100), (54.5, 18.25, 97.75), (53.25, -6.5, 90), (55, 30.5, 200.5), (56, 40, 200),
          (53.5, 30, -10.5)]


def frame_patch_info(frame):
    return synthetic.rects_patch_info([synthetic.pitched_zone_rects(*frame)])


def test_eight_frames_share_one_static_key_and_differ_in_their_records():
    infos = [frame_patch_info(f) for f in FRAMES]
    keys = {G.static_zone_key(pi) for pi in infos}
    assert keys == {((14, 14), (7, 7), (4, 4), (8,))}
    assert keys == {G.static_zone_key(synthetic.make_inputs(1)["additional"]["patch_info"])}      # the default grid's
    recs = [G.zone_records(pi, 480, 640) for pi in infos]
    for r in recs:
        assert r.dtype == np.int32 and r.shape == (3, G.ZONE_REC_LEN)
    assert len({r.tobytes() for r in recs}) == 8
    # rows come in FUSION_SCALES order (16, 8, 4) and are zone_record's own
    for pi, r in zip(infos, recs):
        for i, s in enumerate(G.FUSION_SCALES):
            assert np.array_equal(r[i], G.zone_record(pi, s, *G.token_hw(480, 640, s)))
    at4 = [r[2].tolist() for r in recs]
    assert at4[0] == [4, 24, 112, 112, 4, 116, 24, 136, 12544]
    assert at4[4] == [-1, 22, 105, 107, 0, 104, 22, 129, 11128]
    assert at4[6] == [10, 50, 112, 112, 10, 120, 50, 160, 12100]
    assert at4[7] == [7, -2, 107, 106, 7, 114, 0, 104, 11128]
    # both kinds are present at scale 4: rectangles that resample (extent != zone grid) and rectangles that do not
    assert {r[2][2] == 112 and r[2][3] == 112 for r in recs} == {True, False}


def test_static_key_is_what_the_training_captures_already_use():
    from cfpnet_amd.deltar import _patch_signature
    for f in FRAMES:
        pi = frame_patch_info(f)
        assert _patch_signature(pi, rectangle=False) == G.static_zone_key(pi)
    assert len({_patch_signature(frame_patch_info(f)) for f in FRAMES}) == 8          # the full signature tells them apart


def test_moving_zone_frames_keep_the_static_key_for_64_seeds():
    want = G.static_zone_key(synthetic.make_inputs(1)["additional"]["patch_info"])
    overhang = distinct = 0
    for seed in range(64):
        frames = synthetic.moving_zone_frames(4, seed)
        assert len(frames) == 4
        seen = set()
        for fr in frames:
            r = fr["rect_data"].numpy()
            assert r.shape == (1, 64, 4) and r.dtype == np.float32
            pitch = r[0, 0, 2] - r[0, 0, 0]
            assert 53 <= pitch <= 56
            assert abs(r[0, 0, 0] - (480 - 8 * pitch) / 2) <= 24 and abs(r[0, 0, 1] - (640 - 8 * pitch) / 2) <= 24
            assert G.static_zone_key(fr["patch_info"]) == want
            recs = G.zone_records(fr["patch_info"], 480, 640)                       # validates
            seen.add(recs.tobytes())
            overhang += int(r[..., 0].min() < 0 or r[..., 2].max() > 480)
        distinct += len(seen)
    assert overhang > 0 and distinct > 3 * 64 - 8
    a, b = synthetic.moving_zone_frames(3, 7), synthetic.moving_zone_frames(3, 7)
    assert all(np.array_equal(x["rect_data"].numpy(), y["rect_data"].numpy()) for x, y in zip(a, b))      # seeded
    assert synthetic.moving_zone_frames(2, 7, batch=3)[0]["rect_data"].shape == (3, 64, 4)


def test_validation_rejects_rectangles_that_do_not_fit_the_zone_grid():
    pi = frame_patch_info(FRAMES[0])
    recs = G.zone_records(pi, 480, 640)
    G.check_zone_records(recs, pi)
    for row, col, val in ((2, 2, 0), (1, 3, 0), (0, 2, -1)):                   # an empty rectangle at any scale
        bad = recs.copy()
        bad[row, col] = val
        with pytest.raises(ValueError, match="zone grid"):
            G.check_zone_records(bad, pi)
    # wider and taller than the zone grid: 56 px zones 60 px apart -> 476 px = 59 tokens at 1/8 (the first scale, coarse to fine, where it shows) > 8 * 7
    rects = synthetic.pitched_zone_rects(56, 0, 80)
    for zy in range(8):
        for zx in range(8):
            rects[zy * 8 + zx] += np.float32([4 * zy, 4 * zx, 4 * zy, 4 * zx])
    wide = synthetic.rects_patch_info([rects])
    assert G.static_zone_key(wide) == G.static_zone_key(pi)
    with pytest.raises(ValueError, match="does not fit the 56 x 56 zone grid"):
        G.zone_records(wide, 480, 640)
    for only in (0, 1):                                                           # each axis on its own, at every scale it shows at
        r2 = synthetic.pitched_zone_rects(56, 0, 80)
        for zy in range(8):
            for zx in range(8):
                r2[zy * 8 + zx] += np.float32([4 * zy, 0, 4 * zy, 0] if only == 0 else [0, 4 * zx, 0, 4 * zx])
        with pytest.raises(ValueError, match="does not fit"):
            G.zone_records(synthetic.rects_patch_info([r2]), 480, 640)
    # a batch whose two grids sit apart: the union (135 tokens wide at scale 4) is wider than one grid, every sample fits its own -- the
    # reference reduces over the batch (fusion.py:75-84) and resamples the union, and so do the static and the record-reading path
    two = synthetic.rects_patch_info([synthetic.pitched_zone_rects(*FRAMES[2]), synthetic.pitched_zone_rects(*FRAMES[5])])
    assert G.zone_records(two, 480, 640)[2].tolist()[:4] == [5, 25, 112, 135]
