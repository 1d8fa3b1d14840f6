"""The shape query of the fused 3x3 -> 1x1 launch against a recorded table (no kernel is launched: this runs without a GPU).
cfp_conv3x3_pw_fused_variant promises callers that a launch will fit: it answers from the pixel-pitch rule and the LDS sizes of
csrc/halo_core.h, the same functions the launcher uses.  tests/golden/conv3x3_pw_fused_variant.json holds the answers of the commit before
those functions were unified, over Cin x Cmid x Cout x stride in bf16 plus one float32 row; the test reads it and recomputes nothing."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_conv3x3_pw_fused_variant_answers_the_recorded_table():
    from cfpnet_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = hip.load()
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "conv3x3_pw_fused_variant.json")))
    assert table["columns"] == ["Cin", "Cmid", "Cout", "stride", "dtype", "variant"]
    dt = {"bf16": hip.BF16, "f32": hip.F32}
    rows = table["rows"]
    assert len(rows) == 7 * 6 * 4 * 2 + 1
    assert {r[5] for r in rows} == {-1, 2, 5, 6}                       # every answer the query has occurs in the grid
    assert [r for r in rows if r[4] == "f32"] == [[40, 160, 40, 1, "f32", -1]]
    bad = [(r, got) for r in rows for got in [int(lib.cfp_conv3x3_pw_fused_variant(r[0], r[1], r[2], r[3], dt[r[4]]))] if got != r[5]]
    assert not bad, f"{len(bad)} of {len(rows)} answers changed, first (row, got): {bad[:5]}"
