"""cfp_conv2d_plan without a GPU: the query and the launch share one route function (csrc/conv_route.hip), so the query's table over
tools/conv_plan_table.py's grid of problems and debug states is pinned against the table of the commit before that change
(tests/golden/conv_plan_table.json: one SHA-256 per (debug state, dtype) block and the full rows of the model's own layers).

The earlier query was a second copy of the rules that had drifted from the launch.  tools/conv_plan_table.py's launch_wins() writes down,
class by class, what the LAUNCH did on the rows where the two disagreed; the fixture holds the earlier table after that mapping.  Here every
row must already equal its mapped value (the explicit expectation for the rows of those classes) and every block must hash to the fixture
(every other row is the earlier library's, none left out)."""
import functools
import importlib.util
import json
import os

import pytest

from cfpnet_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("conv_plan_table", os.path.join(ROOT, "tools", "conv_plan_table.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "conv_plan_table.json")))


@functools.lru_cache(maxsize=None)
def _base(dtype):
    return T.block(hip.load(), (), dtype)


def test_the_fixture_covers_the_grid():
    assert set(GOLDEN["digests"]) == {f"{T.state_name(st)}/{dt}" for st in T.STATES for dt in T.DTYPES}
    assert len(GOLDEN["model_rows"]) == 2 * 4 * len(list(T.model_problems()))


@pytest.mark.parametrize("state", T.STATES, ids=T.state_name)
def test_plan_table_block(state):
    lib = hip.load()
    for dtype in T.DTYPES:
        base = _base(dtype)
        rows = T.block(lib, state, dtype) if state else base
        want = T.canonical(state, dtype, rows, base)
        bad = [(pr, vs, w) for pr, vs, w in zip(T.problems(), rows, want) if vs != w]
        assert not bad, f"{T.state_name(state)}/{dtype}: {len(bad)} rows where the query is not what the launch does, e.g. (problem, query, launch) {bad[:3]}"
        assert T.digest(rows) == GOLDEN["digests"][f"{T.state_name(state)}/{dtype}"], f"{T.state_name(state)}/{dtype}"


def test_without_a_forced_variant_only_the_stride2_halo_rows_may_differ_from_the_earlier_table():
    """launch_wins() is the identity outside the 16-bit 3x3 stride-2 shared-weight rows in every state that sets neither key 0 nor key 1
    (x3_split_tile needs a split on a K-group tile, which only those keys produce: no such row exists in these states, see the block test),
    so in those states every other row of the fixture is the earlier library's own answer."""
    probe = (-7, 419)      # a value no class would leave alone if it applied
    for state in T.STATES:
        if any(k in (0, 1) for k, _ in state):
            continue
        for dtype in T.DTYPES:
            for pr in T.problems():
                B, KH, stride, rpb, Cin, Cout, M = pr
                if dtype in (T.BF16, T.F16) and KH == 3 and stride == 2 and rpb == 0:
                    continue
                assert T.launch_wins(state, dtype, pr, (probe[0], 1), probe) == (probe[0], 1), (state, dtype, pr)


def test_the_stride2_halo_rows_are_what_the_launch_runs():
    """The one class of the default state: 16-bit 3x3 stride-2 layers on <= 64 input channels, >= 30 000 pixels, <= 160 output channels
    run conv3x3_halo.hip (halo_wins_s2 + conv3x3_halo_takes) and are reported as 300, un-split; everything the rule leaves out is not."""
    lib = hip.load()
    plan = T.Planner(lib)
    for dtype in (T.BF16, T.F16):
        for B, Cin, Cout, M in ((8, 8, 40, 614400), (8, 16, 64, 153600), (8, 40, 160, 38400), (1, 8, 40, 76800), (1, 64, 8, 30000)):
            assert plan(dtype, B, 3, 2, 0, Cin, Cout, M) == (300, 1), (dtype, B, Cin, Cout, M)
        for B, Cin, Cout, M in ((1, 8, 40, 29999), (8, 72, 64, 153600), (8, 40, 224, 38400), (8, 56, 1024, 614400)):
            assert plan(dtype, B, 3, 2, 0, Cin, Cout, M)[0] != 300, (dtype, B, Cin, Cout, M)
        assert plan(dtype, 8, 3, 2, 38400 // 8, 40, 160, 38400)[0] != 300          # per-image weights
        assert plan(dtype, 8, 1, 2, 0, 40, 160, 38400)[0] != 300                   # 1x1
    assert plan(T.F32X3, 8, 3, 2, 0, 8, 40, 614400)[0] // 100 == 4 and plan(T.F32, 8, 3, 2, 0, 8, 40, 614400)[0] < 100
    try:
        lib.cfp_debug_set(18, 0)
        assert plan(T.BF16, 8, 3, 2, 0, 8, 40, 614400)[0] != 300
    finally:
        lib.cfp_debug_set(18, 1)


def test_model_layers_row_by_row():
    got = T.model_rows(hip.load(), mapped=False)      # the query's own answers
    assert len(got) == len(GOLDEN["model_rows"])
    for g, w in zip(got, GOLDEN["model_rows"]):
        assert g == w, (g, w)
    # the stem and the first convolution of the encoder stages are among them, booked under the kernel that runs them
    assert sum(1 for r in got if r[1] in (T.BF16, T.F16) and r[3:5] == [3, 2] and r[-2:] == [300, 1]) > 0
