"""The zone rectangle of the eval forward read from a device record: the three record-reading kernels against their
scalar-argument twins, the engine with and without `zone_records`, one dynamic capture replayed over moving rectangles, and the module
boundary choosing between static and dynamic graphs.  Everything the record changes must be BIT-identical to the static path."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import rel_l1  # noqa: E402
from cfpnet_amd import geometry as G, hip, ops, spec, synthetic, weights  # noqa: E402
from cfpnet_amd.engine import Engine  # noqa: E402
from oracle import cfpnet_oracle as O  # noqa: E402
from test_dynamic_zones_geometry import FRAMES  # noqa: E402

DEV = "cuda:0"
TOL_F32 = 1e-3      # the gate of the forward tests: relative L1 on the predicted depth map
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
SENTINEL = 7.25     # exact in every storage type


def rec_tensor(sy, sx, tzh, tzw, H, W):
    c = lambda v, hi: max(0, min(v, hi))
    y0, y1, x0, x1 = c(sy, H), c(sy + tzh, H), c(sx, W), c(sx + tzw, W)
    return torch.tensor([sy, sx, tzh, tzw, y0, y1, x0, x1, (y1 - y0) * (x1 - x0)], dtype=torch.int32, device=DEV)


def act(rows, C, dtype, seed=None, ld=24, c0=8):
    """[rows, C] view at column c0 of a wider buffer (a pitch that is not C): random values, or the sentinel everywhere."""
    buf = torch.full((rows, ld), SENTINEL, dtype=dtype, device=DEV)
    if seed is not None:
        g = torch.Generator().manual_seed(seed)
        buf[:, c0:c0 + C] = torch.randn(rows, C, generator=g).to(dtype).to(DEV)
    return ops.Act(buf, c0, C)


# ------------------------------------------------------------------------------------------------ 1. kernels against their scalar twins
@pytest.mark.parametrize("dtype", DTYPES)
def test_resize_from_a_record_equals_the_scalar_launch(dtype):
    B, H, W, C, zn, p1, p2 = 2, 9, 11, 8, 2, 3, 4
    gh, gw = zn * p1, zn * p2
    rects = [(1, 2, 6, 8),        # the zone grid's own extent: no resampling
             (2, 1, 5, 7),        # resampled
             (-1, -2, 6, 8),      # overhangs the top and the left edge
             (5, 6, 6, 8),        # overhangs the bottom and the right edge
             (-2, 7, 5, 7)]       # resampled and overhanging two edges
    valid = torch.ones(B, zn * zn, dtype=torch.uint8, device=DEV)
    valid[1, 2] = 0               # one zone off in image 1
    tokens = act(B * H * W, C, dtype, seed=1)
    grid = act(B * gh * gw, C, dtype, seed=2)
    n = 0
    for (sy, sx, tzh, tzw) in rects:
        rec = rec_tensor(sy, sx, tzh, tzw, H, W)
        for zv in (None, valid):
            for acc in (False, True):
                kw = dict(zone_valid=zv, zn=zn, p1=p1, p2=p2, accumulate=acc)
                # crop: rectangle of the token map -> the whole zone grid
                want, got = act(B * gh * gw, C, dtype), act(B * gh * gw, C, dtype)
                ops.resize_bilinear(tokens, H, W, (sy, sx, tzh, tzw), want, gh, gw, (0, 0, gh, gw), B, **kw)
                ops.resize_bilinear(tokens, H, W, None, got, gh, gw, (0, 0, gh, gw), B, rec=rec, rec_side=0, **kw)
                assert torch.equal(got.buf, want.buf), ("crop", sy, sx, tzh, tzw, zv is not None, acc)
                # paste: the whole zone grid -> rectangle of the token map; the sentinel outside the rectangle (and in the pitch) stays
                want, got = act(B * H * W, C, dtype), act(B * H * W, C, dtype)
                ops.resize_bilinear(grid, gh, gw, (0, 0, gh, gw), want, H, W, (sy, sx, tzh, tzw), B, **kw)
                ops.resize_bilinear(grid, gh, gw, (0, 0, gh, gw), got, H, W, None, B, rec=rec, rec_side=1, **kw)
                assert torch.equal(got.buf, want.buf), ("paste", sy, sx, tzh, tzw, zv is not None, acc)
                if not acc:      # the twin itself wrote the clipped rectangle and nothing else (image 0: every zone valid)
                    inside = (want.buf.float() != SENTINEL).reshape(B, H, W, -1)[..., 8:16].all(-1)
                    y0, y1, x0, x1 = rec[4:8].tolist()
                    assert int(inside[0].sum()) == (y1 - y0) * (x1 - x0) and bool(inside[0, y0:y1, x0:x1].all())
                n += 2
    assert n == 40
    # an empty rectangle has no scalar twin (the scalar launch refuses it): the crop is zero, the paste writes nothing
    for (tzh, tzw) in ((0, 8), (6, 0), (-3, 8)):
        rec = rec_tensor(1, 2, tzh, tzw, H, W)
        for acc in (False, True):
            got = act(B * gh * gw, C, dtype)
            ops.resize_bilinear(tokens, H, W, None, got, gh, gw, (0, 0, gh, gw), B, rec=rec, rec_side=0, accumulate=acc)
            want = act(B * gh * gw, C, dtype)
            if not acc:
                want.buf[:, 8:16] = 0
            assert torch.equal(got.buf, want.buf), ("empty crop", tzh, tzw, acc)
            got = act(B * H * W, C, dtype)
            ops.resize_bilinear(grid, gh, gw, (0, 0, gh, gw), got, H, W, None, B, rec=rec, rec_side=1, zone_valid=valid, zn=zn, p1=p1, p2=p2,
                                accumulate=acc)
            assert torch.equal(got.buf, act(B * H * W, C, dtype).buf), ("empty paste", tzh, tzw, acc)


def _attention_pair(dtype, B, H, W, heads, d, th, tw, count_pad, rect):
    y0, y1, x0, x1 = rect
    n_in = (y1 - y0) * (x1 - x0)
    rec = torch.tensor([y0, x0, y1 - y0, x1 - x0, y0, y1, x0, x1, n_in], dtype=torch.int32, device=DEV)
    D = heads * d
    qkv = act(B * H * W, 3 * D, dtype, seed=3 + d, ld=3 * D + 8, c0=0)
    groups = B * -(-H // th) * -(-W // tw)
    nws = ops.attn_kv_ws_floats(B, H, W, th, tw, heads, d)
    res = []
    for r in (None, rec):
        kv = torch.full((groups * heads * d * d,), SENTINEL, dtype=torch.float32, device=DEV)
        ks = torch.full((groups * heads * d,), SENTINEL, dtype=torch.float32, device=DEV)
        ws = torch.zeros(max(nws, 1), dtype=torch.float32, device=DEV)
        out = act(B * H * W, D, dtype, ld=D + 8, c0=8)
        if r is None:
            ops.attn_kv_reduce(qkv.slice(D, D), qkv.slice(2 * D, D), kv, ks, ws, B, H, W, th, tw, rect, count_pad, float(max(n_in, 1)), heads, d)
            ops.attn_apply(qkv.slice(0, D), kv, ks, out, B, H, W, th, tw, rect, float(max(n_in, 1)), heads, d)
        else:
            ops.attn_kv_reduce(qkv.slice(D, D), qkv.slice(2 * D, D), kv, ks, ws, B, H, W, th, tw, None, count_pad, None, heads, d, rec=r)
            ops.attn_apply(qkv.slice(0, D), kv, ks, out, B, H, W, th, tw, None, None, heads, d, rec=r)
        res.append((kv, ks, out.buf))
    what = (dtype, H, W, d, th, tw, rect)
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), ("kv state", what)
    assert torch.equal(res[0][2], res[1][2]), ("apply", what)
    assert bool(torch.isfinite(res[1][2].float()).all()), what
    return groups, nws


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_pair_from_a_record_equals_the_scalar_launch(dtype):
    B, H, W, heads = 2, 5, 6, 2
    for d in (4, 8, 16, 32):
        for rect in ((1, 4, 2, 5),       # interior
                     (0, H, 0, W),       # the whole map: every query excluded
                     (2, 2, 3, 3)):      # empty: n_inside = 0, v_length = 1
            groups, nws = _attention_pair(dtype, B, H, W, heads, d, H, W, False, rect)      # DAPM: one key group per image
            assert nws == groups * heads * (d * d + d)                                       # a single split at this size
    # more than one split of the key range (the workspace + finishing kernel): 9 x 11 = 99 keys per group
    groups, nws = _attention_pair(dtype, 2, 9, 11, 2, 8, 9, 11, False, (1, 8, 2, 10))
    assert nws > groups * 2 * (8 * 8 + 8)
    # key tiles cut by the clip rectangle, zero-padded window positions counted
    _attention_pair(dtype, 2, 5, 6, 2, 8, 3, 4, True, (1, 4, 2, 5))


# ------------------------------------------------------------------------------------------------ shared inputs of the model-level tests
def frame_input(i, batch=1, seed=21, drop=0.2):
    """A synthetic batch whose every sample carries the zone rectangles of FRAMES[i] (host tensors)."""
    inp = synthetic.make_inputs(batch, seed=seed, drop_hist=drop)
    rects = synthetic.pitched_zone_rects(*FRAMES[i])
    inp["additional"]["rect_data"] = torch.from_numpy(np.stack([rects] * batch))
    inp["additional"]["patch_info"] = synthetic.rects_patch_info([rects] * batch)
    return inp


def records(inp, H=480, W=640):
    return torch.from_numpy(G.zone_records(inp["additional"]["patch_info"], H, W)).to(DEV)


@pytest.fixture(scope="module")
def sd_combine1():
    return weights.make_torch_state_dict(spec.model_manifest(spec.COMBINE1_LAYERS))


@pytest.fixture(scope="module")
def feats():
    return synthetic.make_img_features(1)


def same3(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


# ------------------------------------------------------------------------------------------------ 2. eager engine, decoder only
def test_eager_decoder_with_records_is_bit_identical_and_inside_the_gate(sd_combine1, feats):
    eng = Engine(sd_combine1, layer_names=spec.COMBINE1_LAYERS, dtype=torch.float32)
    for i in range(8):
        inp = frame_input(i)
        want = [t.clone() for t in eng.forward(inp, img_features=feats)]
        got = eng.forward(inp, img_features=feats, zone_records=records(inp))
        torch.cuda.synchronize()
        assert same3(got, want), i
        if i in (3, 4):      # frames 4 and 5: fractional origin; overhang and resampling
            _, p0, _ = O.forward(sd_combine1, inp, layer_names=spec.COMBINE1_LAYERS, img_features=feats)
            r = rel_l1(got[1].cpu().numpy(), p0.numpy())
            print(f"frame {i + 1}: pred relL1 vs oracle = {r:.3e}")
            assert r < TOL_F32, (i, r)


def test_eager_baseline_decoder_with_records_is_bit_identical(feats):
    layers = spec.BASELINE_LAYERS
    eng = Engine(weights.make_torch_state_dict(spec.model_manifest(layers)), layer_names=layers, change_embedding=False, no_skip_inside=True,
                 dtype=torch.float32)
    for i in range(8):
        inp = frame_input(i)
        want = [t.clone() for t in eng.forward(inp, img_features=feats)]
        got = eng.forward(inp, img_features=feats, zone_records=records(inp))
        torch.cuda.synchronize()
        assert same3(got, want), i


# ------------------------------------------------------------------------------------------------ 3. captured, full model
@pytest.mark.parametrize("mode", ["f32x3", "f16"])
def test_one_dynamic_capture_replays_every_frame(sd_combine1, mode):
    kw = {} if mode == "f32x3" else {"dtype": torch.float16}
    eng = Engine(sd_combine1, layer_names=spec.COMBINE1_LAYERS, **kw)
    assert eng.x3 == (mode == "f32x3")
    inps = [synthetic.to_device(frame_input(i, seed=40 + i), DEV) for i in range(8)]
    wants = []
    for x in inps:
        wants.append([t.clone() for t in eng.forward(x)])       # the static path, eager
    eng.capture(inps[0], dynamic_zones=True)
    graphs = eng._graph[0]
    for i in range(1, 8):
        got = eng.replay(inps[i])
        torch.cuda.synchronize()
        assert same3(got, wants[i]), (mode, i)
    got = eng.replay(inps[0])
    torch.cuda.synchronize()
    assert same3(got, wants[0]) and eng._graph[0] is graphs      # back to the captured frame: still the one capture
    # another zone grid is another capture's business; the refused replay leaves this one intact
    with pytest.raises(ValueError, match="zone_num"):
        eng.replay(synthetic.to_device(synthetic.make_inputs(1, 480, 640, 6, 64, seed=3), DEV))
    got = eng.replay(inps[5])
    torch.cuda.synchronize()
    assert same3(got, wants[5])
    with pytest.raises(ValueError, match="inflight"):
        eng.capture(inps[0], inflight=2, dynamic_zones=True)


def test_dynamic_capture_with_adopted_inputs_reads_the_callers_tensors(sd_combine1):
    eng = Engine(sd_combine1, layer_names=spec.COMBINE1_LAYERS)
    a, b = synthetic.to_device(frame_input(0, seed=50), DEV), synthetic.to_device(frame_input(4, seed=51), DEV)
    want_a = [t.clone() for t in eng.forward(a)]
    want_b = [t.clone() for t in eng.forward(b)]
    eng.capture(a, adopt_inputs=True, dynamic_zones=True)
    torch.cuda.synchronize()
    assert same3(eng.replay(), want_a)
    for k in ("hist_data", "mask"):
        a["additional"][k].copy_(b["additional"][k])
    a["rgb"].copy_(b["rgb"])
    got = eng.replay(patch_info=b["additional"]["patch_info"])      # new contents in place, new rectangle through the record
    torch.cuda.synchronize()
    assert same3(got, want_b)


def test_dynamic_capture_at_the_benchmark_batch(sd_combine1):
    """Batch 8 (the size the benchmark and the README's second headline latency run): other kernel plans than a single image's."""
    eng = Engine(sd_combine1, layer_names=spec.COMBINE1_LAYERS)
    a, b = synthetic.to_device(frame_input(0, batch=8, seed=55), DEV), synthetic.to_device(frame_input(4, batch=8, seed=56), DEV)
    want_a = [t.clone() for t in eng.forward(a)]
    want_b = [t.clone() for t in eng.forward(b)]
    eng.capture(a, dynamic_zones=True)
    got = eng.replay(b)
    torch.cuda.synchronize()
    assert same3(got, want_b)
    got = eng.replay(a)
    torch.cuda.synchronize()
    assert same3(got, want_a)


def test_dynamic_capture_of_a_batch_with_two_rect_sets(sd_combine1):
    """Images 0 and 1 carry frames 3 and 6: the record is the batch union (fusion.py:70-84), as the reference reduces it."""
    eng = Engine(sd_combine1, layer_names=spec.COMBINE1_LAYERS)
    first = frame_input(0, batch=2, seed=60)
    mixed = synthetic.make_inputs(2, seed=61, drop_hist=0.2)
    rects = [synthetic.pitched_zone_rects(*FRAMES[2]), synthetic.pitched_zone_rects(*FRAMES[5])]
    mixed["additional"]["rect_data"] = torch.from_numpy(np.stack(rects))
    mixed["additional"]["patch_info"] = synthetic.rects_patch_info(rects)
    r4 = G.zone_records(mixed["additional"]["patch_info"], 480, 640)[2]
    assert r4.tolist()[:4] == [5, 25, 112, 135]                  # rows 5..117 of frame 3 and 7..117 of frame 6; columns 25..133 and 50..160
    dm = synthetic.to_device(mixed, DEV)
    want = [t.clone() for t in eng.forward(dm)]
    eng.capture(synthetic.to_device(first, DEV), dynamic_zones=True)
    got = eng.replay(dm)
    torch.cuda.synchronize()
    assert same3(got, want)
    _, p0, _ = O.forward(sd_combine1, mixed, layer_names=spec.COMBINE1_LAYERS)
    per_image = [rel_l1(got[1][b].cpu().numpy(), p0[b].numpy()) for b in range(2)]
    print(f"batch of two rect sets vs oracle: {per_image}")
    assert max(per_image) < TOL_F32


# ------------------------------------------------------------------------------------------------ 4. boundary
def _boundary_model():
    from cfpnet_amd import config
    from cfpnet_amd.deltar import make_model
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = config.parse_args(["@" + os.path.join(root, "configs", "cfpnet_combine1.txt")])
    return make_model(args).eval().to(DEV)


@pytest.fixture
def captures(monkeypatch):
    """Every Engine.capture call of the test, as its `dynamic_zones` argument."""
    calls = []
    real = Engine.capture

    def counted(self, *a, **kw):
        calls.append(bool(kw.get("dynamic_zones", False)))
        return real(self, *a, **kw)

    monkeypatch.setattr(Engine, "capture", counted)
    return calls


def test_boundary_serves_moving_rectangles_from_a_bounded_number_of_captures(captures):
    """Fails before this feature: eight rectangles evict a four-entry cache keyed on the rectangle and every forward captures."""
    model, ref = _boundary_model(), _boundary_model()
    ref.eval_graphs = False
    xs = [synthetic.to_device(frame_input(i, seed=70 + i), DEV) for i in range(8)]
    wants = [ref(x) for x in xs]
    for rnd in range(2):
        before = len(captures)
        for i, x in enumerate(xs):
            got = model(x)
            torch.cuda.synchronize()
            assert same3(got, wants[i]) and got[3] is None, (rnd, i)
        if rnd == 1:
            assert len(captures) == before, captures           # the second round captures nothing
    assert len(captures) <= 1 + model.eval_out_ring, captures
    assert captures[0] is False and all(captures[1:])            # the first rectangle by the static graph, the rest by dynamic ones
    assert len(model._eval_caps) == 1


def test_boundary_same_tensors_with_alternating_patch_info(captures):
    model, ref = _boundary_model(), _boundary_model()
    ref.eval_graphs = False
    a = synthetic.to_device(frame_input(1, seed=80), DEV)
    b = {"rgb": a["rgb"], "additional": dict(a["additional"], patch_info=frame_input(6)["additional"]["patch_info"])}
    want = [ref(a), ref(b)]
    seen_both = None
    for n in range(8):
        got = model((a, b)[n % 2])
        torch.cuda.synchronize()
        assert same3(got, want[n % 2]), n
        if n == 1:
            seen_both = len(captures)
    assert len(captures) == seen_both, captures                  # nothing captured once both rectangles have been seen
    assert seen_both <= 1 + model.eval_out_ring
    # contents changed in place are seen too (the adopted-input graphs read the caller's tensors)
    c = synthetic.to_device(frame_input(1, seed=81), DEV)
    a["rgb"].copy_(c["rgb"]); a["additional"]["hist_data"].copy_(c["additional"]["hist_data"]); a["additional"]["mask"].copy_(c["additional"]["mask"])
    want = [ref(a), ref(b)]
    for n in range(4):
        assert same3(model((a, b)[n % 2]), want[n % 2]), n
    assert len(captures) == seen_both


def test_boundary_with_one_rectangle_captures_what_it_always_did(captures):
    """private-copy graphs for the two ring slots, then adopted-input graphs for the two ring slots: four static captures, no dynamic one."""
    model, ref = _boundary_model(), _boundary_model()
    ref.eval_graphs = False
    a = synthetic.to_device(frame_input(3, seed=90), DEV)
    b = synthetic.to_device(frame_input(3, seed=91), DEV)
    for x in (a, b, b, b, b, a, b):
        assert same3(model(x), ref(x))
    assert captures == [False] * 4, captures
