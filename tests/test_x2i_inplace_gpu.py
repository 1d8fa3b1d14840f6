"""hist2image at 1:1 (cfp_loftr_tail_x2i): the fused tail reads and accumulates the token map in place instead of running between a crop
and a paste launch -- bit-identical to the three launches at op level, and the whole forward bit-identical with CFP_KV_PROJECT and
CFP_X2I_INPLACE off and on."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cfpnet_amd import ops, spec, synthetic, weights  # noqa: E402
from cfpnet_amd.engine import Engine  # noqa: E402
from cfpnet_amd.geometry import FusionGeometry  # noqa: E402

DEV = "cuda:0"
HALF = [torch.bfloat16, torch.float16]


def _rand(shape, dtype, g, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


# D, heads, B, H, W, zones per side, pixels per zone, rectangle origin: the grid overhangs the map at the top and on the right; the row
# counts take the one-, two- and four-wave workgroups of the tail (<= 4 800, < 8 192, >= 8 192 rows)
CASES = [(128, 4, 2, 10, 12, 3, 4, -1, 3), (64, 4, 2, 52, 49, 10, 5, -1, 2), (32, 4, 2, 66, 61, 8, 8, -3, 1), (32, 8, 1, 9, 9, 2, 5, -1, 1)]


@pytest.mark.parametrize("accumulate", [True, False])
@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("case", CASES)
def test_mapped_tail_equals_crop_tail_paste(case, dtype, accumulate):
    D, heads, B, H, W, zn, pz, sy, sx = case
    d = D // heads
    gh = gw = zn * pz
    assert sy < 0 and sx + gw > W
    g = torch.Generator().manual_seed(D + heads)
    tok = torch.full((B * H * W, 2 * D), 5.0, dtype=dtype, device=DEV)      # tokens = columns [0, D) of a [rows, 2D] buffer, as in the engine
    tok[:, :D] = _rand((B * H * W, D), dtype, g)
    valid = (torch.rand(B, zn, zn, generator=g) > 0.3).to(torch.uint8)
    valid[0, 1, 0] = 0
    valid = valid.to(DEV)
    # a token value of -0.0 under a dropped zone: zone (1, 0) of image 0 starts at grid (pz, 0) = token (sy + pz, sx)
    tok.view(B, H, W, 2 * D)[0, sy + pz, sx, 3] = -0.0
    assert bool(torch.signbit(tok.view(B, H, W, 2 * D)[0, sy + pz, sx, 3]))
    # a key/value state per zone from 16 random samples
    G = B * zn * zn
    kvs = ops.Act(_rand((G * 16, 2 * D), dtype, g), 0, 2 * D)
    kv, ks = torch.empty(G * heads * d * d, device=DEV), torch.empty(G * heads * d, device=DEV)
    ops.attn_kv_reduce(kvs.slice(0, D), kvs.slice(D, D), kv, ks, None, G, 1, 16, 1, 16, (0, 1, 0, 16), False, 16.0, heads, d)
    wq, wm = _rand((D, D), dtype, g, D ** -0.5), _rand((D, D), dtype, g, D ** -0.5)
    w0, w2 = _rand((2 * D, 2 * D), dtype, g, (2 * D) ** -0.5), _rand((D, 2 * D), dtype, g, (2 * D) ** -0.5)
    ln1 = (1 + 0.1 * torch.randn(D, generator=g).to(DEV), 0.1 * torch.randn(D, generator=g).to(DEV))
    ln2 = (1 + 0.1 * torch.randn(D, generator=g).to(DEV), 0.1 * torch.randn(D, generator=g).to(DEV))

    # the three launches
    want = tok.clone()
    tw = ops.Act(want, 0, D)
    zin = ops.new_act(B * gh * gw, D, dtype, DEV)
    zout = ops.new_act(B * gh * gw, D, dtype, DEV)
    ops.resize_bilinear(tw, H, W, (sy, sx, gh, gw), zin, gh, gw, (0, 0, gh, gw), B)
    ops.loftr_tail(None, kv, ks, zin, zout, wq, wm, w0, w2, ln1, ln2, B, gh, gw, pz, pz, 16.0, heads)
    ops.resize_bilinear(zout, gh, gw, (0, 0, gh, gw), tw, H, W, (sy, sx, gh, gw), B, zone_valid=valid, zn=zn, p1=pz, p2=pz, accumulate=accumulate)
    # the one launch, in place
    got = tok.clone()
    ops.loftr_tail_x2i(kv, ks, ops.Act(got, 0, D), H, W, sy, sx, wq, wm, w0, w2, ln1, ln2, B, gh, gw, pz, pz, valid, zn, accumulate, 16.0, heads)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want.float()).all())
    assert not torch.equal(want, tok)                        # the layer did something ...
    assert torch.equal(want[:, D:], tok[:, D:])              # ... to the token columns only
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (case, dtype, accumulate)      # bit patterns: the sign of a zero counts
    # under the dropped zone the token is kept (accumulating: token + 0, so the -0.0 became +0.0) or zeroed
    z = got.view(B, H, W, 2 * D)[0, sy + pz, sx, :D]
    assert not bool(torch.signbit(z[3])) and float(z[3]) == 0.0
    if not accumulate:
        assert bool((z == 0).all())


@pytest.fixture(scope="module")
def state_dict():
    return weights.make_torch_state_dict(spec.model_manifest(spec.COMBINE1_LAYERS))


# 256 x 320 with 3 x 3 zones of 64 px: every scale 1:1.  192 x 256 with 8 x 8 zones of 20 px: 1:1 at stride 4, resampling at strides 8 and
# 16, ragged LSA windows at every scale.
@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("shape", [(256, 320, 3, 64, (False, False, False)), (192, 256, 8, 20, (False, True, True))])
def test_forward_is_bit_identical_with_both_switches_off_and_on(shape, dtype, state_dict, monkeypatch):
    H, W, zn, zpx, interp = shape
    inp = synthetic.make_inputs(2, H, W, zn, zpx, seed=31, drop_hist=0.25)
    geos = [FusionGeometry.from_patch_info(inp["additional"]["patch_info"], s) for s in (4, 8, 16)]
    assert tuple(g.interpolate for g in geos) == interp
    if zn == 8:
        for s in (4, 8, 16):
            h, w = H // s, W // s
            ws = spec.window_size((480 // s, 640 // s))      # the model's windows: 12 / 9 / 6
            assert h % ws or w % ws, (s, h, w, ws)
    dinp = synthetic.to_device(inp, DEV)
    res = []
    for on in ("0", "1"):
        monkeypatch.setenv("CFP_KV_PROJECT", on)
        monkeypatch.setenv("CFP_X2I_INPLACE", on)
        eng = Engine(state_dict, layer_names=spec.COMBINE1_LAYERS, dtype=dtype)
        assert eng.kv_project == (on == "1") and eng.x2i_inplace == (on == "1")
        res.append([t.clone() for t in eng.forward(dinp)])
        torch.cuda.synchronize()
        del eng
    for name, a, b in zip(("bin_edges", "pred", "prob"), res[0], res[1]):
        assert bool(torch.isfinite(a.float()).all()), name
        assert torch.equal(a, b), (name, shape, dtype)
