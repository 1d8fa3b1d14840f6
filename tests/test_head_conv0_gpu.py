"""cfp_depth_head_conv0_fused (csrc/head_conv0.hip): decoder.conv0 computed inside the fused head, `unet` kept on the chip.

The reference of every assertion is the pair the kernel replaces, on the same inputs: cfp_conv2d_nhwc for conv0 into a `unet` buffer, then
cfp_depth_head_fused.  `unet` is computed and rounded as conv0 stores it and is zero outside the image, so prob and pred must be the
pair's BIT FOR BIT -- no tolerance.  Shapes are the smallest at which the 16 x 16 tiling can go wrong."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from cfpnet_amd import hip, ops

DEV = "cuda:0"
HALF = [torch.bfloat16, torch.float16]


def _rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def _ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _act(x2d, dtype, ld):
    rows, C = x2d.shape
    buf = torch.zeros(rows, ld, dtype=dtype, device=DEV)
    buf[:, :C] = x2d.to(dtype).to(DEV)
    return ops.Act(buf, 0, C)


def _pack(w, dtype):      # [Cout, Cin, 3, 3] -> [Cout][kh][kw][Cin] as cfp_conv2d_nhwc lays weights out
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).to(dtype).to(DEV).contiguous()


def _case(B, H, W, dtype, integers=False, frame=False):
    """The operands of both paths (CPU float32, already representable in `dtype` where the device stores them in it)."""
    M = B * H * W
    if integers:      # every product and partial sum of both 3x3 convolutions is an exact float32: any summation order gives the same bits
        t = _ints((M, 32), -3, 3, 1)
        w0 = _ints((128, 32, 3, 3), -2, 2, 2)
        b0 = _ints((128,), -4, 4, 3)
        w3 = _ints((128, 128, 3, 3), -1, 1, 4)
        s3 = torch.full((128,), 2.0 ** -10)
        b3 = _ints((128,), -2, 2, 5) * 0.25
    else:
        t = _rnd(M, 32, seed=1).to(dtype).float()
        w0 = _rnd(128, 32, 3, 3, seed=2, scale=1.0 / math.sqrt(9 * 32)).to(dtype).float()
        b0 = _rnd(128, seed=3, scale=0.5)
        w3 = _rnd(128, 128, 3, 3, seed=4, scale=1.0 / math.sqrt(9 * 128)).to(dtype).float()
        s3 = None
        b3 = _rnd(128, seed=5, scale=0.5)
    if frame:         # t = 0 in a two-pixel frame and a bias well away from 0: unet is exactly the bias on the image's border ring, and 0 outside
        t4 = t.reshape(B, H, W, 32).clone()
        t4[:, :2] = 0; t4[:, -2:] = 0; t4[:, :, :2] = 0; t4[:, :, -2:] = 0
        t = t4.reshape(M, 32)
        b0 = b0.abs() + 0.75
    wo = _rnd(256, 128, seed=6, scale=0.6)
    bo = _rnd(256, seed=7)
    centers = torch.sort(torch.rand(B, 256, generator=torch.Generator().manual_seed(8)) * 10, dim=1)[0]
    return dict(t=t, w0=w0, b0=b0, w3=w3, s3=s3, b3=b3, wo=wo, bo=bo, centers=centers)


def _run_both(c, B, H, W, dtype, ld=32):
    """-> (pred, prob) of the pair, (pred, prob) of the fused kernel."""
    M = B * H * W
    ta = _act(c["t"], dtype, ld)
    w0p, w3p = _pack(c["w0"], dtype), _pack(c["w3"], dtype)
    wop = ops.permute_wout(c["wo"], dtype, hilo=False).to(DEV)
    b0, b3, bo, cen = c["b0"].to(DEV), c["b3"].to(DEV), c["bo"].to(DEV), c["centers"].to(DEV)
    s3 = c["s3"].to(DEV) if c["s3"] is not None else None
    # the pair
    unet = ops.new_act(M, 128, dtype, DEV)
    need = ops.conv2d_ws_bytes(M, 128, 9 * 32, ta.dt)
    ws = torch.zeros((need + 3) // 4, dtype=torch.float32, device=DEV) if need else None
    ops.conv2d(ta, w0p, None, b0, unet, B, H, W, 3, 3, 1, 1, 1, H, W, hip.ACT_NONE, None, ws)
    prob0 = torch.zeros(B, 256, H * W, dtype=dtype, device=DEV)
    pred0 = torch.zeros(M, device=DEV)
    ops.depth_head_fused(unet, w3p, s3, b3, wop, bo, cen, prob0, pred0, B, H, W, ram_hilo=False)
    # one launch
    prob1 = torch.full((B, 256, H * W), 7.0, dtype=dtype, device=DEV)
    pred1 = torch.full((M,), 7.0, device=DEV)
    ops.depth_head_conv0_fused(ta, w0p, None, b0, w3p, s3, b3, wop, bo, cen, prob1, pred1, B, H, W)
    pred2 = torch.full((M,), 7.0, device=DEV)
    ops.depth_head_conv0_fused(ta, w0p, None, b0, w3p, s3, b3, wop, bo, cen, None, pred2, B, H, W)      # no prob output: the same pred
    torch.cuda.synchronize()
    assert torch.equal(pred1, pred2)
    return (pred0, prob0), (pred1, prob1)


def _assert_identical(ref, got, B, H, W, what):
    (pred0, prob0), (pred1, prob1) = ref, got
    dp = (pred0.view(torch.int32) != pred1.view(torch.int32)).reshape(B, H, W)
    dq = (prob0.view(torch.int16) != prob1.view(torch.int16)).any(1).reshape(B, H, W)
    bad = (dp | dq).nonzero()
    print(f"{what}: {int(dp.sum())} pred and {int(dq.sum())} prob pixels of {B * H * W} differ; first {bad[:6].tolist()}")
    assert bad.numel() == 0, what


# one tile with every border at once | tile seams in both directions, a tile row that ends one image and the next that starts another |
# three images of two tiles | a pitch wider than the 32 channels (the engine passes slices)
SHAPES = [(1, 16, 16, 32), (2, 32, 48, 32), (3, 16, 32, 32), (3, 16, 32, 40)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("B,H,W,ld", SHAPES)
def test_bit_identical_to_the_pair(B, H, W, ld, dtype):
    """Random operands that exercise the rounding of `unet` and `ram` to the storage type."""
    c = _case(B, H, W, dtype)
    ref, got = _run_both(c, B, H, W, dtype, ld)
    _assert_identical(ref, got, B, H, W, f"random {dtype} {B}x{H}x{W} ld {ld}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", HALF)
def test_bit_identical_on_small_integers(dtype):
    """Small-integer operands: every summation order of the two 3x3 convolutions is exact, so a difference here is a wrong tap or border,
    not a re-association."""
    B, H, W = 2, 32, 48
    c = _case(B, H, W, dtype, integers=True)
    ref, got = _run_both(c, B, H, W, dtype)
    _assert_identical(ref, got, B, H, W, f"integers {dtype}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", HALF)
def test_unet_is_zero_outside_the_image(dtype):
    """The head pads unet, not t.  With a conv0 bias away from 0 and t = 0 in a two-pixel frame, a halo that holds conv0 of the zero-padded t
    outside the image (= the bias) instead of 0 changes every border pixel and no other.  Checked against the pair bit for bit, and
    against the float64 chain with the tolerances test_depth_head_fused uses, which the wrong padding rule exceeds on the border."""
    B, H, W = 1, 32, 32
    c = _case(B, H, W, dtype, frame=True)
    ref, got = _run_both(c, B, H, W, dtype)
    _assert_identical(ref, got, B, H, W, f"frame {dtype}")

    def chain(pad_unet_with_bias):
        t = c["t"].double().reshape(B, H, W, 32).permute(0, 3, 1, 2)
        unet = F.conv2d(t, c["w0"].double(), c["b0"].double(), padding=1).float().to(dtype).double()
        if pad_unet_with_bias:
            up = c["b0"].float().to(dtype).double()[None, :, None, None].expand(B, 128, H + 2, W + 2).clone()
            up[:, :, 1:-1, 1:-1] = unet
            ram = F.conv2d(up, c["w3"].double(), c["b3"].double())
        else:
            ram = F.conv2d(unet, c["w3"].double(), c["b3"].double(), padding=1)
        logits = F.conv2d(ram.float().to(dtype).double(), c["wo"].to(dtype).double()[:, :, None, None], c["bo"].double())
        return torch.softmax(logits, dim=1).reshape(B, 256, H * W).float()

    tol = 2e-3 if dtype == torch.float16 else 1.2e-2
    right, wrong = chain(False), chain(True)
    err = (got[1].float().cpu() - right).abs().max()
    gap = (wrong - right).abs().amax(1).reshape(B, H, W)
    border = torch.ones(H, W, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    print(f"frame {dtype}: max prob error vs float64 {float(err):.3e} (bound {tol}); wrong padding rule moves the border by "
          f"{float(gap[:, border].min()):.3e} .. {float(gap[:, border].max()):.3e}, the interior by {float(gap[:, ~border].max()):.3e}")
    assert float(gap[:, ~border].max()) < 1e-6 and float(gap[:, border].max()) > 4 * tol      # the check has teeth, on the border only
    assert float(err) < tol


@pytest.mark.gpu
def test_shape_without_whole_tiles_is_refused():
    """24 x 40 is not whole 16 x 16 tiles: no tail-tile path, CFP_ESHAPE, the engine runs the pair."""
    B, H, W = 1, 24, 40
    assert not ops.depth_head_conv0_fits(H, W) and ops.depth_head_conv0_fits(240, 320)
    c = _case(B, H, W, torch.bfloat16)
    with pytest.raises(RuntimeError, match=r"cfp_depth_head_conv0_fused failed \(-2\).*16 x 16"):
        _run_both(c, B, H, W, torch.bfloat16)


def test_argument_errors():
    """Invalid arguments return their code and a message before anything is launched (16 = a non-null, 16-byte aligned dummy pointer;
    nothing is dereferenced): this runs without a GPU."""
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = hip.load()
    P = 16

    def call(*args):
        return lib.cfp_depth_head_conv0_fused(*args), hip.last_error()

    # (t, t_ld, w0, scale0, shift0, w3, scale3, shift3, wout_perm, bias_out, centers, prob, pred, B, H, W, flags, dtype, stream)
    rc, msg = call(P, 32, P, 0, 0, P, 0, 0, P, P, P, 0, 0, 1, 16, 16, 0, hip.BF16, 0)
    assert rc == -1 and "null" in msg                                   # null pred
    rc, msg = call(P, 32, 0, 0, 0, P, 0, 0, P, P, P, 0, P, 1, 16, 16, 0, hip.BF16, 0)
    assert rc == -1 and "null" in msg                                   # null conv0 weights
    rc, msg = call(P, 32, P, 0, 0, P, 0, 0, P, P, P, 0, P, 1, 16, 16, 0, hip.F32, 0)
    assert rc == -1 and "bf16/f16 only" in msg
    rc, msg = call(P + 8, 32, P, 0, 0, P, 0, 0, P, P, P, 0, P, 1, 16, 16, 0, hip.F16, 0)
    assert rc == -1 and "16-byte aligned" in msg
    rc, msg = call(P, 32, P, 0, 0, P, 0, 0, P, P, P, 0, P, 1, 24, 40, 0, hip.BF16, 0)
    assert rc == -2 and "16 x 16" in msg                                # not whole tiles
    rc, msg = call(P, 24, P, 0, 0, P, 0, 0, P, P, P, 0, P, 1, 16, 16, 0, hip.BF16, 0)
    assert rc == -2 and "32 input channels" in msg                      # pitch below the 32 channels
    rc, msg = call(P, 32, P, 0, 0, P, 0, 0, P, P, P, 0, P, 4096, 512, 512, 0, hip.BF16, 0)
    assert rc == -2 and "2 GB" in msg                                   # 32-bit byte offsets
    rc, msg = call(P, 32, P, 0, 0, P, 0, 0, P, P, P, 0, P, 1, 16, 16, 1, hip.BF16, 0)
    assert rc == -1 and "flags" in msg


@pytest.mark.gpu
def test_engine_switch_gives_the_same_forward(monkeypatch):
    """A whole forward with CFP_HEAD_CONV0=1 and =0, each in its own engine: edges, pred and prob identical; the plan of the fused run holds
    no `unet` buffer and the other one does."""
    from cfpnet_amd import spec, synthetic, weights
    from cfpnet_amd.engine import Engine
    layers = spec.COMBINE1_LAYERS
    sd = weights.make_torch_state_dict(spec.model_manifest(layers))
    inp = synthetic.to_device(synthetic.make_inputs(1, 480, 640, 8, 56, seed=11), DEV)
    outs, has_unet = [], []
    for v in ("1", "0"):
        monkeypatch.setenv("CFP_HEAD_CONV0", v)
        eng = Engine(sd, layer_names=layers, dtype=torch.bfloat16)
        assert eng.head_conv0 == (v == "1")
        e, p, pr = eng.forward(inp)
        torch.cuda.synchronize()
        outs.append((e.clone(), p.clone(), pr.clone()))
        has_unet.append(any("unet" in plan["bufs"] for plan in eng._plans.values()))
        del eng
    assert has_unet == [False, True]
    for a, b, what in zip(outs[0], outs[1], ("edges", "pred", "prob")):
        assert torch.equal(a, b), what
