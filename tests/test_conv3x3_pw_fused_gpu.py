"""cfp_conv3x3_pw_fused (3x3 conv -> BN -> activation -> 1x1 conv -> BN (+ skip) in one launch, the expanded tensor kept on the chip)
against the two cfp_conv2d_nhwc launches it replaces, and the engine's forward with the fused EdgeResidual blocks against the unfused one."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import rel_l1  # noqa: E402
from cfpnet_amd import hip, ops, spec, synthetic, weights  # noqa: E402
from cfpnet_amd.engine import Engine  # noqa: E402
from oracle import cfpnet_oracle as O  # noqa: E402
from test_forward_gpu import TOL_BF16, TOL_F16  # noqa: E402
from test_ops_gpu import DEV, HALF, close, from_nhwc, nhwc, q, rnd, to_act  # noqa: E402

# B, H, W, Cin, mid, Cout, stride, pads (t, l, b, r), skip, act of the 3x3, extra columns behind the output slice
MODEL_CASES = [
    (1, 240, 320, 16, 64, 40, 2, (0, 0, 1, 1), False, hip.ACT_SILU, 0),      # conv1.0
    (1, 120, 160, 40, 160, 40, 1, (1, 1, 1, 1), True, hip.ACT_SILU, 0),      # conv1.1, conv1.2
    (2, 120, 160, 40, 160, 56, 2, (0, 0, 1, 1), False, hip.ACT_SILU, 0),     # conv2.0
    (2, 60, 80, 56, 224, 56, 1, (1, 1, 1, 1), True, hip.ACT_SILU, 0),        # conv2.1, conv2.2
    (1, 120, 160, 64, 64, 32, 1, (1, 1, 1, 1), False, hip.ACT_LRELU, 32),    # decoder up3.b -> conv1 into the dcat3 slice
]
RAGGED_CASES = [
    (2, 21, 35, 40, 160, 40, 1, (1, 1, 1, 1), True, hip.ACT_SILU, 24),       # W not a multiple of 16, rows not a multiple of the tile
    (1, 5, 70, 56, 224, 56, 1, (1, 1, 1, 1), False, hip.ACT_SILU, 0),        # fewer rows than a tile
    (1, 13, 19, 16, 64, 32, 1, (1, 1, 1, 1), True, hip.ACT_LRELU, 8),
    (3, 9, 11, 24, 64, 56, 1, (0, 2, 2, 0), False, hip.ACT_SILU, 0),         # asymmetric padding
    (1, 17, 18, 8, 160, 32, 1, (1, 1, 1, 1), True, hip.ACT_LRELU, 40),       # one chunk per pixel
    (1, 9, 33, 40, 224, 40, 1, (1, 1, 1, 1), False, hip.ACT_LRELU, 0),
    (1, 21, 35, 40, 160, 56, 2, (1, 1, 1, 1), False, hip.ACT_SILU, 16),      # stride 2 on odd sizes
    (2, 24, 32, 16, 64, 40, 2, (0, 0, 1, 1), False, hip.ACT_SILU, 0),
    (1, 10, 20, 8, 48, 24, 1, (1, 1, 1, 1), True, hip.ACT_SILU, 0),          # channel counts that fill no tile / K block exactly
    (1, 12, 16, 32, 144, 48, 1, (1, 1, 1, 1), True, hip.ACT_NONE, 0),
]


def _act_ref(x, act):
    return {hip.ACT_NONE: lambda v: v, hip.ACT_SILU: F.silu, hip.ACT_LRELU: lambda v: F.leaky_relu(v, 0.01)}[act](x)


def _run_pair(case, dtype, x, w1, s1, t1, w2, s2, t2, res, act2=hip.ACT_NONE):
    """-> (fused, unfused, neighbours untouched) on the same 16-bit operands; the unfused expand is forced onto the fused launch's halo variant."""
    B, H, W, Cin, mid, Cout, s, (pt, pl, pb, pr), skip, act1, extra = case
    lib = hip.load()
    Ho, Wo = (H + pt + pb - 3) // s + 1, (W + pl + pr - 3) // s + 1
    M = B * Ho * Wo
    v = ops.conv3x3_pw_fused_variant(Cin, mid, Cout, s, ops.DT[dtype])
    assert v >= 0, case
    xa = to_act(nhwc(x), dtype, ld=Cin + 16, c0=8)
    w1a = w1.permute(0, 2, 3, 1).reshape(mid, 9 * Cin).contiguous().to(dtype).to(DEV)
    w2a = w2.to(dtype).to(DEV).contiguous()
    dev = lambda t: None if t is None else t.to(DEV)
    ra = to_act(nhwc(res), dtype, ld=Cout + 8) if skip else None
    outs = []
    for fused in (True, False):
        buf = ops.new_act(M, Cout + 24 + extra, dtype, DEV, zero=True)      # an output slice: 16 columns before it, 8 + extra behind
        out = ops.Act(buf.buf, 16, Cout)
        if fused:
            ops.conv3x3_pw_fused(xa, w1a, dev(s1), dev(t1), act1, ops.pad_pw_w(w2a), dev(s2), dev(t2), out, B, H, W, s, pt, pl, Ho, Wo,
                                 act2, ra)
        else:
            midb = ops.new_act(M, mid, dtype, DEV)
            try:
                lib.cfp_debug_set(0, 300 + v)
                ops.conv2d(xa, w1a, dev(s1), dev(t1), midb, B, H, W, 3, 3, s, pt, pl, Ho, Wo, act1, None, None)
            finally:
                lib.cfp_debug_set(0, -1)
            nws = ops.conv2d_ws_bytes(M, Cout, mid, ops.DT[dtype])
            ws = torch.empty(max(nws // 4, 1), device=DEV) if nws else None
            ops.conv2d(midb, w2a, dev(s2), dev(t2), out, B, Ho, Wo, 1, 1, 1, 0, 0, Ho, Wo, act2, ra, ws)
        torch.cuda.synchronize()
        assert float(buf.buf[:, :16].abs().max()) == 0 and float(buf.buf[:, 16 + Cout:].abs().max()) == 0, f"slice neighbours written {case}"
        outs.append(out.torch().clone())
    return outs[0], outs[1], (B, Ho, Wo)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("case", MODEL_CASES + RAGGED_CASES)
def test_fused_matches_the_two_launches(case, dtype):
    """Same 16-bit operands through the fused launch and through expand (same halo variant) + 1x1: both round `mid` identically, so the
    only difference allowed is float32 re-association in the second GEMM -- the halo-against-implicit-GEMM bound of test_ops_gpu.py: <= 2 ulp
    of the storage type relative to max(|b|, 1), fewer than 2 % of the elements differing -- and the kernel leaves none: bit-identical.  And
    against float32 torch."""
    B, H, W, Cin, mid, Cout, s, (pt, pl, pb, pr), skip, act1, extra = case
    x = q(rnd(B, Cin, H, W, seed=1), dtype)
    w1 = q(rnd(mid, Cin, 3, 3, seed=2, scale=1.0 / math.sqrt(9 * Cin)), dtype)
    w2 = q(rnd(Cout, mid, seed=3, scale=1.0 / math.sqrt(mid)), dtype)
    s1, t1 = rnd(mid, seed=4).abs() + 0.5, rnd(mid, seed=5)
    s2, t2 = rnd(Cout, seed=6).abs() + 0.5, rnd(Cout, seed=7)
    Ho, Wo = (H + pt + pb - 3) // s + 1, (W + pl + pr - 3) // s + 1
    res = q(rnd(B, Cout, Ho, Wo, seed=8), dtype)
    m = F.conv2d(F.pad(x, (pl, pr, pt, pb)), w1, None, s)
    m = q(_act_ref(m * s1[None, :, None, None] + t1[None, :, None, None], act1), dtype)      # the expanded tensor is a 16-bit tensor
    ref = F.conv2d(m, w2[:, :, None, None]) * s2[None, :, None, None] + t2[None, :, None, None]
    if skip:
        ref = ref + res
    a, b2, (B_, Ho_, Wo_) = _run_pair(case, dtype, x, w1, s1, t1, w2, s2, t2, res)
    a32, b32 = a.float(), b2.float()
    ulp = 2.0 ** (-7 if dtype == torch.bfloat16 else -10)
    worst = float(((a32 - b32).abs() / b32.abs().clamp(min=1.0)).max())
    frac = float((a32 != b32).float().mean())
    print(f"fused vs pair {case} {dtype}: max rel diff {worst:.3e} ({worst / ulp:.2f} ulp), differing {100 * frac:.3f} %")
    assert worst <= 2 * ulp, f"fused vs pair {case}"
    assert frac < 0.02, f"fused vs pair {case}: {frac}"
    # the fused 1x1 walks the K blocks in the order of the launch it replaces, into one accumulator: not even re-association is left
    assert torch.equal(a.view(torch.int16), b2.view(torch.int16)), f"fused vs pair {case}: bits differ"
    close(from_nhwc(a, B, Ho, Wo), ref, dtype, f"fused 3x3 -> 1x1 {case}")


@pytest.mark.parametrize("dtype", HALF)
def test_fused_with_a_leaky_relu_behind_the_1x1(dtype):
    """The 1x1's own activation (none or LeakyReLU): same bound against the pair."""
    case = (2, 21, 35, 40, 160, 40, 1, (1, 1, 1, 1), True, hip.ACT_SILU, 8)
    B, H, W, Cin, mid, Cout, s, (pt, pl, pb, pr), skip, act1, extra = case
    x = q(rnd(B, Cin, H, W, seed=11), dtype)
    w1 = q(rnd(mid, Cin, 3, 3, seed=12, scale=1.0 / math.sqrt(9 * Cin)), dtype)
    w2 = q(rnd(Cout, mid, seed=13, scale=1.0 / math.sqrt(mid)), dtype)
    res = q(rnd(B, Cout, H, W, seed=14), dtype)
    a, b2, _ = _run_pair(case, dtype, x, w1, rnd(mid, seed=15).abs() + 0.5, rnd(mid, seed=16), w2, rnd(Cout, seed=17).abs() + 0.5, rnd(Cout, seed=18), res,
                         act2=hip.ACT_LRELU)
    a32, b32 = a.float(), b2.float()
    ulp = 2.0 ** (-7 if dtype == torch.bfloat16 else -10)
    assert float((b32 < 0).float().mean()) > 0.2
    assert float(((a32 - b32).abs() / b32.abs().clamp(min=1.0)).max()) <= 2 * ulp and float((a32 != b32).float().mean()) < 0.02
    xa = ops.new_act(64, 40, dtype, DEV, zero=True)
    with pytest.raises(RuntimeError, match="bad activation"):
        ops.conv3x3_pw_fused(xa, torch.zeros(160, 360, dtype=dtype, device=DEV), None, None, hip.ACT_SILU, torch.zeros(48, 160, dtype=dtype, device=DEV),
                             None, None, ops.new_act(64, 40, dtype, DEV), 1, 8, 8, 1, 1, 1, 8, 8, act2=hip.ACT_SILU)


def _int_tensor(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("case", [
    (2, 20, 24, 40, 160, 40, 1, (1, 1, 1, 1), True, hip.ACT_NONE, 0), (1, 11, 16, 56, 224, 56, 1, (0, 1, 1, 0), True, hip.ACT_NONE, 8),
    (1, 17, 33, 16, 64, 32, 1, (1, 1, 1, 1), False, hip.ACT_NONE, 0), (1, 21, 35, 40, 160, 56, 2, (1, 1, 1, 1), False, hip.ACT_NONE, 0),
    (2, 24, 32, 16, 64, 40, 2, (0, 0, 1, 1), False, hip.ACT_NONE, 0)])
def test_fused_is_bit_identical_on_small_integers(case, dtype):
    """Integer inputs and weights, no activation in the middle: `mid` is rounded identically by both paths and every float32 sum of the
    second GEMM is exact, so the bits agree."""
    B, H, W, Cin, mid, Cout, s, (pt, pl, pb, pr), skip, act1, extra = case
    x = _int_tensor((B, Cin, H, W), -3, 3, 1)
    w1 = _int_tensor((mid, Cin, 3, 3), -2, 2, 2)
    w2 = _int_tensor((Cout, mid), -2, 2, 3)
    Ho, Wo = (H + pt + pb - 3) // s + 1, (W + pl + pr - 3) // s + 1
    res = _int_tensor((B, Cout, Ho, Wo), -4, 4, 4)
    a, b2, _ = _run_pair(case, dtype, x, w1, None, None, w2, None, None, res)
    assert float(a.float().abs().max()) > 0
    assert torch.equal(a.view(torch.int16), b2.view(torch.int16)), f"fused != pair on integers {case}"
    m = F.conv2d(F.pad(x.double(), (pl, pr, pt, pb)), w1.double(), None, s).float().to(dtype).double()
    ref = F.conv2d(m, w2.double()[:, :, None, None]).float().to(dtype)
    if skip:
        ref = (ref.float() + res).to(dtype)
    got = a.cpu().reshape(B, Ho, Wo, Cout).permute(0, 3, 1, 2)
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), f"fused integers vs float64 {case}"


def test_shapes_outside_the_preconditions_are_refused():
    lib = hip.load()
    assert ops.conv3x3_pw_fused_variant(40, 160, 40, 1, hip.BF16) == 5 and ops.conv3x3_pw_fused_variant(56, 224, 56, 1, hip.F16) == 6
    assert ops.conv3x3_pw_fused_variant(16, 64, 40, 2, hip.BF16) == 2
    for bad in [(40, 256, 40, 1, hip.BF16), (40, 160, 72, 1, hip.BF16), (40, 160, 40, 1, hip.F32), (56, 224, 56, 2, hip.BF16), (40, 160, 36, 1, hip.BF16),
                (136, 160, 40, 1, hip.BF16), (40, 160, 40, 3, hip.BF16)]:
        assert ops.conv3x3_pw_fused_variant(*bad) == -1, bad
    x = ops.new_act(64, 40, torch.bfloat16, DEV, zero=True)
    w1 = torch.zeros(256, 360, dtype=torch.bfloat16, device=DEV)
    w2 = torch.zeros(48, 256, dtype=torch.bfloat16, device=DEV)
    out = ops.new_act(64, 40, torch.bfloat16, DEV, zero=True)
    with pytest.raises(RuntimeError, match="shape not taken"):
        ops.conv3x3_pw_fused(x, w1, None, None, hip.ACT_SILU, w2, None, None, out, 1, 8, 8, 1, 1, 1, 8, 8)
    assert lib.cfp_conv3x3_pw_fused(0, 40, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 40, 1, 8, 8, 40, 160, 40, 1, 1, 1, 8, 8, hip.BF16, 0) == -1


def _forward_recorded(monkeypatch, sd, layers, inp, dtype, fused, taps=None):
    names = []
    real = hip.call

    def rec(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setenv("CFP_ER_FUSED", fused)
    monkeypatch.setattr(hip, "call", rec)
    eng = Engine(sd, layer_names=layers, dtype=dtype)
    e, p, pr = eng.forward(inp, taps=taps)
    torch.cuda.synchronize()
    monkeypatch.setattr(hip, "call", real)
    return p.clone(), names, eng


@pytest.mark.parametrize("dtype,bound", [(torch.bfloat16, TOL_BF16), (torch.float16, TOL_F16)])
def test_engine_forward_fused_against_unfused(dtype, bound, monkeypatch):
    """The same weights and inputs with CFP_ER_FUSED=1 and =0: the fused run takes the new entry point once per fused block and makes two
    fewer cfp_conv2d_nhwc* calls per fused block; its prediction meets test_forward_gpu.py's tolerance against the CPU oracle for that
    storage type (the fusion only changes the summation order of one GEMM per block); a forward that asks for taps runs unfused and
    returns every tap."""
    layers = spec.COMBINE1_LAYERS
    sd = weights.make_torch_state_dict(spec.model_manifest(layers))
    inp = synthetic.make_inputs(2, 480, 640, 8, 56, seed=21, drop_hist=0.2)
    e0, p0, pr0 = O.forward(sd, inp, layer_names=layers)
    pu, nu, _ = _forward_recorded(monkeypatch, sd, layers, inp, dtype, "0")
    pf, nf, eng = _forward_recorded(monkeypatch, sd, layers, inp, dtype, "1")
    blocks = sum(1 for b in spec.ENC_BLOCKS if b.kind == "er" and b.stride == 1)
    convs = lambda names: sum(1 for n in names if n.startswith("cfp_conv2d_nhwc"))
    assert blocks == 4 and nu.count("cfp_conv3x3_pw_fused") == 0
    assert nf.count("cfp_conv3x3_pw_fused") == blocks and convs(nu) - convs(nf) == 2 * blocks
    assert not any(k.endswith(".mid") and k.startswith("enc") and spec.ENC_BLOCKS[int(k[3:-4])].kind == "er" and spec.ENC_BLOCKS[int(k[3:-4])].stride == 1
                   for plan in eng._plans.values() for k in plan["bufs"])
    ru, rf = rel_l1(pu.cpu().numpy(), p0.numpy()), rel_l1(pf.cpu().numpy(), p0.numpy())
    print(f"{dtype}: pred relL1 vs CPU oracle unfused {ru:.4e} fused {rf:.4e}; fused vs unfused {rel_l1(pf.cpu().numpy(), pu.cpu().numpy()):.3e}")
    assert rf < bound and ru < bound
    assert torch.equal(pf, pu)          # same sums in the same order: the fused forward is the unfused one bit for bit
    # every stride / decoder option of the switch still meets the tolerance
    pa, na, _ = _forward_recorded(monkeypatch, sd, layers, inp, dtype, "12d")
    assert na.count("cfp_conv3x3_pw_fused") == sum(1 for b in spec.ENC_BLOCKS if b.kind == "er") + 1
    assert convs(nu) - convs(na) == 2 * na.count("cfp_conv3x3_pw_fused")
    ra = rel_l1(pa.cpu().numpy(), p0.numpy())
    print(f"{dtype}: CFP_ER_FUSED=12d pred relL1 vs CPU oracle {ra:.4e}")
    assert ra < bound and torch.equal(pa, pu)
    # taps: the unfused path, every tap present, bit for bit the forward with taps of the unfused engine
    tu, tf = {}, {}
    ptu, _, _ = _forward_recorded(monkeypatch, sd, layers, inp, dtype, "0", taps=tu)
    pt, nt, _ = _forward_recorded(monkeypatch, sd, layers, inp, dtype, "1", taps=tf)
    assert nt.count("cfp_conv3x3_pw_fused") == 0 and set(tf) == set(tu) and len(tf) > 0
    assert torch.equal(pt, ptu)
    for k in tu:
        assert torch.equal(tf[k], tu[k]), k
