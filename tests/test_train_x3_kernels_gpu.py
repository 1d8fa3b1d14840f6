"""The f16x3 training kernels (float32 tensors, split-precision matrix math in the dense-convolution backward) against float64
PyTorch on the CPU copy: the weight gradient (cfp_conv2d_wgrad_x3 / cfp_conv2d_wgrad with CFP_F32X3), the data gradient
(cfp_conv2d_dgrad_x3 over the pre-split flipped weights), the power-of-two dY scale (exact: results scale bit for bit) and the batched
packing of the pre-split operands (cfp_pack_w_x3_batch == cfp_conv2d_weight_flip + cfp_pack_w_x3)."""

import pytest
import torch
import torch.nn.functional as F

from cfpnet_amd import hip, ops, train_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = [  # B, H, W, Cin, Cout, k, stride, pads (t, l, b, r)
    (2, 12, 16, 16, 24, 3, 1, (1, 1, 1, 1)),
    (2, 9, 11, 8, 40, 3, 2, (0, 0, 1, 1)),        # stem-like: stride 2, TF SAME on odd sizes
    (2, 33, 35, 8, 32, 3, 2, (0, 0, 1, 1)),       # stem: Cin 3 padded to 8 (K = 72, a ragged K tile)
    (1, 10, 14, 16, 64, 3, 2, (0, 0, 1, 1)),
    (3, 8, 8, 136, 816, 1, 1, (0, 0, 0, 0)),      # pointwise, ragged Cout tile
    (1, 1, 300, 64, 128, 1, 1, (0, 0, 0, 0)),     # Linear
    (1, 1, 500, 8, 24, 1, 1, (0, 0, 0, 0)),       # Linear, K = 8 (not a multiple of 32)
    (1, 32, 48, 32, 32, 4, 4, (0, 0, 0, 0)),      # patch convs: kernel = stride
    (1, 40, 48, 16, 32, 8, 8, (0, 0, 0, 0)),
    (1, 36, 48, 16, 64, 12, 12, (0, 0, 0, 0)),
    (2, 64, 80, 24, 64, 3, 1, (1, 1, 1, 1)),      # 10 240 rows, K = 216
]
IDS = [f"b{c[0]}_{c[1]}x{c[2]}_{c[3]}to{c[4]}_k{c[5]}s{c[6]}" for c in CASES]


def _rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _geom(c):
    B, H, W, Cin, Cout, k, s, (pt, pl, pb, pr) = c
    return B, H, W, Cin, Cout, k, s, pt, pl, (H + pt + pb - k) // s + 1, (W + pl + pr - k) // s + 1


def _data(c, seed=1):
    B, H, W, Cin, Cout, k, s, pt, pl, Ho, Wo = _geom(c)
    x = _rnd(B * H * W, Cin, seed=seed)
    dy = _rnd(B * Ho * Wo, Cout, seed=seed + 1) * 1e-3
    w = _rnd(Cout, k * k * Cin, seed=seed + 2) / (k * (Cin ** 0.5))
    return x, dy, w


def _ref(c, x, dy, w):
    """float64 autograd of the padded convolution -> (dW [Cout, k*k*Cin], dX [B*H*W, Cin])."""
    B, H, W, Cin, Cout, k, s, pt, pl, Ho, Wo = _geom(c)
    pads = c[7]
    xn = x.double().reshape(B, H, W, Cin).permute(0, 3, 1, 2).clone().requires_grad_(True)
    wn = w.double().reshape(Cout, k, k, Cin).permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.conv2d(F.pad(xn, (pads[1], pads[3], pads[0], pads[2])), wn, stride=s)
    assert y.shape == (B, Cout, Ho, Wo)
    y.backward(dy.double().reshape(B, Ho, Wo, Cout).permute(0, 3, 1, 2))
    dw = wn.grad.permute(0, 2, 3, 1).reshape(Cout, k * k * Cin)
    dx = xn.grad.permute(0, 2, 3, 1).reshape(B * H * W, Cin)
    return dw, dx


def _rel(a, ref):
    return float((a.double().cpu() - ref).norm() / ref.norm())


def _wgrad(c, x, dy, dtype, dy_scale=None, x3=False):
    B, H, W, Cin, Cout, k, s, pt, pl, Ho, Wo = _geom(c)
    return train_ops.conv2d_wgrad(x.to(DEV, dtype), dy.to(DEV, dtype), B, H, W, k, k, s, pt, pl, Ho, Wo, x3=x3, dy_scale=dy_scale)


def _dgrad(c, dy, w, dtype, x3=False, scaled=True):
    B, H, W, Cin, Cout, k, s, pt, pl, Ho, Wo = _geom(c)
    wf = train_ops.conv2d_weight_flip(w.to(DEV, torch.float32 if x3 else dtype), Cout, k, k, Cin)
    g = dy.to(DEV, torch.float32 if x3 else dtype)
    if not x3:
        return train_ops.conv2d_dgrad(g, wf, B, H, W, Cin, k, k, s, pt, pl, Ho, Wo)
    sc = train_ops.grad_absmax(g) if scaled else None
    return train_ops.conv2d_dgrad(g, ops.pack_w_x3(wf), B, H, W, Cin, k, k, s, pt, pl, Ho, Wo, x3=True, dy_scale=sc)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_x3_weight_gradient_vs_float64(c):
    x, dy, w = _data(c)
    ref, _ = _ref(c, x, dy, w)
    e32 = _rel(_wgrad(c, x, dy, torch.float32), ref)
    e16 = _rel(_wgrad(c, x, dy, torch.float16), ref)
    g = dy.to(DEV)
    got = _wgrad(c, x, dy, torch.float32, dy_scale=train_ops.grad_absmax(g), x3=True)
    # the plain entry point with dtype CFP_F32X3 (no scale): same kernel
    B, H, W, Cin, Cout, k, s, pt, pl, Ho, Wo = _geom(c)
    K, M = k * k * Cin, B * Ho * Wo
    nb = hip.load().cfp_conv2d_wgrad_ws_bytes(Cout, K, M)
    ws = torch.empty(nb // 4, dtype=torch.float32, device=DEV)
    plain = torch.empty(Cout, K, dtype=torch.float32, device=DEV)
    xd = x.to(DEV)
    # (dY of unit size: unscaled, gradients of 1e-3 would lose their low bits in subnormal lo halves -- what the scale is for)
    g = g * 1024.0
    hip.call("cfp_conv2d_wgrad", xd.data_ptr(), Cin, g.data_ptr(), Cout, plain.data_ptr(), B, H, W, Cin, Cout, k, k, s, pt, pl, Ho, Wo, 0.0,
             hip.F32X3, ws.data_ptr(), nb, hip.current_stream())
    torch.cuda.synchronize()
    ex3, ep = _rel(got, ref), _rel(plain / 1024.0, ref)
    print(f"wgrad {c}: f32 {e32:.2e} f16 {e16:.2e} f32x3 {ex3:.2e} (unscaled {ep:.2e})")
    assert ex3 <= max(4 * e32, 2e-6) and ex3 * 50 <= e16, (ex3, e32, e16)
    assert ep <= max(4 * e32, 2e-6) and ep * 50 <= e16, (ep, e32, e16)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_x3_data_gradient_vs_float64(c):
    B, H, W, Cin, Cout, k, s, pt, pl, Ho, Wo = _geom(c)
    x, dy, w = _data(c)
    _, ref = _ref(c, x, dy, w)
    e32 = _rel(_dgrad(c, dy, w, torch.float32), ref)
    e16 = _rel(_dgrad(c, dy, w, torch.float16), ref)
    ex3 = _rel(_dgrad(c, dy, w, torch.float32, x3=True), ref)
    # the plain entry point (cfp_conv2d_dgrad, dtype CFP_F32X3, no scale; dY of unit size)
    g = dy.to(DEV) * 1024.0
    pkt = ops.pack_w_x3(train_ops.conv2d_weight_flip(w.to(DEV), Cout, k, k, Cin))
    nb = hip.load().cfp_conv2d_dgrad_x3_ws_bytes(B, Ho, Wo, Cout, Cin, s)
    ws = torch.empty(nb // 4, dtype=torch.float32, device=DEV)
    plain = torch.empty(B * H * W, Cin, dtype=torch.float32, device=DEV)
    hip.call("cfp_conv2d_dgrad", g.data_ptr(), Cout, pkt.data_ptr(), plain.data_ptr(), Cin, B, H, W, Cin, Cout, k, k, s, pt, pl, Ho, Wo, 0,
             hip.F32X3, ws.data_ptr(), nb, hip.current_stream())
    torch.cuda.synchronize()
    ep = _rel(plain / 1024.0, ref)
    print(f"dgrad {c}: f32 {e32:.2e} f16 {e16:.2e} f32x3 {ex3:.2e} (unscaled {ep:.2e})")
    assert ex3 <= max(4 * e32, 2e-6) and ex3 * 50 <= e16, (ex3, e32, e16)
    assert ep <= max(4 * e32, 2e-6) and ep * 50 <= e16, (ep, e32, e16)


def test_x3_patch_conv_data_gradient_gemm():
    """The patch-conv route of the tape (k == stride): dY x W as the data gradient of a 1x1 conv over k*k*Cin channels with the
    pre-split TRANSPOSED weights (pack mode 1 of the (Cout, 1, 1, k*k*Cin) geometry)."""
    M, Cout, K = 700, 64, 8 * 8 * 16
    dy, w = _rnd(M, Cout, seed=3) * 1e-4, _rnd(Cout, K, seed=4) * 0.05
    ref = dy.double() @ w.double()
    g = dy.to(DEV)
    got = train_ops.conv2d_dgrad(g, ops.pack_w_x3(w.to(DEV).t().contiguous()), 1, M, 1, K, 1, 1, 1, 0, 0, M, 1, x3=True,
                                 dy_scale=train_ops.grad_absmax(g))
    e32 = _rel(ops_gemm_f32(g, w.to(DEV)), ref)
    ex3 = _rel(got, ref)
    assert ex3 <= max(4 * e32, 2e-6), (ex3, e32)


def ops_gemm_f32(g, w):
    out = torch.empty(g.shape[0], w.shape[1], dtype=torch.float32, device=DEV)
    ops.conv2d(ops.Act(g, 0, g.shape[1]), w.t().contiguous(), None, None, ops.Act(out, 0, w.shape[1]), 1, 1, g.shape[0], 1, 1, 1, 0, 0, 1, g.shape[0])
    return out


@pytest.mark.parametrize("c", [CASES[0], CASES[1], CASES[5], CASES[8]], ids=[IDS[0], IDS[1], IDS[5], IDS[8]])
@pytest.mark.parametrize("p2", [-40, 30])
def test_x3_gradient_scale_is_exact(c, p2):
    """dY * 2^p through both GEMMs = (the results for dY) * 2^p, bit for bit: the scale is a power of two taken from max|dY|, so the
    split operand is the same and only exact power-of-two multiplications differ."""
    x, dy, w = _data(c)
    f = 2.0 ** p2
    g0, g1 = dy.to(DEV), (dy * f).to(DEV)
    assert torch.equal(g1 / f, g0)
    dw0 = _wgrad(c, x, dy, torch.float32, dy_scale=train_ops.grad_absmax(g0), x3=True)
    dw1 = _wgrad(c, x, dy * f, torch.float32, dy_scale=train_ops.grad_absmax(g1), x3=True)
    dx0 = _dgrad(c, dy, w, torch.float32, x3=True)
    dx1 = _dgrad(c, dy * f, w, torch.float32, x3=True)
    torch.cuda.synchronize()
    assert bool(dw0.abs().max() > 0) and bool(dx0.abs().max() > 0)
    assert torch.equal(dw1, dw0 * f) and torch.equal(dx1, dx0 * f)
    # without the scale the tiny gradient loses its bits in the halves: the scale is what keeps it
    if p2 < 0:
        dw_raw = _wgrad(c, x, dy * f, torch.float32, x3=True)
        assert not torch.equal(dw_raw, dw0 * f)


def test_pack_w_x3_batch_equals_flip_and_pack():
    shapes = [(24, 3, 3, 16, 0), (24, 3, 3, 16, 1), (40, 3, 3, 8, 1), (816, 1, 1, 136, 0), (816, 1, 1, 136, 1), (32, 1, 1, 12 * 12 * 16, 1),
              (32, 12, 12, 16, 0), (36, 1, 1, 8, 0)]
    lib = hip.load()
    srcs, off = [], 0
    for i, (co, kh, kw, ci, _) in enumerate(shapes):
        srcs.append((off, _rnd(co, kh * kw * ci, seed=10 + i)))
        off += co * kh * kw * ci + 5                 # unaligned source offsets
    base = torch.zeros(off, dtype=torch.float32)
    for o, t in srcs:
        base[o:o + t.numel()] = t.reshape(-1)
    base = base.to(DEV)
    rows, doff, blocks, want = [], 0, 0, []
    for (o, t), (co, kh, kw, ci, mode) in zip(srcs, shapes):
        w = base[o:o + t.numel()].view(co, kh * kw * ci)
        src = w if mode == 0 else train_ops.conv2d_weight_flip(w, co, kh, kw, ci)
        ref = ops.pack_w_x3(src.contiguous())
        r, k = (co, kh * kw * ci) if mode == 0 else (ci, kh * kw * co)
        assert ref.shape == (r, (k + 31) // 32 * 64)
        rows.append([o, doff, co, kh, kw, ci, blocks, mode])
        want.append((doff, ref))
        doff += (ref.numel() + 127) // 128 * 128
        blocks += int(lib.cfp_pack_w_x3_blocks(r, k))
    dst = torch.full((doff,), float("nan"), dtype=torch.float16, device=DEV)
    desc = torch.tensor(rows, dtype=torch.int64).to(DEV)
    hip.call("cfp_pack_w_x3_batch", base.data_ptr(), dst.data_ptr(), desc.data_ptr(), len(rows), blocks, hip.current_stream())
    torch.cuda.synchronize()
    for d, ref in want:
        got = dst[d:d + ref.numel()].view(ref.shape)
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
