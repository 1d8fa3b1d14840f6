"""Dynamic-zone-geometry kernels (csrc/zone_window.hip, cfp_linattn_*_dev) against torch: F.pad + slicing +
F.interpolate(align_corners=True) for the forward, torch autograd of the same expression for the backward; the zone
rectangle is read from a device record (geometry.zone_record layout)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cfpnet_amd import train_ops

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["f32", "f16", "bf16"]
B, H, W, C, ZN, P1, P2 = 2, 20, 24, 32, 3, 4, 4          # grid 12 x 12
PAD = 16


def _rec(sy, sx, tzh, tzw):
    c = lambda v, hi: max(0, min(v, hi))
    y0, y1, x0, x1 = c(sy, H), c(sy + tzh, H), c(sx, W), c(sx + tzw, W)
    return torch.tensor([sy, sx, tzh, tzw, y0, y1, x0, x1, (y1 - y0) * (x1 - x0)], dtype=torch.int32, device="cuda")


# (sy, sx, tzh, tzw): shifted grid without resampling, widened union (resamples), rectangle overhanging the map (zero-extended part),
# a narrower rectangle (upsampling: the negative-offset truncation of index_wo_pad)
GEOMS = {"shifted": (3, 5, 12, 12), "widened": (2, 4, 15, 17), "overhang": (-3, -2, 14, 13), "overhang_far": (10, 14, 13, 12),
         "narrow": (4, 6, 11, 10)}


def _tol(dtype):
    return {torch.float32: 2e-6, torch.float16: 2e-3, torch.bfloat16: 1.6e-2}[dtype]


def _map(rows):          # [B*H*W, C] -> [B, C, H, W] float32
    return rows.float().view(B, H, W, C).permute(0, 3, 1, 2)


def _crop_ref(tok_map, sy, sx, tzh, tzw):
    z = F.pad(tok_map, (PAD, PAD, PAD, PAD))[:, :, sy + PAD:sy + PAD + tzh, sx + PAD:sx + PAD + tzw]
    if (tzh, tzw) != (ZN * P1, ZN * P2):
        z = F.interpolate(z, size=[ZN * P1, ZN * P2], mode="bilinear", align_corners=True)
    return z.reshape(B, C, ZN, P1, ZN, P2).permute(0, 2, 4, 3, 5, 1).reshape(-1, C)


def _paste_ref(tok_map, z_rows, sy, sx, tzh, tzw):
    g = z_rows.view(B, ZN, ZN, P1, P2, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, ZN * P1, ZN * P2)
    if (tzh, tzw) != (ZN * P1, ZN * P2):
        g = F.interpolate(g, size=[tzh, tzw], mode="bilinear", align_corners=True)
    big = F.pad(g, (sx + PAD, W + PAD - sx - tzw, sy + PAD, H + PAD - sy - tzh))
    out = tok_map + big[:, :, PAD:PAD + H, PAD:PAD + W]
    return out.permute(0, 2, 3, 1).reshape(-1, C)


def _close(a, b, dtype):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    err = float((a - b).abs().max())
    assert err <= _tol(dtype) * max(float(b.abs().max()), 1e-6), err


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("geom", list(GEOMS), ids=list(GEOMS))
def test_zone_crop_forward_and_backward(dtype, geom):
    sy, sx, tzh, tzw = GEOMS[geom]
    torch.manual_seed(1)
    tok = torch.randn(B * H * W, C, device="cuda").to(dtype)
    rec = _rec(sy, sx, tzh, tzw)
    out = train_ops.zone_crop(tok, rec, B, H, W, ZN, P1, P2)
    x = _map(tok).detach().requires_grad_(True)
    ref = _crop_ref(x, sy, sx, tzh, tzw)
    _close(out, ref, dtype)
    dz = torch.randn_like(ref).to(dtype)
    ref.backward(dz.float())
    dtok = train_ops.zone_crop_bwd(dz, rec, B, H, W, ZN, P1, P2)
    _close(dtok, x.grad.permute(0, 2, 3, 1).reshape(-1, C), dtype)
    dtok2 = train_ops.zone_crop_bwd(dz, rec, B, H, W, ZN, P1, P2)
    assert torch.equal(dtok, dtok2)                                   # gather form: deterministic


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_zone_crop_without_resampling_is_the_gather_path_bit_for_bit(dtype):
    """Extent == grid: the weights are 1 / 0, the output equals the cfp_index_rows crop + regroup of the static path."""
    for sy, sx in ((3, 5), (-2, -4), (9, 13)):
        torch.manual_seed(2)
        tok = torch.randn(B * H * W, C, device="cuda").to(dtype)
        rec = _rec(sy, sx, ZN * P1, ZN * P2)
        b, zy, zx, i, j = np.meshgrid(np.arange(B), np.arange(ZN), np.arange(ZN), np.arange(P1), np.arange(P2), indexing="ij")
        y, x = sy + zy * P1 + i, sx + zx * P2 + j
        idx = np.where((y >= 0) & (y < H) & (x >= 0) & (x < W), (b * H + y) * W + x, -1).reshape(-1)
        ref = train_ops.index_rows(tok, torch.as_tensor(idx, dtype=torch.int32, device="cuda"))
        out = train_ops.zone_crop(tok, rec, B, H, W, ZN, P1, P2)
        assert torch.equal(out.view(torch.int16 if dtype != torch.float32 else torch.int32),
                           ref.view(torch.int16 if dtype != torch.float32 else torch.int32)), (sy, sx)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("geom", list(GEOMS), ids=list(GEOMS))
def test_zone_paste_forward_and_backward(dtype, geom):
    sy, sx, tzh, tzw = GEOMS[geom]
    torch.manual_seed(3)
    tok = torch.randn(B * H * W, C, device="cuda").to(dtype)
    z = torch.randn(B * ZN * ZN * P1 * P2, C, device="cuda").to(dtype)
    rec = _rec(sy, sx, tzh, tzw)
    out = train_ops.zone_paste(tok, z, rec, B, H, W, ZN, P1, P2)
    zr = z.float().detach().requires_grad_(True)
    ref = _paste_ref(_map(tok), zr, sy, sx, tzh, tzw)
    _close(out, ref, dtype)
    dy = torch.randn_like(ref).to(dtype)
    ref.backward(dy.float())
    dz = train_ops.zone_paste_bwd(dy, rec, B, H, W, ZN, P1, P2)
    _close(dz, zr.grad, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_no_skip_inside_and_rect_rows(dtype):
    """no_skip_inside (fusion.py:156): the rectangle is replaced -- mask the inside rows, then paste; the inside gather of DAPM
    into a capacity-sized buffer (rows >= n_inside zero) and its adjoint."""
    sy, sx, tzh, tzw = GEOMS["overhang"]
    torch.manual_seed(4)
    tok = torch.randn(B * H * W, C, device="cuda").to(dtype)
    z = torch.randn(B * ZN * ZN * P1 * P2, C, device="cuda").to(dtype)
    rec = _rec(sy, sx, tzh, tzw)
    y0, y1, x0, x1, n = (int(v) for v in rec[4:].tolist())
    m = _map(tok).clone()
    m[:, :, y0:y1, x0:x1] = 0
    masked = train_ops.zone_rect_rows(tok, rec, B, H, W, train_ops.ZONE_MASK)
    assert torch.equal(masked.float().cpu(), m.permute(0, 2, 3, 1).reshape(-1, C).cpu())
    out = train_ops.zone_paste(masked, z, rec, B, H, W, ZN, P1, P2)
    _close(out, _paste_ref(m, z.float(), sy, sx, tzh, tzw), dtype)
    cap = n + 37
    ins = train_ops.zone_rect_rows(tok, rec, B, H, W, train_ops.ZONE_INSIDE, cap).view(B, cap, C)
    ref = _map(tok)[:, :, y0:y1, x0:x1].permute(0, 2, 3, 1).reshape(B, n, C)
    assert torch.equal(ins[:, :n].float().cpu(), ref.cpu()) and not bool(ins[:, n:].float().abs().any())
    g = torch.randn(B * cap, C, device="cuda").to(dtype)
    back = _map(train_ops.zone_rect_rows(g, rec, B, H, W, train_ops.ZONE_INSIDE_BWD, cap))
    exp = torch.zeros(B, C, H, W)
    exp[:, :, y0:y1, x0:x1] = g.float().view(B, cap, C)[:, :n].cpu().reshape(B, y1 - y0, x1 - x0, C).permute(0, 3, 1, 2)
    assert torch.equal(back.cpu(), exp)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("L,n,cap", [(480, 150, 230), (64, 20, 40)], ids=["split", "wave"])
def test_dapm_attention_with_device_key_count(dtype, L, n, cap):
    """Keys / values in a capacity-sized buffer whose rows from n on are padding: the device key count leaves them out of KV and
    Ksum (elu(0)+1 = 1, so a zero row would count) and out of the v/S .. *S pair; their dk / dv are zero."""
    heads, d = 4, 8
    torch.manual_seed(5)
    q = (0.5 * torch.randn(B * L, heads * d, device="cuda")).to(dtype)
    kk = (0.5 * torch.randn(B * n, heads * d, device="cuda")).to(dtype)
    vv = torch.randn(B * n, heads * d, device="cuda").to(dtype)
    kp = torch.zeros(B, cap, heads * d, device="cuda", dtype=dtype)
    vp = torch.full((B, cap, heads * d), 7.0, device="cuda", dtype=dtype)      # padding must not leak, whatever it holds
    kp[:, :n], vp[:, :n] = kk.view(B, n, -1), vv.view(B, n, -1)
    kp, vp = kp.reshape(B * cap, -1), vp.reshape(B * cap, -1)
    s_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
    out_ref, st_ref = train_ops.linattn_fwd(q, kk, vv, B, L, n, heads, d)
    out, st = train_ops.linattn_fwd(q, kp, vp, B, L, cap, heads, d, s_dev=s_dev)
    _close(out, out_ref, dtype)
    dout = torch.randn_like(out)
    dq_r, dk_r, dv_r = train_ops.linattn_bwd(q, kk, vv, dout, st_ref, B, L, n, heads, d)
    dq, dk, dv = train_ops.linattn_bwd(q, kp, vp, dout, st, B, L, cap, heads, d, s_dev=s_dev)
    _close(dq, dq_r, dtype)
    _close(dk.view(B, cap, -1)[:, :n], dk_r.view(B, n, -1), dtype)
    _close(dv.view(B, cap, -1)[:, :n], dv_r.view(B, n, -1), dtype)
    assert not bool(dk.view(B, cap, -1)[:, n:].float().abs().any()) and not bool(dv.view(B, cap, -1)[:, n:].float().abs().any())
