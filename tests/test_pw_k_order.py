"""Host helpers for the weight operands of the fused kernels: the K-axis fragment order of cfp_depth_head_fused and the padded 1x1 operand of
cfp_conv3x3_pw_fused (pure torch)."""
import pytest
import torch

from cfpnet_amd import ops


@pytest.mark.parametrize("K", [64, 160, 224])
def test_pw_k_order_is_a_bijection_in_the_documented_order(K):
    src = ops.pw_k_order(K)
    assert src.shape == (K,) and sorted(src.tolist()) == list(range(K))
    for pos in range(K):
        kb, q, e = pos // 32, (pos % 32) // 8, pos % 8
        assert int(src[pos]) == 32 * kb + 16 * (e >> 2) + 4 * q + (e & 3)
    # a lane's eight K-values (fq = q) are the four channels 4 q .. 4 q + 3 of two adjacent 16-channel tiles: the packed accumulators
    blk = src.reshape(K // 32, 4, 8)
    assert torch.equal(blk[:, :, 4:], blk[:, :, :4] + 16) and torch.equal(blk[:, :, 1:4], blk[:, :, :1] + torch.arange(1, 4))


def test_the_head_operand_uses_that_order():
    w128 = torch.randn(256, 128)
    assert torch.equal(ops.permute_wout(w128, torch.float32, hilo=False)[0], w128[:, ops.pw_k_order(128)])


@pytest.mark.parametrize("K,Co", [(64, 32), (160, 40), (224, 56), (48, 24), (144, 48)])
def test_pad_pw_w_pads_with_zeros_and_keeps_every_weight_in_place(K, Co):
    """The 1x1 operand of cfp_conv3x3_pw_fused: rows to a multiple of 16, K to a multiple of 32, K axis in its own order (the kernel walks
    the K blocks in the order of the 1x1 launch it replaces)."""
    w = torch.arange(1, Co * K + 1, dtype=torch.float32).reshape(Co, K)
    wp = ops.pad_pw_w(w)
    assert wp.shape == ((Co + 15) // 16 * 16, (K + 31) // 32 * 32) and wp.is_contiguous()
    assert torch.equal(wp[:Co, :K], w) and float(wp[Co:].abs().sum()) == 0.0 and float(wp[:, K:].abs().sum()) == 0.0
    assert wp.numel() * 2 % 1024 == 0      # whole KB: the kernel's 1 KB LDS-DMA pieces
