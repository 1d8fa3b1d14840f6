"""`train_ops.SILogLoss` (csrc/loss.hip) forward and backward at every relation between the prediction and the target size, and at the
masks that leave 0, 1, 2 or no pixels of one image -- against `oracle.cfpnet_oracle.silog_loss` under float64 autograd on the CPU.

The backward pass is a gather whose window of target rows comes from float32 ceil / floor of (y -+ 1) / scale: a window one row too
narrow shows as a wrong gradient on a few prediction rows only, which the whole-step tests (0.15 relative per parameter) cannot see.

Bounds (the constants and forms of test_training_step_matches_autograd_of_the_oracle and
test_silog_loss_matches_reference_golden_and_autograd), with the float32 autograd of the same oracle call as the yardstick:
    loss       |hip - f64| <= 2e-6 |f64| + |f32 - f64|
    gradient   max|g_hip - g64| <= 2e-5 max|g64| + max|g32 - g64|        for backward(1.0) and backward(0.5)
Every test prints its worst error as a share of its bound (`pytest -s`)."""
import functools
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cfpnet_amd import train_ops  # noqa: E402
from oracle import cfpnet_oracle as O  # noqa: E402

DEV = "cuda:0"
B = 2
BIG = ((13, 17), (52, 68))          # 4x, not 2x: scale 12 / 51


@functools.lru_cache(maxsize=None)
def _inputs(hp, wp, ht, wt):
    """pred [B,1,hp,wp] in [0.3, 9], target [B,1,ht,wt] in [0.5, 9]; shared and never modified."""
    rng = np.random.default_rng(1000 * hp + 10 * ht + wt)
    pred = torch.from_numpy(rng.uniform(0.3, 9.0, (B, 1, hp, wp)).astype(np.float32))
    target = torch.from_numpy(rng.uniform(0.5, 9.0, (B, 1, ht, wt)).astype(np.float32))
    return pred, target


def _oracle(pred, target, mask, dt):
    p = pred.detach().to(dt).clone().requires_grad_(True)          # a copy: the shared inputs stay as they are
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # torch.var of fewer than two elements warns and returns NaN: the case wanted
        loss = O.silog_loss(p, target.to(dt), mask=mask, interpolate=True)
        loss.backward()
    return loss.detach().double(), p.grad.double()


def _hip(pred, target, mask, crit=None):
    crit = crit or train_ops.SILogLoss()
    loss = crit(pred.to(DEV), target.to(DEV), mask=None if mask is None else mask.to(DEV), interpolate=True)
    g1, gh = crit.backward(1.0), crit.backward(0.5)
    torch.cuda.synchronize()
    return loss.cpu(), g1.cpu(), gh.cpu(), crit


def _check(pred, target, mask, what):
    l64, g64 = _oracle(pred, target, mask, torch.float64)
    l32, g32 = _oracle(pred, target, mask, torch.float32)
    loss, g1, gh, crit = _hip(pred, target, mask)
    n = target.numel() if mask is None else int(mask.sum())
    assert float(crit._stats[2]) == n, what
    lerr, lbound = abs(float(loss) - float(l64)), 2e-6 * abs(float(l64)) + abs(float(l32 - l64))
    print(f"  silog {what}: n {n} loss {float(loss):.6f} err {lerr:.3e} = {lerr / lbound:.3f} of the bound (f32 autograd: {abs(float(l32 - l64)):.3e})")
    assert lerr <= lbound, (what, float(loss), float(l64))
    for s, g in ((1.0, g1), (0.5, gh)):
        gerr = float((g.double() - s * g64).abs().max())
        gbound = 2e-5 * float((s * g64).abs().max()) + float((s * (g32 - g64)).abs().max())
        print(f"    backward({s}): max|g64| {float((s * g64).abs().max()):.3e} err {gerr:.3e} = {gerr / gbound:.3f} of the bound")
        assert gerr <= gbound, (what, s, gerr, gbound)
    return g1


@pytest.mark.parametrize("hp,wp,ht,wt", [(13, 17, 52, 68), (9, 11, 9, 11), (12, 16, 7, 9), (1, 1, 5, 6), (1, 5, 4, 13), (2, 2, 31, 37), (6, 5, 1, 1)],
                         ids=["up_4x", "same_size", "down", "one_pixel_pred", "one_row_pred", "two_pixels_stretched", "one_pixel_target"])
def test_silog_at_every_size_relation(hp, wp, ht, wt):
    """interpolate=True, no mask.  Catches: the backward window's +-1 margin dropped or its ceil / floor swapped (up_4x: scale 12/51,
    where (y - 1) / scale is an integer at every fourth row; down: scale 11/6 > 1, where the window is one or two rows), the `scale == 0`
    branch gathering one row instead of all (one_pixel_pred, one_row_pred) or all instead of one (one_pixel_target: exactly two valid
    pixels, the smallest n with a finite loss), the tap clamp at the last row (same_size, where both taps of the last row coincide), and
    forward and backward computing the scale from different sizes."""
    pred, target = _inputs(hp, wp, ht, wt)
    _check(pred, target, None, f"{hp}x{wp}->{ht}x{wt}")


def _mask(kind):
    ht, wt = BIG[1]
    if kind == "none":
        return None
    m = torch.zeros(B, 1, ht, wt, dtype=torch.bool)
    if kind == "30_percent_invalid":
        m = torch.rand(B, 1, ht, wt, generator=torch.Generator().manual_seed(7)) > 0.3
    elif kind == "image_1_masked_out":
        m[0] = torch.rand(1, ht, wt, generator=torch.Generator().manual_seed(8)) > 0.3
    elif kind == "two_valid_pixels":
        m[0, 0, 10, 20] = m[1, 0, 40, 3] = True
    elif kind == "one_valid_pixel":
        m[1, 0, 51, 67] = True
    else:
        assert kind == "no_valid_pixel"
    return m


@pytest.mark.parametrize("kind", ["30_percent_invalid", "none", "image_1_masked_out", "two_valid_pixels"])
def test_silog_masks(kind):
    """13x17 -> 52x68.  Catches: the mask indexed per image instead of per batch element (image_1_masked_out: image 1 must receive an
    exactly zero gradient, and image 0's must not change), masked pixels counted in n or in the sums, `n - 1` replaced by `n` (visible at
    n = 2, where the two differ by a factor of two), and a `mask == None` path that reads a null pointer's flags."""
    pred, target = _inputs(*BIG[0], *BIG[1])
    g = _check(pred, target, _mask(kind), kind)
    if kind == "image_1_masked_out":
        assert float(g[1].abs().max()) == 0.0 and float(g[0].abs().max()) > 0.0
    if kind == "two_valid_pixels":
        assert int((g != 0).sum()) <= 8          # two target pixels, four taps each


@pytest.mark.parametrize("kind", ["one_valid_pixel", "no_valid_pixel"])
def test_silog_without_a_variance_is_nan_like_the_reference(kind):
    """n = 1 and n = 0: the reference's unbiased variance is NaN, and so must the kernel's loss be (a guard such as max(n - 1, 1) would
    report a finite loss for a batch without depth); the count is exact and both launches return."""
    pred, target = _inputs(*BIG[0], *BIG[1])
    mask = _mask(kind)
    l64, _ = _oracle(pred, target, mask, torch.float64)
    loss, g1, _, crit = _hip(pred, target, mask)
    print(f"  silog {kind}: reference {float(l64)} kernel {float(loss)} n {float(crit._stats[2])}")
    assert bool(torch.isnan(l64)) and bool(torch.isnan(loss))
    assert float(crit._stats[2]) == int(mask.sum())
    assert g1.shape == pred.shape


def test_silog_masked_pixels_contribute_exactly_nothing():
    """The target under a masked pixel set to 0 (log -> -inf) or to 1e30 leaves loss and gradient bit-identical.  Catches: `g * mask`
    instead of a skip (-inf * 0 = NaN), and a backward pass that weighs every pixel of the window and relies on g == 0 under the mask."""
    pred, target = _inputs(*BIG[0], *BIG[1])
    mask = _mask("30_percent_invalid")
    base = _hip(pred, target, mask)
    assert bool(torch.isfinite(base[0])) and bool(torch.isfinite(base[1]).all())
    for v in (0.0, 1e30):
        t = torch.where(mask, target, torch.full_like(target, v))
        got = _hip(pred, t, mask)
        assert got[0].view(torch.int32) == base[0].view(torch.int32), v
        assert torch.equal(got[1], base[1]) and torch.equal(got[2], base[2]), v


def test_silog_workspace_reuse_from_a_larger_to_a_smaller_shape():
    """One SILogLoss object runs 13x17 -> 52x68, then 12x16 -> 7x9 in the workspace the first run sized: bit-identical to a fresh
    object.  Catches: the partial sums placed by the workspace's size instead of the current n, the backward pass using the first
    run's shape, and block partials of the larger run left in the sum."""
    crit = train_ops.SILogLoss()
    big = _hip(*_inputs(*BIG[0], *BIG[1]), _mask("30_percent_invalid"), crit=crit)
    ws_ptr = crit._ws.data_ptr()
    pred, target = _inputs(12, 16, 7, 9)
    mask = torch.rand(B, 1, 7, 9, generator=torch.Generator().manual_seed(9)) > 0.3
    again = _hip(pred, target, mask, crit=crit)
    fresh = _hip(pred, target, mask)
    assert crit._ws.data_ptr() == ws_ptr, "the second run was meant to reuse the workspace"
    assert bool(torch.isfinite(big[0])) and bool(torch.isfinite(fresh[0]))
    assert again[0].view(torch.int32) == fresh[0].view(torch.int32)
    assert torch.equal(again[1], fresh[1]) and torch.equal(again[2], fresh[2])
