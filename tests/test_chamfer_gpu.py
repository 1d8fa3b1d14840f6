"""`cfp_bins_chamfer` on the GPU against float64 brute force (`chamfer_ref.py`) over the case table.

Loss:      |hip - f64| <= 2e-6 |f64| + |f32 brute force - f64|          (the form and constant of the SILog check of the training step)
Gradient:  max|g_hip - g64| <= MARGIN * max|g32 - g64| + 1e-6 max|g64|   with g32 the float32 brute force on the same case.
MARGIN = 2: the kernel sums in float64 / exact fixed point, so what it adds to the true gradient is the float32 rounding of each
output entry (2^-24 relative: under the floor) -- it has to be at least as good as float32 brute force; 2 leaves room for the different
summation order where both errors are of the size of the floor.  Measured ratios: DESIGN.md 4.23.
"""
import numpy as np
import pytest
import torch

import chamfer_ref as R

pytestmark = pytest.mark.gpu

from cfpnet_amd import hip, train_ops  # noqa: E402

DEV = "cuda:0"
MARGIN = 2.0
_REF = {}


def reference(name):
    """(edges, target, mask) on the device and the float64 / float32 brute force of the case, computed once per session."""
    if name not in _REF:
        wn, target, mask = R.make_case(name)
        edges, _ = train_ops.bin_centers(wn.to(DEV), R.MIN_VAL, R.MAX_VAL)             # what the model produces
        e = edges.cpu()
        assert np.array_equal(e.numpy(), R.edges_from_widths(wn.numpy()))
        a, b = R.tie_margins(e, target, mask)
        assert a > 1e-5 and b > 1e-5, (name, a, b)                                       # tie guard, on the reference
        _REF[name] = (edges, target.to(DEV), None if mask is None else mask.to(DEV),
                      R.chamfer_ref(e, target, mask, torch.float64), R.chamfer_ref(e, target, mask, torch.float32))
    return _REF[name]


@pytest.mark.parametrize("name", list(R.CASES))
def test_kernel_matches_float64_brute_force(name):
    edges, target, mask, (L64, Lb64, g64), (L32, Lb32, g32) = reference(name)
    crit = train_ops.BinsChamferLoss()
    L = crit.forward(edges, target, mask)
    g = crit.backward(1.0)
    torch.cuda.synchronize()
    L, Lb, g = float(L), crit.per_image.double().cpu(), g.double().cpu()
    L64f, L32f = float(L64), float(L32)
    e32, gmax = float((g32.double() - g64).abs().max()), float(g64.abs().max())
    eh = float((g - g64).abs().max())
    print(f"{name}: loss f64 {L64f:.9g} f32 {L32f:.9g} hip {L:.9g} | grad err hip {eh:.3e} f32 {e32:.3e} ratio {eh / max(e32, 1e-300):.3g} "
          f"floor {1e-6 * gmax:.3e}")
    assert abs(L - L64f) <= 2e-6 * abs(L64f) + abs(L32f - L64f)
    for b in range(len(Lb64)):
        assert abs(float(Lb[b]) - float(Lb64[b])) <= 2e-6 * abs(float(Lb64[b])) + abs(float(Lb32[b]) - float(Lb64[b]))
    assert eh <= MARGIN * e32 + 1e-6 * gmax
    if name == "empty_middle_image":                                 # the empty-image rule: exactly nothing, the denominator stays B
        assert float(Lb[1]) == 0.0 and not bool(g[1].any()) and bool(g[0].any()) and bool(g[2].any())


def test_grad_scale_and_null_gradient():
    edges, target, mask, (L64, _, g64), _ = reference("p80")
    crit = train_ops.BinsChamferLoss()
    L1 = crit.forward(edges, target, mask).clone()
    g1 = crit.backward(1.0).clone()
    L2 = crit.forward(edges, target, mask, grad_scale=0.5).clone()
    assert torch.equal(L1, L2) and torch.equal(crit.grad_centers, 0.5 * g1)            # a power of two: exact
    assert torch.allclose(crit.backward(1.0), g1, rtol=1e-6, atol=0)
    B, P = g1.shape
    ws = torch.empty(int(hip.load().cfp_bins_chamfer_ws_bytes(B, 37, 41, P)), dtype=torch.uint8, device=DEV)
    out = torch.empty(1 + B, dtype=torch.float32, device=DEV)
    hip.call("cfp_bins_chamfer", edges.data_ptr(), target.data_ptr(), mask.to(torch.uint8).data_ptr(), B, 37, 41, P, 1.0, ws.data_ptr(), ws.numel(),
             out.data_ptr(), 0, hip.current_stream())                                    # grad_centers NULL: the value alone
    assert torch.equal(out[0], L1)


def test_too_many_bins_is_refused():
    e = torch.linspace(0.0, 10.0, 1027, device=DEV)[None].contiguous()
    with pytest.raises(RuntimeError, match=r"cfp_bins_chamfer failed \(-2\)"):
        train_ops.BinsChamferLoss().forward(e, torch.ones(1, 1, 4, 4, device=DEV))


@pytest.mark.parametrize("name", ["p256", "one_416x544_image"])
def test_two_calls_are_bit_identical(name):
    edges, target, mask, _, _ = reference(name)
    a, b = train_ops.BinsChamferLoss(), train_ops.BinsChamferLoss()
    La, Lb = a.forward(edges, target, mask), b.forward(edges, target, mask)
    assert torch.equal(La, Lb) and torch.equal(a.grad_centers, b.grad_centers) and torch.equal(a.per_image, b.per_image)


def test_graph_replay_with_new_targets_equals_the_eager_call():
    edges, target, mask, _, _ = reference("one_416x544_image")
    t_static, crit = target.clone(), train_ops.BinsChamferLoss()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        crit.forward(edges, t_static, mask)                          # warm-up: allocates the workspace outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        L = crit.forward(edges, t_static, mask)
        grad = crit.grad_centers
    t2 = torch.where(target > 1e-3, 10.3 - target, target)           # other contents, same valid set
    t_static.copy_(t2)
    g.replay()
    torch.cuda.synchronize()
    eager = train_ops.BinsChamferLoss()
    L2 = eager.forward(edges, t2, mask)
    assert torch.equal(L, L2) and torch.equal(grad, eager.grad_centers)
    L1 = train_ops.BinsChamferLoss().forward(edges, target, mask)
    assert not torch.equal(L1, L2)                                   # the replay did read the new targets


def test_torch_loss_wrapper_is_differentiable_in_the_edges():
    edges, target, mask, (L64, _, g64), _ = reference("p80")
    e = edges.clone().requires_grad_(True)
    loss = 0.25 * train_ops.bins_chamfer(e, target, mask)
    loss.backward()
    assert abs(float(loss.detach()) - 0.25 * float(L64)) <= 1e-5 * float(L64)
    want = 0.25 * train_ops.centers_grad_to_edges(g64)               # g_e[k] = 0.5 (g_c[k-1] + g_c[k])
    assert float((e.grad.double().cpu() - want).abs().max()) <= 1e-5 * float(want.abs().max())
