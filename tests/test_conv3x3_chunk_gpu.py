"""conv3x3_chunk.hip: the 16-bit 3x3 stride-1 convolution for more than 64 input channels (64-channel chunks of the halo through LDS).

Op level, every tile forced through cfp_debug_set(0, 600 + v):
  * bit-identical to the forced direct kernel (cfp_debug_set(0, 200 + v)) on the same operands -- the two share their K order;
  * bit-exact against a float64 host convolution on small-integer operands (every partial sum is an integer below 2^24);
  * against a forced implicit-GEMM tile within the bound of the whole-depth halo kernel's tests (float32 re-association only).
Shapes: the smallest at which each mechanism can go wrong -- ragged tiles in both directions, a tile seam, the seam between two images,
a channel tail inside the first / second 32-deep block of the last chunk, one to four chunks (both halo buffers and both weight stages
reused), a partial last channel tile, two channel blocks, slices of wider buffers on the input, the output and the residual.
Refusals: what the kernel does not take is an error when forced and never planned.  Engine: the B = 2 forward of test_forward_gpu.py with
the kernel wherever it can run and nowhere, both inside the existing bounds against the CPU oracle."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from cfpnet_amd import hip, ops  # noqa: E402

DEV = "cuda:0"
HALF = [torch.bfloat16, torch.float16]
TILES = [0, 1]                      # 128 channels x 8 x 16 pixels, 64 channels x 8 x 16 pixels
DIRECT_OF = {0: 0, 1: 1}                       # the direct kernel's tile of the same channel width (its result does not depend on the tile)
SENTINEL = 7.0

SHAPES = [(9, 20), (16, 16), (20, 35)]
CINS = [72, 128, 168, 192, 256]
COUTS = [32, 64, 128, 256, 136]
# every Cin x every Cout on the smallest shape, every shape on the corners of that grid
CASES = [(2, 9, 20, ci, co) for ci in CINS for co in COUTS] + [(2, h, w, ci, co) for (h, w) in SHAPES[1:] for (ci, co) in ((72, 136), (168, 64), (256, 256))]


def _rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def _nhwc(x):
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()


def _slice_of(x2d, dtype, pad_l, pad_r, fill=0.0):
    rows, C = x2d.shape
    buf = torch.full((rows, pad_l + C + pad_r), fill, dtype=dtype, device=DEV)
    buf[:, pad_l:pad_l + C] = x2d.to(dtype).to(DEV)
    return ops.Act(buf, pad_l, C)


@functools.lru_cache(maxsize=None)
def _operands(B, H, W, Cin, Cout, dtype):
    """x as a channel slice of a wider buffer (in_ld > Cin), weights, scale / shift, residual as a slice (res_ld > Cout)."""
    x = _rnd(B, Cin, H, W, seed=11)
    w = _rnd(Cout, Cin, 3, 3, seed=12, scale=1.0 / math.sqrt(9 * Cin))
    xa = _slice_of(_nhwc(x), dtype, 8, 16, fill=3.0)
    wa = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous().to(dtype).to(DEV)
    scale = (_rnd(Cout, seed=13).abs() + 0.5).to(DEV)
    shift = _rnd(Cout, seed=14).to(DEV)
    ra = _slice_of(_nhwc(_rnd(B, Cout, H, W, seed=15)), dtype, 16, 8, fill=5.0)
    return xa, wa, scale, shift, ra


def _run(lib, force, xa, wa, scale, shift, B, H, W, Cout, dtype, act, res):
    """One forced launch into a channel slice of a sentinel-filled buffer; the columns outside the slice must come back untouched."""
    lib.cfp_debug_set(0, force)
    buf = torch.full((B * H * W, 16 + Cout + 24), SENTINEL, dtype=dtype, device=DEV)
    out = ops.Act(buf, 16, Cout)
    ops.conv2d(xa, wa, scale, shift, out, B, H, W, 3, 3, 1, 1, 1, H, W, act, res, None)
    torch.cuda.synchronize()
    assert bool((buf[:, :16] == SENTINEL).all()) and bool((buf[:, 16 + Cout:] == SENTINEL).all()), "columns outside the output slice were written"
    return out.torch().contiguous()


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("tile", TILES)
def test_chunk_equals_direct_bit_for_bit_and_igemm_to_reassociation(tile, dtype):
    lib = hip.load()
    ulp = 2.0 ** (-7 if dtype == torch.bfloat16 else -10)
    try:
        for n, (B, H, W, Cin, Cout) in enumerate(CASES):
            xa, wa, scale, shift, ra = _operands(B, H, W, Cin, Cout, dtype)
            # the activations of the moved layers (none: the DAPM convolutions, LeakyReLU: the decoder's), with and without the residual
            act, res = [(hip.ACT_LRELU, None), (hip.ACT_NONE, ra), (hip.ACT_NONE, None), (hip.ACT_LRELU, ra)][n % 4]
            got = _run(lib, 600 + tile, xa, wa, scale, shift, B, H, W, Cout, dtype, act, res)
            ref = _run(lib, 200 + DIRECT_OF[tile], xa, wa, scale, shift, B, H, W, Cout, dtype, act, res)
            assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), f"chunk tile {tile} != direct kernel: {(B, H, W, Cin, Cout)} act {act}"
            gem = _run(lib, 4, xa, wa, scale, shift, B, H, W, Cout, dtype, act, res)
            a, b2 = got.float(), gem.float()
            assert float(((a - b2).abs() / b2.abs().clamp(min=1.0)).max()) <= 2 * ulp, f"chunk tile {tile} vs igemm2: {(B, H, W, Cin, Cout)}"
            assert float((a != b2).float().mean()) < 0.02
    finally:
        lib.cfp_debug_set(0, -1)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("tile", TILES)
def test_chunk_bit_exact_on_integers(tile, dtype):
    lib = hip.load()
    try:
        for (B, H, W, Cin, Cout) in [(2, 9, 20, 72, 32), (2, 16, 16, 168, 136), (2, 20, 35, 128, 64), (2, 9, 20, 256, 256), (2, 16, 16, 192, 128)]:
            g = torch.Generator().manual_seed(100 + Cin + Cout)
            x = torch.randint(-3, 4, (B, Cin, H, W), generator=g).float()
            w = torch.randint(-2, 3, (Cout, Cin, 3, 3), generator=g).float()
            ref = F.conv2d(x.double(), w.double(), None, 1, 1).float()      # |sum| <= 6 * 9 * 256 < 2^24: every partial sum is exact in float32
            xa = _slice_of(_nhwc(x), dtype, 8, 16, fill=3.0)
            wa = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous().to(dtype).to(DEV)
            got = _run(lib, 600 + tile, xa, wa, None, None, B, H, W, Cout, dtype, hip.ACT_NONE, None).float().cpu()
            got = got.reshape(B, H, W, Cout).permute(0, 3, 1, 2)
            # the stored value is the storage type's rounding of the exact integer sum
            assert torch.equal(got, ref.to(dtype).float()), f"chunk tile {tile} integers {(B, H, W, Cin, Cout)}"
    finally:
        lib.cfp_debug_set(0, -1)


def _sentinel_out(rows, Cout, dtype):
    buf = torch.full((rows, Cout), SENTINEL, dtype=dtype, device=DEV)
    return buf, ops.Act(buf, 0, Cout)


@pytest.mark.parametrize("tile", TILES)
def test_chunk_refuses_what_it_does_not_take(tile):
    """A forced tile is an error for stride 2, Cin <= 64, Cin % 8 != 0, a LayerNorm epilogue and per-image weights, and nothing is launched."""
    lib = hip.load()
    dtype = torch.bfloat16
    B, H, W = 2, 10, 12

    def x_w(Cin, Cout, per_image=False):
        x = ops.Act(torch.ones(B * H * W, Cin, dtype=dtype, device=DEV), 0, Cin)
        w = torch.ones((B, Cout, 9 * Cin) if per_image else (Cout, 9 * Cin), dtype=dtype, device=DEV)
        return x, w

    try:
        lib.cfp_debug_set(0, 600 + tile)
        # stride 2
        x, w = x_w(128, 64)
        buf, out = _sentinel_out(B * 5 * 6, 64, dtype)
        with pytest.raises(Exception):
            ops.conv2d(x, w, None, None, out, B, H, W, 3, 3, 2, 0, 0, 5, 6, hip.ACT_NONE, None, None)
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all())
        # Cin <= 64, Cin % 8 != 0
        for Cin in (64, 32, 68):
            x, w = x_w(Cin, 64)
            buf, out = _sentinel_out(B * H * W, 64, dtype)
            with pytest.raises(Exception):
                ops.conv2d(x, w, None, None, out, B, H, W, 3, 3, 1, 1, 1, H, W, hip.ACT_NONE, None, None)
            torch.cuda.synchronize()
            assert bool((buf == SENTINEL).all()), Cin
        # LayerNorm epilogue
        x, w = x_w(128, 64)
        buf, out = _sentinel_out(B * H * W, 64, dtype)
        ln = (torch.ones(64, device=DEV), torch.zeros(64, device=DEV), 1e-5)
        with pytest.raises(Exception):
            ops.conv2d(x, w, None, None, out, B, H, W, 3, 3, 1, 1, 1, H, W, hip.ACT_NONE, None, None, ln=ln)
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all())
        # per-image weights
        x, w = x_w(128, 64, per_image=True)
        buf, out = _sentinel_out(B * H * W, 64, dtype)
        with pytest.raises(Exception):
            ops.conv2d(x, w, None, None, out, B, H, W, 3, 3, 1, 1, 1, H, W, hip.ACT_NONE, None, None, per_image_weights=True)
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all())
        # a tile that does not exist
        lib.cfp_debug_set(0, 600 + len(TILES))
        x, w = x_w(128, 64)
        buf, out = _sentinel_out(B * H * W, 64, dtype)
        with pytest.raises(Exception):
            ops.conv2d(x, w, None, None, out, B, H, W, 3, 3, 1, 1, 1, H, W, hip.ACT_NONE, None, None)
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all())
    finally:
        lib.cfp_debug_set(0, -1)
    # ... and never planned
    for M in (9600, 38400, 153600):
        for fl in (1, 4):
            assert lib.cfp_conv3x3_chunk_variant(M, 64, 128, fl) == -1 and lib.cfp_conv3x3_chunk_variant(M, 32, 64, fl) == -1
            assert lib.cfp_conv3x3_chunk_variant(M, 68, 128, fl) == -1 and lib.cfp_conv3x3_chunk_variant(M, 132, 128, fl) == -1
        assert ops.conv2d_plan(M, 128, 9 * 256, hip.BF16, 0, 8, 3, 2)[0] < 600           # stride 2
        assert ops.conv2d_plan(M, 128, 9 * 256, hip.BF16, M // 8, 8, 3, 1)[0] < 600      # per-image weights
        assert ops.conv2d_plan(M, 128, 9 * 64, hip.BF16, 0, 8, 3, 1)[0] < 600            # Cin <= 64


@functools.lru_cache(maxsize=None)
def _b2_case():
    from cfpnet_amd import spec, synthetic, weights
    from oracle import cfpnet_oracle as O
    layers = spec.COMBINE1_LAYERS
    sd = weights.make_torch_state_dict(spec.model_manifest(layers))
    inp = synthetic.make_inputs(2, 480, 640, 8, 56, seed=21, drop_hist=0.2)      # the B = 2 case of test_forward_gpu.py
    _, p0, _ = O.forward(sd, inp, layer_names=layers)
    return layers, sd, inp, p0.numpy()


@pytest.mark.parametrize("dtype,bound", [(torch.bfloat16, 1e-2), (torch.float16, 1e-3)])      # TOL_BF16 / TOL_F16 of test_forward_gpu.py
def test_engine_forward_with_the_kernel_everywhere_and_nowhere(dtype, bound):
    """The B = 2 forward with every 3x3 convolution the kernel takes running through it (cfp_debug_set(40, 2)), as planned (1) and with none
    (cfp_debug_set(40, 0)): all inside the bound of test_full_model_16bit_error_is_bounded against the CPU oracle."""
    from cfpnet_amd.engine import Engine
    lib = hip.load()
    layers, sd, inp, p0 = _b2_case()
    rel = {}
    try:
        for mode in (2, 1, 0):
            lib.cfp_debug_set(40, mode)
            eng = Engine(sd, layer_names=layers, dtype=dtype)
            _, p1, _ = eng.forward(inp)
            torch.cuda.synchronize()
            p1 = p1.cpu().numpy()
            rel[mode] = float(np.abs(p1 - p0).sum() / np.abs(p0).sum())
            worst = max(float(np.abs(p1[b] - p0[b]).sum() / np.abs(p0[b]).sum()) for b in range(2))
            print(f"{dtype} B=2 forward, chunk kernel {('off', 'as planned', 'everywhere')[mode]}: pred relL1 vs CPU oracle {rel[mode]:.4e}, worst image {worst:.4e}")
            del eng
    finally:
        lib.cfp_debug_set(40, 1)
    assert rel[2] < bound and rel[1] < bound and rel[0] < bound, rel
