"""cfp_pw_rows (csrc/pw_rows.hip: short-K pointwise GEMM, input rows in registers, weights streamed once per workgroup) against
cfp_conv2d_nhwc on the same operands: bit-identical, for both 16-bit types and both activations, on slices of wider buffers."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cfpnet_amd import hip, ops  # noqa: E402

DEV = "cuda:0"
HALF = [torch.bfloat16, torch.float16]

# M, K, N, column groups (0 = the kernel's choice, -1 = the most the shape allows)
# M: one wave / one full tile / a ragged tile / several tiles.  K: one 8-element chunk, one 32 block, a tail inside the second block of a
# 64 step (56), inside the fourth (112), a third step that holds one chunk and a whole zero block (136), the last chunk missing (232),
# the register cap (256).  N: one fragment column, N % 16 != 0, seven chunks, and 25.5 chunks over 4 groups (7 + 7 + 7 + 5 chunks, the
# last one ragged).
CASES = [
    (16, 8, 16, 0),
    (64, 32, 24, 0),
    (69, 136, 816, 0),
    (69, 136, 816, 1),
    (69, 136, 816, 4),
    (69, 136, 816, -1),
    (200, 232, 24, 0),
    (200, 56, 224, 0),
    (200, 56, 224, 1),
    (200, 56, 224, -1),
    (64, 112, 224, 3),
    (69, 256, 816, 0),
    (16, 232, 16, 0),
    (200, 256, 224, 2),
]


def _operands(M, K, N, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    xin = torch.full((M, K + 24), float("nan"), dtype=dtype)      # the input is columns [8, 8 + K): a K tail that reads past it meets NaN
    xin[:, 8:8 + K] = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dtype)
    s = torch.rand(N, generator=g) + 0.5
    t = torch.randn(N, generator=g)
    return xin.to(DEV), w.to(DEV).contiguous(), s.to(DEV), t.to(DEV)


def _out(M, N, dtype):
    buf = torch.full((M + 3, N + 24), 7.0, dtype=dtype, device=DEV)      # the output is columns [16, 16 + N) of rows [0, M)
    return buf, ops.Act(buf, 16, N)


@pytest.mark.parametrize("act", [hip.ACT_NONE, hip.ACT_SILU])
@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("case", CASES)
def test_bit_identical_to_conv2d(case, dtype, act):
    M, K, N, groups = case
    auto, most = ops.pw_rows_groups(M, K, N)
    assert 1 <= auto <= most == (N + 31) // 32
    if groups < 0:
        groups = most
    xin, w, s, t = _operands(M, K, N, dtype, seed=M + K + N)
    x = ops.Act(xin, 8, K)
    assert ops.pw_rows_fits(M, K, N, x.ld, N + 24, ops.DT[dtype])
    wbuf, want = _out(M, N, dtype)
    ops.conv2d(x, w, s, t, want, 1, 1, M, 1, 1, 1, 0, 0, 1, M, act)
    gbuf, got = _out(M, N, dtype)
    ops.pw_rows(x, w, s, t, got, M, act, groups)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(wbuf.float()).all()) and bool(torch.isfinite(gbuf.float()).all()), case
    assert not bool((wbuf[:M, 16:16 + N] == 7.0).all())
    for b in (wbuf, gbuf):      # sentinels left, right and below survive
        assert bool((b[:, :16] == 7.0).all()) and bool((b[:, 16 + N:] == 7.0).all()) and bool((b[M:] == 7.0).all()), case
    assert torch.equal(gbuf.view(torch.int16), wbuf.view(torch.int16)), (case, dtype, act)


@pytest.mark.parametrize("tm", [1, 2])
@pytest.mark.parametrize("dtype", HALF)
def test_both_row_counts_per_wave(dtype, tm):
    """cfp_debug_set(41, 1 / 2) forces 16 or 32 rows per wave (64- or 128-row workgroups): the ragged cases, one group, the most groups and
    an uneven split."""
    lib = hip.load()
    try:
        lib.cfp_debug_set(41, tm)
        for M, K, N, groups in [(69, 136, 816, 0), (69, 136, 816, 1), (69, 136, 816, 4), (69, 136, 816, -1), (200, 232, 24, 0), (16, 8, 16, 0),
                                (200, 256, 224, 2), (64, 56, 224, -1), (130, 112, 224, 3)]:
            auto, most = ops.pw_rows_groups(M, K, N)
            assert most == (N + 31) // 32
            xin, w, s, t = _operands(M, K, N, dtype, seed=M + K + N + tm)
            x = ops.Act(xin, 8, K)
            wbuf, want = _out(M, N, dtype)
            ops.conv2d(x, w, s, t, want, 1, 1, M, 1, 1, 1, 0, 0, 1, M, hip.ACT_SILU)
            gbuf, got = _out(M, N, dtype)
            ops.pw_rows(x, w, s, t, got, M, hip.ACT_SILU, most if groups < 0 else groups)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(gbuf.float()).all()), (M, K, N, groups)
            assert torch.equal(gbuf.view(torch.int16), wbuf.view(torch.int16)), (M, K, N, groups, tm)
    finally:
        lib.cfp_debug_set(41, 0)


@pytest.mark.parametrize("dtype", HALF)
def test_without_scale_and_shift(dtype):
    M, K, N = 69, 136, 224
    xin, w, _, _ = _operands(M, K, N, dtype, seed=5)
    x = ops.Act(xin, 8, K)
    wbuf, want = _out(M, N, dtype)
    ops.conv2d(x, w, None, None, want, 1, 1, M, 1, 1, 1, 0, 0, 1, M, hip.ACT_SILU)
    gbuf, got = _out(M, N, dtype)
    ops.pw_rows(x, w, None, None, got, M, hip.ACT_SILU)
    torch.cuda.synchronize()
    assert torch.equal(gbuf.view(torch.int16), wbuf.view(torch.int16))


def test_a_shape_it_does_not_take_is_an_error():
    x = ops.new_act(64, 264, torch.bfloat16, DEV, zero=True)
    out = ops.new_act(64, 64, torch.bfloat16, DEV, zero=True)
    w = torch.zeros(64, 264, dtype=torch.bfloat16, device=DEV)
    assert not ops.pw_rows_fits(64, 264, 64, 264, 64, hip.BF16)
    with pytest.raises(RuntimeError):
        ops.pw_rows(x, w, None, None, out, 64)
