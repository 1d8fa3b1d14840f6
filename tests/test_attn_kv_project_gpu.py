"""cfp_attn_kv_project_reduce[_dev]: the k|v projection inside the key/value reduction.  Its kv, ksum and split slabs must be BIT-identical
to the launches it replaces -- ops.linear with the k|v weight followed by ops.attn_kv_reduce -- on the same operands (within
rounding is not accepted for a fused path)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cfpnet_amd import ops  # noqa: E402

DEV = "cuda:0"
HALF = [torch.bfloat16, torch.float16]
SENTINEL = -77.0


def _operands(rows, D, dtype, ld, c0, seed):
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((rows, ld), 3.0, dtype=dtype, device=DEV)      # the rest of the pitch is not the kernel's to read
    buf[:, c0:c0 + D] = torch.randn(rows, D, generator=g).to(dtype).to(DEV)
    w = (torch.randn(2 * D, D, generator=g) * D ** -0.5).to(dtype).to(DEV).contiguous()
    return ops.Act(buf, c0, D), w


def _state(groups, heads, d, nws):
    return (torch.full((groups * heads * d * d,), SENTINEL, device=DEV), torch.full((groups * heads * d,), SENTINEL, device=DEV),
            torch.full((max(nws, 1),), SENTINEL, device=DEV))


def _groups(NB, Hk, Wk, th, tw):
    return NB * -(-Hk // th) * -(-Wk // tw)


def _pair(x, w, NB, Hk, Wk, th, tw, clip, count_pad, v_length, heads, d, rec=None):
    """The launches the fused op replaces."""
    D = heads * d
    kvb = ops.Act(torch.zeros(x.rows, 2 * D, dtype=x.buf.dtype, device=DEV), 0, 2 * D)
    ops.linear(x, w, None, None, kvb, x.rows)
    nws = ops.attn_kv_ws_floats(NB, Hk, Wk, th, tw, heads, d)
    kv, ks, ws = _state(_groups(NB, Hk, Wk, th, tw), heads, d, nws)
    ops.attn_kv_reduce(kvb.slice(0, D), kvb.slice(D, D), kv, ks, ws, NB, Hk, Wk, th, tw, clip, count_pad, v_length, heads, d, rec=rec)
    return kv, ks, ws, nws


def _check(dtype, D, heads, NB, Hk, Wk, th, tw, clip, count_pad, v_length, ld=None, c0=0, seed=1):
    d = D // heads
    assert ops.attn_kv_project_fits(NB, Hk, Wk, th, tw, heads, d, dtype)
    x, w = _operands(NB * Hk * Wk, D, dtype, ld or D, c0, seed)
    want_kv, want_ks, want_ws, nws = _pair(x, w, NB, Hk, Wk, th, tw, clip, count_pad, v_length, heads, d)
    kv, ks, ws = _state(_groups(NB, Hk, Wk, th, tw), heads, d, nws)
    ops.attn_kv_project_reduce(x, w, kv, ks, ws, NB, Hk, Wk, th, tw, clip, count_pad, v_length, heads, d)
    torch.cuda.synchronize()
    what = (dtype, D, heads, NB, Hk, Wk, th, tw, clip)
    assert bool(torch.isfinite(kv).all()) and bool(torch.isfinite(ks).all()), what
    assert torch.equal(kv, want_kv), ("kv", what)
    assert torch.equal(ks, want_ks), ("ksum", what)
    assert torch.equal(ws, want_ws), ("split slabs", what)      # (all SENTINEL when the keys are not split)
    return nws


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("heads", [4, 8])
@pytest.mark.parametrize("D", [32, 64, 128])
def test_ragged_windows_with_padding_from_a_slice_of_a_wider_buffer(D, heads, dtype):
    """LSA: 6 x 6 windows on a 13 x 17 grid (ragged on both sides, zero-padded positions counted), tokens = columns [0, D) of [rows, 2D]."""
    _check(dtype, D, heads, 2, 13, 17, 6, 6, (0, 13, 0, 17), True, 36.0, ld=2 * D)


@pytest.mark.parametrize("dtype", HALF)
def test_clip_rectangle_cuts_groups_and_empties_one(dtype):
    # columns 7 .. 15 of rows 2 .. 10: the first column of windows (x < 6) has no key left (S = 0), the others are cut
    _check(dtype, 64, 8, 2, 13, 17, 6, 6, (2, 11, 7, 16), True, 36.0, ld=72, c0=8)
    _check(dtype, 128, 4, 2, 13, 17, 6, 6, (2, 11, 7, 16), False, 36.0)
    # one group per image, the rectangle inside it (DAPM's shape at a size that fits)
    _check(dtype, 32, 4, 2, 9, 11, 9, 11, (1, 8, 2, 10), False, 56.0)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("Wk", [200, 203])
def test_split_keys(Wk, dtype):
    """GSA: one group of 200 (203) keys in four splits of 50 (51, the last one 50): no multiple of 16; the slabs are compared too."""
    nws = _check(dtype, 32, 4, 1, 1, Wk, 1, Wk, (0, 1, 0, Wk), False, float(Wk))
    assert nws == 4 * 4 * (8 * 8 + 8)
    nws = _check(dtype, 128, 8, 2, 1, Wk, 1, Wk, (0, 1, 0, Wk), False, float(Wk))
    assert nws == 2 * 8 * 4 * (16 * 16 + 16)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("D", [32, 64, 128])
def test_sixteen_key_groups(D, dtype):
    """hist2image: a zone's 16 ToF samples."""
    _check(dtype, D, 4, 18, 1, 16, 1, 16, (0, 1, 0, 16), False, 16.0)


@pytest.mark.parametrize("dtype", HALF)
def test_two_records_through_one_captured_graph(dtype):
    D, heads, NB, Hk, Wk = 64, 4, 2, 9, 11
    d = D // heads
    x, w = _operands(NB * Hk * Wk, D, dtype, D + 8, 8, seed=5)
    rects = [(1, 8, 2, 10), (3, 5, 0, 11), (4, 4, 6, 6)]      # the last one is empty: n_inside = 0, v_length = 1

    def record(r):
        y0, y1, x0, x1 = r
        return torch.tensor([y0, x0, y1 - y0, x1 - x0, y0, y1, x0, x1, (y1 - y0) * (x1 - x0)], dtype=torch.int32, device=DEV)

    nws = ops.attn_kv_ws_floats(NB, Hk, Wk, Hk, Wk, heads, d)
    kv, ks, ws = _state(NB, heads, d, nws)
    rec = record(rects[0])
    ops.attn_kv_project_reduce(x, w, kv, ks, ws, NB, Hk, Wk, Hk, Wk, None, False, None, heads, d, rec=rec)      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.attn_kv_project_reduce(x, w, kv, ks, ws, NB, Hk, Wk, Hk, Wk, None, False, None, heads, d, rec=rec)
    for r in rects[1:] + rects[:1]:
        rec.copy_(record(r))
        kv.fill_(SENTINEL), ks.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        n_in = (r[1] - r[0]) * (r[3] - r[2])
        want_kv, want_ks, _, _ = _pair(x, w, NB, Hk, Wk, Hk, Wk, r, False, float(max(n_in, 1)), heads, d)      # the scalar pair
        dev_kv, dev_ks, _, _ = _pair(x, w, NB, Hk, Wk, Hk, Wk, None, False, None, heads, d, rec=record(r))      # the record-reading pair
        assert torch.equal(kv, want_kv) and torch.equal(ks, want_ks), (dtype, r)
        assert torch.equal(kv, dev_kv) and torch.equal(ks, dev_ks), (dtype, r)


@pytest.mark.parametrize("dtype", HALF)
def test_small_integer_operands_are_exact(dtype):
    """x in {0, 1, 2}, k weights in {0, 1}, v weights in {-1, 0, 1}: K >= 0 is an integer <= 64 (elu(K) + 1 = K + 1), V an integer, v_length 16
    a power of two -- every product and sum is exact in every format on the way, so the state equals the float64 one."""
    D, heads, NB, N = 32, 4, 5, 16
    d = D // heads
    g = torch.Generator().manual_seed(9)
    xi = torch.randint(0, 3, (NB * N, D), generator=g)
    wi = torch.cat([torch.randint(0, 2, (D, D), generator=g), torch.randint(-1, 2, (D, D), generator=g)], 0)
    x = ops.Act(xi.to(dtype).to(DEV).contiguous(), 0, D)
    w = wi.to(dtype).to(DEV).contiguous()
    kv, ks, ws = _state(NB, heads, d, 0)
    ops.attn_kv_project_reduce(x, w, kv, ks, ws, NB, 1, N, 1, N, (0, 1, 0, N), False, float(N), heads, d)
    torch.cuda.synchronize()
    kvp = (xi.double() @ wi.double().t()).reshape(NB, N, 2, heads, d)
    K1, V = kvp[:, :, 0] + 1, kvp[:, :, 1] / N
    want_kv = torch.einsum("nshd,nshv->nhdv", K1, V)
    assert torch.equal(kv.cpu().double().reshape(NB, heads, d, d), want_kv)
    assert torch.equal(ks.cpu().double().reshape(NB, heads, d), K1.sum(1))


def test_problems_that_do_not_fit_are_refused_before_any_launch():
    cases = [
        (torch.float32, 2, 13, 17, 6, 6, 4, 8),          # float32 storage
        (torch.bfloat16, 2, 13, 17, 6, 6, 4, 4),         # D = 16
        (torch.bfloat16, 2, 13, 17, 6, 6, 2, 16),        # two heads
        (torch.float16, 1, 100, 100, 100, 100, 4, 32),   # 64 splits of 157 keys at D = 128: 128 000 bytes of LDS
        (torch.bfloat16, 8, 120, 160, 120, 160, 4, 8),   # DAPM at the 1/4 scale of the benchmark: 300 keys per split
    ]
    for dtype, NB, Hk, Wk, th, tw, heads, d in cases:
        D = heads * d
        assert not ops.attn_kv_project_fits(NB, Hk, Wk, th, tw, heads, d, dtype)
        x = ops.Act(torch.zeros(NB * Hk * Wk, D, dtype=dtype, device=DEV), 0, D)
        w = torch.zeros(2 * D, D, dtype=dtype, device=DEV)
        nws = ops.attn_kv_ws_floats(NB, Hk, Wk, th, tw, heads, d)
        kv, ks, ws = _state(_groups(NB, Hk, Wk, th, tw), heads, d, nws)
        code = -1 if dtype == torch.float32 else -2      # CFP_EINVAL for the dtype, CFP_ESHAPE for a shape
        with pytest.raises(RuntimeError, match=r"cfp_attn_kv_project_reduce failed \(%d\)" % code):
            ops.attn_kv_project_reduce(x, w, kv, ks, ws, NB, Hk, Wk, th, tw, (0, Hk, 0, Wk), False, float(th * tw), heads, d)
        torch.cuda.synchronize()
        for t in (kv, ks, ws):
            assert bool((t == SENTINEL).all())
    # the model's own shapes at the benchmark size all fit: LSA windows, GSA, hist2image
    for NB, Hk, Wk, th, tw, heads, d in [(8, 120, 160, 12, 12, 8, 4), (8, 60, 80, 9, 9, 8, 8), (8, 30, 40, 6, 6, 8, 16),
                                         (8, 1, 140, 1, 140, 8, 4), (8, 1, 63, 1, 63, 8, 8), (8, 1, 35, 1, 35, 8, 16),
                                         (512, 1, 16, 1, 16, 4, 8), (512, 1, 16, 1, 16, 4, 16), (512, 1, 16, 1, 16, 4, 32)]:
        assert ops.attn_kv_project_fits(NB, Hk, Wk, th, tw, heads, d, torch.bfloat16)
