"""Per-pixel uncertainty planes of the bin heads (std of the bin distribution, entropy, largest bin probability) on the GPU.

Truth is float64 in the test, from the definitions in include/cfpnet_hip.h: in the operator tests from the same x, w, bias and centres the
kernel gets, end to end from the CPU oracle's `prob` and bin edges.  Every pixel counts.

THE ACCURACY RULE.  The promise is "at least as good as what a caller can do today with the `prob` we return".  Per statistic and case, as
maxima over all pixels: err_new = error of the kernel's plane, err_post = error of the same statistic evaluated in float64 from the `prob`
returned by the same call without `stats`.  Required: err_new <= 1.5 * err_post + floor.  The floors are what float32 arithmetic over 256
terms costs when err_post is (near) zero: 2e-5 nats (entropy), 2e-6 * (max_val - min_val) metres (std), 2e-5 relative (pmax) -- a float32
CPU emulation of the formulas gives 8e-7 nats, 7e-7 m at a 10 m range and 4e-7 relative; the factor of ~25 on top is room for `__expf`.
"""
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from cfpnet_amd import hip, ops, spec, synthetic, weights  # noqa: E402
from cfpnet_amd.engine import Engine  # noqa: E402
from oracle import cfpnet_oracle as O  # noqa: E402

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
HALF = [torch.bfloat16, torch.float16]
FLOOR_ENT, FLOOR_STD_PER_M, FLOOR_PMAX = 2e-5, 2e-6, 2e-5
NAMES = ("std", "entropy", "pmax")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def q(x, dtype):
    return x.to(dtype).float()


def to_act(x2d, dtype, ld=None):
    rows, C = x2d.shape
    ld = ld or C
    buf = torch.zeros(rows, ld, dtype=dtype, device=DEV)
    buf[:, :C] = x2d.to(dtype).to(DEV)
    return ops.Act(buf, 0, C)


def make_centers(B, nb):
    return torch.sort(torch.rand(B, nb, generator=torch.Generator().manual_seed(2)) * 10, dim=1)[0]


def truth_from_logits(logits, centers):
    """logits [B, HW, nb], centers [B, nb] (any float type) -> float64 [B, 3, HW] by the definitions."""
    l = logits.double()
    c = centers.double()[:, None, :]
    logp = torch.log_softmax(l, dim=2)
    p = logp.exp()
    mu = (p * c).sum(2, keepdim=True)
    std = (p * (c - mu) ** 2).sum(2).sqrt()
    ent = -(p * logp).sum(2)
    return torch.stack([std, ent, p.max(2)[0]], 1)


def stats_from_prob(prob, centers):
    """What a caller can do with a returned prob [B, nb, HW]: the three statistics in float64 -> [B, 3, HW]."""
    p = prob.double().cpu()
    c = centers.double().cpu()[:, :, None]
    mu = (p * c).sum(1, keepdim=True)
    std = (p * (c - mu) ** 2).sum(1).clamp(min=0).sqrt()
    ent = -torch.xlogy(p, p).sum(1)
    return torch.stack([std, ent, p.max(1)[0]], 1)


def errors(got, truth):
    """max over all pixels: absolute for std and entropy, relative for pmax."""
    d = (got.double().cpu() - truth).abs()
    return (float(d[:, 0].max()), float(d[:, 1].max()), float((d[:, 2] / truth[:, 2]).max()))


def check_rule(what, unc, prob, centers, truth, span):
    """(b) the accuracy rule and (c) the range of every value.  `prob` = the tensor of the same call without stats."""
    nb = centers.shape[1]
    u = unc.double().cpu().reshape(truth.shape)
    assert bool(torch.isfinite(u).all()), what
    floors = (FLOOR_STD_PER_M * span, FLOOR_ENT, FLOOR_PMAX)
    assert float(u[:, 0].min()) >= 0 and float(u[:, 1].min()) >= 0 and float(u[:, 2].max()) <= 1, what
    assert float(u[:, 1].max()) <= math.log(nb) + FLOOR_ENT and float(u[:, 2].min()) >= (1.0 / nb) * (1 - FLOOR_PMAX), what
    new = errors(u, truth)
    post = errors(stats_from_prob(prob.reshape(prob.shape[0], nb, -1), centers), truth)
    print(f"  {what}: " + "  ".join(f"{n} new {a:.2e} post {b:.2e}" for n, a, b in zip(NAMES, new, post)))
    for n, a, b, f in zip(NAMES, new, post, floors):
        assert a <= 1.5 * b + f, f"{what}: {n} err_new {a:.3e} > 1.5 * err_post {b:.3e} + floor {f:.1e}"
    return new, post


def run_three_ways(call, B, nb, HW, prob_dtype):
    """(a): `call(prob, pred, stats)` without stats, with stats, with stats and prob = NULL.  pred / prob must not notice the statistics
    and the statistics must not notice prob.  -> (prob of the call without stats, pred, stats)."""
    prob0 = torch.zeros(B, nb, HW, dtype=prob_dtype, device=DEV)
    pred0 = torch.empty(B, HW, device=DEV)
    call(prob0, pred0, None)
    prob1 = torch.zeros(B, nb, HW, dtype=prob_dtype, device=DEV)
    pred1 = torch.empty(B, HW, device=DEV)
    st1 = torch.full((B, 3, HW), float("nan"), device=DEV)
    call(prob1, pred1, st1)
    pred2 = torch.empty(B, HW, device=DEV)
    st2 = torch.full((B, 3, HW), float("nan"), device=DEV)
    call(None, pred2, st2)
    torch.cuda.synchronize()
    assert torch.equal(pred0, pred1) and torch.equal(prob0, prob1) and torch.equal(pred0, pred2)
    assert torch.equal(st1, st2)
    return prob0, pred0, st1


# ---- 4. operator level ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [64, 128, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_bin_softmax_stats(dtype, nb):
    """bin_softmax_kernel: ragged last tile (HW = 1000), logits at the existing test's spread, near-uniform and near-one-hot rows."""
    B = 2
    centers = make_centers(B, nb)
    for HW in (64, 1000, 76800 // 16):
        for scale in (3.0, 0.01, 40.0):
            logits = q(rnd(B * HW, nb, seed=1, scale=scale), dtype)
            la = to_act(logits, dtype)
            prob, pred, st = run_three_ways(lambda pr, pd, s: ops.bin_softmax(la, centers.to(DEV), pr, pd, B, HW, nb, stats=s), B, nb, HW, dtype)
            truth = truth_from_logits(logits.reshape(B, HW, nb), centers)
            check_rule(f"bin_softmax {dtype} nb={nb} HW={HW} scale={scale}", st, prob, centers, truth, 10.0)


@pytest.mark.parametrize("dtype", HALF)
def test_bin_head_fused_stats(dtype):
    """bin_head_fused_kernel (16-bit): the existing test's shapes (ragged last tile, two images inside one tile), three spreads."""
    B, Cin, nb = 2, 128, 256
    centers = make_centers(B, nb)
    for HW in (128 * 3, 1000, 4808):
        for f in (1.0, 0.003, 12.0):
            x = q(rnd(B * HW, Cin, seed=1), dtype)
            w = q(rnd(nb, Cin, seed=2, scale=0.25 * f), dtype)
            bias = rnd(nb, seed=3, scale=f)
            xa, wd = to_act(x, dtype), w.to(dtype).to(DEV)
            prob, pred, st = run_three_ways(
                lambda pr, pd, s: ops.bin_head_fused(xa, wd, bias.to(DEV), centers.to(DEV), pr, pd, B, HW, stats=s), B, nb, HW, dtype)
            truth = truth_from_logits((x.double() @ w.double().t() + bias.double()).reshape(B, HW, nb), centers)
            check_rule(f"bin_head_fused {dtype} HW={HW} spread x{f}", st, prob, centers, truth, 10.0)


@pytest.mark.parametrize("rows", [64, 128])
def test_bin_head_fused_x3_stats(rows):
    """bin_head_x3_kernel<64 | 128> (the default numerics; debug key 25 picks the pixel rows per workgroup)."""
    B, Cin, nb = 2, 128, 256
    centers = make_centers(B, nb)
    lib = hip.load()
    try:
        lib.cfp_debug_set(25, rows)
        for HW in (8 * 8, 30 * 40 + 4, 240 * 320):
            for f in (1.0, 0.003, 12.0):
                x = rnd(B * HW, Cin, seed=1)
                w = rnd(nb, Cin, seed=2, scale=0.25 * f)
                bias = rnd(nb, seed=3, scale=f)
                xa, wx = to_act(x, torch.float32), ops.pack_w_x3(w.contiguous().to(DEV))
                prob, pred, st = run_three_ways(
                    lambda pr, pd, s: ops.bin_head_fused(xa, wx, bias.to(DEV), centers.to(DEV), pr, pd, B, HW, stats=s), B, nb, HW, torch.float32)
                truth = truth_from_logits((x.double() @ w.double().t() + bias.double()).reshape(B, HW, nb), centers)
                check_rule(f"bin_head_x3<{rows}> HW={HW} spread x{f}", st, prob, centers, truth, 10.0)
    finally:
        lib.cfp_debug_set(25, 64)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("hilo", [(True, True), (False, False)])
def test_depth_head_fused_stats(hilo, dtype):
    """depth_head_fused_kernel with and without the hi / lo islands: the existing test's shapes (tiles that straddle rows and images, a
    ragged last tile, an input pitch > 128), three spreads of conv_out."""
    for (B, H, W, ld) in [(2, 12, 20, 128), (1, 16, 24, 136), (3, 8, 18, 128), (1, 40, 64, 128)]:
        M = B * H * W
        centers = make_centers(B, 256)
        x = q(rnd(M, 128, seed=1), dtype)
        w3 = rnd(128, 128, 3, 3, seed=2, scale=1.0 / math.sqrt(9 * 128))
        b3 = rnd(128, seed=3, scale=0.5)
        w3q = ops.round_taps(w3, dtype)
        w3p = w3q.permute(0, 2, 3, 1).reshape(128, 9 * 128).to(dtype).to(DEV).contiguous()
        xa = to_act(x, dtype, ld=ld)
        xi = x.double().reshape(B, H, W, 128).permute(0, 3, 1, 2)
        ram = F.conv2d(xi, w3q.double(), b3.double(), padding=1)
        ram = ram if hilo[1] else ram.float().to(dtype).double()
        for f in (1.0, 0.002, 6.0):
            wo = rnd(256, 128, seed=4, scale=0.6 * f)
            bo = rnd(256, seed=5, scale=f)
            wop = ops.permute_wout(wo, dtype, hilo=hilo[0]).to(DEV)

            def call(pr, pd, s):
                ops.depth_head_fused(xa, w3p, None, b3.to(DEV), wop, bo.to(DEV), centers.to(DEV), pr, pd.reshape(-1), B, H, W,
                                     ram_hilo=hilo[1], stats=s)
            prob, pred, st = run_three_ways(call, B, 256, H * W, dtype)
            wo_eff = wo if hilo[0] else q(wo, dtype)
            logits = F.conv2d(ram, wo_eff.double()[:, :, None, None], bo.double()).reshape(B, 256, H * W).permute(0, 2, 1)
            check_rule(f"depth_head_fused {dtype} hilo={hilo} {B}x{H}x{W} spread x{f}", st, prob, centers, truth_from_logits(logits, centers), 10.0)


# ---- 5. closed forms --------------------------------------------------------------------------------------------------------------------
def _closed_form_checks(what, st, centers, HW, peaked):
    st = st.double().cpu()
    if not peaked:
        want_std = centers.double().std(dim=1, unbiased=False)
        assert float((st[:, 0] - want_std[:, None]).abs().max()) <= FLOOR_STD_PER_M * 10.0, what
        assert float((st[:, 1] - math.log(256)).abs().max()) <= FLOOR_ENT, what
        assert float((st[:, 2] * 256 - 1).abs().max()) <= FLOOR_PMAX, what
    else:
        assert 0 <= float(st[:, 0].min()) and float(st[:, 0].max()) <= FLOOR_STD_PER_M * 10.0, what
        assert 0 <= float(st[:, 1].min()) and float(st[:, 1].max()) <= FLOOR_ENT, what
        assert bool((st[:, 2] == 1).all()), what


@pytest.mark.parametrize("peaked", [False, True])
def test_closed_forms_bin_softmax(peaked):
    """All logits equal: entropy ln 256, pmax 1/256, std = population std of the image's centres.  One logit 100 above the rest: entropy
    and std inside [0, floor], pmax exactly 1."""
    B, HW, nb = 2, 1000, 256
    centers = make_centers(B, nb)
    logits = torch.full((B * HW, nb), 0.75)
    if peaked:
        logits[torch.arange(B * HW), torch.arange(B * HW) % nb] += 100.0
    pred = torch.empty(B, HW, device=DEV)
    st = torch.full((B, 3, HW), float("nan"), device=DEV)
    ops.bin_softmax(to_act(logits, torch.float32), centers.to(DEV), None, pred, B, HW, nb, stats=st)
    torch.cuda.synchronize()
    _closed_form_checks(f"bin_softmax peaked={peaked}", st, centers, HW, peaked)


@pytest.mark.parametrize("peaked", [False, True])
def test_closed_forms_x3_head(peaked):
    """The same through the default mode's fused head with zero weights: the logits are the bias."""
    B, HW, Cin, nb = 2, 30 * 40 + 4, 128, 256
    centers = make_centers(B, nb)
    bias = torch.full((nb,), -0.5)
    if peaked:
        bias[37] += 100.0
    wx = ops.pack_w_x3(torch.zeros(nb, Cin, device=DEV))
    pred = torch.empty(B, HW, device=DEV)
    st = torch.full((B, 3, HW), float("nan"), device=DEV)
    ops.bin_head_fused(to_act(rnd(B * HW, Cin, seed=1), torch.float32), wx, bias.to(DEV), centers.to(DEV), None, pred, B, HW, stats=st)
    torch.cuda.synchronize()
    _closed_form_checks(f"x3 head peaked={peaked}", st, centers, HW, peaked)


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------------
def _full_case(B, H, W, zn, zpx, seed, drop):
    layers = spec.COMBINE1_LAYERS
    sd = weights.make_torch_state_dict(spec.model_manifest(layers))
    inp = synthetic.make_inputs(B, H, W, zn, zpx, seed=seed, drop_hist=drop)
    return layers, sd, inp


@pytest.fixture(scope="module")
def full_case():
    """The two-image 480x640 case with 34 % dropped zones of test_full_model_vs_oracle_f32, and the CPU oracle's float64 truth."""
    layers, sd, inp = _full_case(2, 480, 640, 8, 56, 9, 0.34)
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    e0, p0, pr0 = O.forward(sd, inp, layer_names=layers)
    e = e0.double()
    centers = 0.5 * (e[:, :-1] + e[:, 1:])
    B, nb, h, w = pr0.shape
    truth = stats_from_prob(pr0.reshape(B, nb, h * w), centers)
    return layers, sd, inp, centers, truth


MODES = {"f32x3": dict(dtype=torch.float32, x3=True), "f32": dict(dtype=torch.float32), "fp16": dict(dtype=torch.float16),
         "bf16": dict(dtype=torch.bfloat16)}


@pytest.mark.parametrize("mode", list(MODES))
def test_engine_uncertainty_vs_oracle(full_case, mode):
    """f32x3 reaches bin_head_x3_kernel, plain f32 bin_softmax_kernel, fp16 / bf16 depth_head_fused_kernel."""
    layers, sd, inp, centers, truth = full_case
    eng = Engine(sd, layer_names=layers, **MODES[mode])
    span = eng.max_val - eng.min_val
    dinp = synthetic.to_device(inp, DEV)
    e0, p0, pr0 = eng.forward(dinp)                                      # the call without the feature: today's 3-tuple
    e0, p0, pr0 = e0.clone(), p0.clone(), pr0.clone()
    e1, p1, pr1, u1 = eng.forward(dinp, uncertainty=True)
    torch.cuda.synchronize()
    assert u1.shape == (2, 3, 240, 320) and u1.dtype == torch.float32
    assert torch.equal(e0, e1) and torch.equal(p0, p1) and torch.equal(pr0, pr1)
    u1 = u1.clone()
    check_rule(f"{mode} eager", u1, pr0, centers, truth, span)
    # return_prob=False composes with it: the point of the feature
    out = eng.forward(dinp, uncertainty=True, return_prob=False)
    torch.cuda.synchronize()
    assert len(out) == 4 and out[2] is None and torch.equal(out[3], u1) and torch.equal(out[1], p0)
    # single-graph replay: bit for bit the eager map
    cap = eng.capture(dinp, uncertainty=True)
    assert len(cap) == 4
    rep = eng.replay(dinp)
    torch.cuda.synchronize()
    assert len(rep) == 4 and torch.equal(rep[3], u1) and torch.equal(rep[1], p0) and torch.equal(rep[2], pr0)
    assert len(eng.capture(dinp)) == 3 and len(eng.replay(dinp)) == 3   # without the keyword: the 3-tuple of today
    # two batches in flight: the other kernel plan (re-association noise upstream), both slots inside the rule, equal on the same input
    eng.capture(dinp, inflight=2, uncertainty=True)
    slots = []
    for _ in range(2):
        o, ev = eng.replay_async(dinp)
        ev.synchronize()
        assert len(o) == 4
        slots.append(o)
    assert slots[0][3].data_ptr() != slots[1][3].data_ptr()
    assert torch.equal(slots[0][3], slots[1][3])
    for i, o in enumerate(slots):
        check_rule(f"{mode} inflight slot {i}", o[3], o[2], centers, truth, span)


def _boundary_model():
    from cfpnet_amd import config
    from cfpnet_amd.deltar import make_model
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = config.parse_args(["@" + os.path.join(root, "configs", "cfpnet_combine1.txt")])
    return make_model(args).eval().to(DEV)


@pytest.mark.parametrize("graphs", [True, False])
def test_model_boundary_returns_the_map_as_element_3(graphs):
    """`model(input_data, return_uncertainty=True)`: the map of the module's own engine (whose accuracy the test above pins), bit for bit."""
    _, _, inp = _full_case(2, 480, 640, 8, 56, 9, 0.34)
    model = _boundary_model()
    model.eval_graphs = graphs
    a = synthetic.to_device(inp, DEV)
    b = synthetic.to_device(synthetic.make_inputs(2, 480, 640, 8, 56, seed=4, drop_hist=0.1), DEV)
    eng = model.engine(DEV)
    want_a = eng.forward(a, uncertainty=True)[3].clone()
    want_b = eng.forward(b, uncertainty=True)[3].clone()
    plain = model(a)
    assert len(plain) == 4 and plain[3] is None                          # without the flag the tuple still ends in None
    ra = model(a, return_uncertainty=True)
    rb = model(b, return_uncertainty=True)                               # a fresh tensor by default: the first result stays intact
    torch.cuda.synchronize()
    assert len(ra) == 4 and ra[3].shape == (2, 3, 240, 320) and ra[3].dtype == torch.float32
    assert ra[3].data_ptr() != rb[3].data_ptr()
    assert torch.equal(ra[3], want_a) and torch.equal(rb[3], want_b) and torch.equal(ra[1], plain[1])
    out = model(a, return_uncertainty=True, return_prob=False)
    torch.cuda.synchronize()
    assert out[2] is None and torch.equal(out[3], want_a)
    if graphs:                                                           # the opt-in ring semantics: the ring's own buffers
        model.eval_static_outputs = True
        model.eval_out_ring = 2
        r = [model(x, return_uncertainty=True)[3] for x in (a, b, a)]
        torch.cuda.synchronize()
        assert r[0].data_ptr() == r[2].data_ptr() != r[1].data_ptr()
        assert torch.equal(r[1], want_b) and torch.equal(r[2], want_a)
