"""`cfp_eval_metrics_regions` on the GPU against the numpy restatement of its definition (`region_metrics_ref.py`, itself checked in
test_region_metrics_abi.py), its consistency properties, `--zone_type` in the eval input builder and the engine, and the new
switches of evaluate_all.py.

Tolerance: the project's own (tests/test_metrics.py): |got - want| <= 2e-5 * max(|want|, 1e-3) per metric, counts exact.  Both sides
evaluate the same float32 terms; the oracle sums them in float32, the kernel in float64, and test_region_metrics_abi.py shows that on
these very inputs the summation order costs under a quarter of that bound down to the smallest segment."""
import contextlib
import copy
import io
import json
import os

import numpy as np
import pytest
import torch

import region_metrics_ref as R

pytestmark = pytest.mark.gpu

from cfpnet_amd import config, data, geometry, metrics, spec, synthetic, weights  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu(pred, gt, rect, mask, edges, mode=0, lo=R.LO, hi=R.HI):
    """Batched numpy inputs -> (table [B,5,Q,9], counts [B,5,Q]) from the device."""
    t = metrics.region_metrics(torch.from_numpy(np.array(pred)).to(DEV), torch.from_numpy(np.array(gt)).to(DEV), lo, hi,
                               torch.from_numpy(np.array(rect)).to(DEV), torch.from_numpy(np.array(mask)).to(DEV), edges, mode=mode)
    assert t.dtype == torch.float64 and t.is_cuda
    a = t.cpu().numpy()
    return a[..., :9], a[..., 9]


# ---- 1. the kernel against the reference -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(R.CASES))
def test_kernel_matches_the_reference(name, mode):
    gt, pred, rect, mask, edges = R.case_inputs(name)
    want, counts = R.case_reference(name, mode)
    got, n = gpu(pred[None], gt[None], rect[None], mask[None], edges, mode)
    Q = 1 if not edges else len(edges) + 2
    assert got.shape == (1, 5, Q, 9) and want.shape == (5, Q, 9)
    if name == "overhang_top_left_E7":
        assert (counts > 0).sum() * 2 >= counts.size                       # at least half of the segments are non-empty
    if name == "full_size":
        assert (n[0, :, 3] == 0).all() and np.isnan(got[0, :, 3]).all()     # nothing at or beyond 4 m, in every region
    R.close(got[0], want, n[0], counts, f"{name} mode {mode}")


def test_batch_of_three_with_an_image_without_zones_and_an_empty_image():
    gt, pred, rect, mask, edges = R.batch_inputs()
    for mode in (0, 1):
        got, n = gpu(pred, gt, rect, mask, edges, mode)
        for b in range(3):
            want, counts = R.reference(pred[b], gt[b], R.LO, R.HI, rect[b], mask[b], edges, mode)
            R.close(got[b], want, n[b], counts, f"batch image {b} mode {mode}")
        assert (n[1, 3] == 0).all() and np.array_equal(n[1, 4], n[1, 1]) and n[1, 1, 0] > 0       # every zone dropped
        assert np.array_equal(got[1, 4], got[1, 1], equal_nan=True)
        assert (n[2] == 0).all() and np.isnan(got[2]).all()                                         # no valid pixel at all
        assert n[0, 3, 0] > 0 and n[0, 4, 0] > 0


# ---- 2. consistency --------------------------------------------------------------------------------------------------------------------

def test_repeatability_the_all_row_and_additive_counts():
    gt, pred, rect, mask, edges = R.batch_inputs()
    P, G = torch.from_numpy(pred.copy()).to(DEV), torch.from_numpy(gt.copy()).to(DEV)
    Rc, M = torch.from_numpy(rect.copy()).to(DEV), torch.from_numpy(mask.copy()).to(DEV)
    for mode in (metrics.EVALUATE_ALL, metrics.VALIDATE):
        first = metrics.region_metrics(P, G, R.LO, R.HI, Rc, M, edges, mode=mode)
        again = metrics.region_metrics(P, G, R.LO, R.HI, Rc, M, edges, mode=mode)
        into = torch.empty_like(first)
        assert metrics.region_metrics(P, G, R.LO, R.HI, Rc, M.to(torch.uint8), edges, mode=mode, out=into) is into
        plain = metrics.eval_metrics(P, G, R.LO, R.HI, mode=mode).cpu().numpy()
        a, b, c = first.cpu().numpy(), again.cpu().numpy(), into.cpu().numpy()
        assert a.tobytes() == b.tobytes() == c.tobytes()                                         # bit-identical launches
        # all/all is cfp_eval_metrics: the same float32 terms in float64, another summation order
        assert np.array_equal(a[:, 0, 0, 9], plain[:, 9])
        for img in range(2):
            rel = np.abs(a[img, 0, 0, :9] - plain[img, :9]) / np.abs(plain[img, :9])
            print(f"mode {mode} image {img}: all/all vs cfp_eval_metrics, worst relative difference {rel.max():.3e}")
            assert rel.max() <= 1e-10
        assert np.isnan(a[2, 0, 0, :9]).all() and np.isnan(plain[2, :9]).all()
        n = a[..., 9]
        assert np.array_equal(n[:, 1] + n[:, 2], n[:, 0]) and np.array_equal(n[:, 3] + n[:, 4], n[:, 1])
        assert np.array_equal(n[:, :, 1:].sum(2), n[:, :, 0])
    # without edges: Q = 1 and the same "all depths" rows, bit for bit
    q1 = metrics.region_metrics(P, G, R.LO, R.HI, Rc, M).cpu().numpy()
    full = metrics.region_metrics(P, G, R.LO, R.HI, Rc, M, edges).cpu().numpy()
    assert q1.shape == (3, 5, 1, 10) and np.array_equal(q1[:, :, 0, 9], full[:, :, 0, 9])
    ne = ~np.isnan(full[:, :, 0, :9])
    assert np.abs(q1[:, :, 0, :9][ne] - full[:, :, 0, :9][ne]).max() <= 1e-12
    with pytest.raises(RuntimeError, match="strictly increasing"):
        metrics.region_metrics(P, G, R.LO, R.HI, Rc, M, (2.0, 1.0))
    with pytest.raises(ValueError):
        metrics.region_metrics(P, G, R.LO, R.HI, Rc, M, tuple(range(1, 9)))
    with pytest.raises(ValueError):
        metrics.region_metrics(P, G, R.LO, R.HI, Rc[:, :4], M)


def test_running_region_average_over_a_split_batch():
    gt, pred, rect, mask, edges = R.batch_inputs()
    rows = metrics.region_metrics(torch.from_numpy(pred.copy()).to(DEV), torch.from_numpy(gt.copy()).to(DEV), R.LO, R.HI,
                                  torch.from_numpy(rect.copy()).to(DEV), torch.from_numpy(mask.copy()).to(DEV), edges)
    run = metrics.RunningRegionAverage(edges)
    run.update(rows[:1])
    run.update(rows[1:])
    val = run.get_value()
    a = rows.cpu().numpy()
    labels = metrics.range_labels(edges)
    assert list(val) == list(metrics.REGIONS) and all(list(val[r]) == list(labels) for r in val)
    skipped = 0
    for ri, region in enumerate(metrics.REGIONS):
        for qi, label in enumerate(labels):
            imgs = [b for b in range(3) if a[b, ri, qi, 9] > 0]
            assert run.image_counts[region][label] == len(imgs)
            skipped += 3 - len(imgs)
            if not imgs:
                assert val[region][label] == {}
                continue
            for k, key in enumerate(metrics.KEYS):
                want = a[imgs, ri, qi, k].mean()
                assert abs(val[region][label][key] - want) <= 1e-12 * max(abs(want), 1.0), (region, label, key)
    assert skipped > 20                                                       # image 2 everywhere, image 1 in zone_valid


# ---- 3. --zone_type --------------------------------------------------------------------------------------------------------------------

def _args(zone_type):
    a = copy.copy(config.defaults())
    a.zone_type = zone_type
    return a


def test_eval_input_builder_zone_types_equal_the_gather_from_the_8x8_build():
    samples = list(data.SyntheticEvalSamples(2, 480, 640))
    img, dep, _ = next(data.batches(samples, 2))
    full, gt8 = data.EvalInputBuilder(_args("8x8"), DEV)(img, dep)
    f = full["additional"]
    assert f["rect_data"].shape == (2, 64, 4) and int(f["patch_info"]["zone_num"][0]) == 8
    for zt, n in (("2x2", 2), ("4x4", 4), ("6x6", 6)):
        inp, gt = data.EvalInputBuilder(_args(zt), DEV)(img, dep)
        a = inp["additional"]
        idx = torch.from_numpy(geometry.central_zone_block(zt)).to(DEV)
        assert torch.equal(gt, gt8) and torch.equal(inp["rgb"], full["rgb"])
        for k in ("hist_data", "rect_data", "mask"):
            assert a[k].shape[1] == n * n and a[k].dtype == f[k].dtype
            assert a[k].cpu().numpy().tobytes() == f[k][:, idx].contiguous().cpu().numpy().tobytes(), (zt, k)
        rects = geometry.centered_zone_rects(480, 640, 8, 56)[geometry.central_zone_block(zt)]
        assert np.array_equal(a["rect_data"][0].cpu().numpy(), rects)
        want = geometry.collate_patch_info([geometry.patch_info_from_rect_data(rects, (480, 640))] * 2)
        assert a["patch_info"]["zone_num"].tolist() == [n, n]
        for s in (4, 8, 16):
            for k in ("pad_size", "patch_size", "index_wo_pad"):
                assert np.array_equal(a["patch_info"][s][k].numpy(), want[s][k]), (zt, s, k)
    with pytest.raises(ValueError, match="zone_type"):
        data.EvalInputBuilder(_args("3x3"), DEV)


def _block_inputs(zone_type, seed):
    """The 480x640 batch of one image the builder would hand over: the 8x8 inputs, central block kept, patch_info of the kept rectangles."""
    inp = synthetic.make_inputs(1, 480, 640, 8, 56, seed=seed, drop_hist=0.34)
    idx = torch.from_numpy(geometry.central_zone_block(zone_type))
    add = inp["additional"]
    kept = {k: add[k][:, idx].contiguous() for k in ("hist_data", "rect_data", "mask")}
    pi = geometry.collate_patch_info([geometry.patch_info_from_rect_data(kept["rect_data"][0].numpy(), (480, 640))])
    kept["patch_info"] = {s: {k: torch.from_numpy(v) for k, v in pi[s].items()} for s in (4, 8, 16)}
    kept["patch_info"]["zone_num"] = torch.from_numpy(pi["zone_num"])
    return {"rgb": inp["rgb"], "additional": kept}


@pytest.mark.parametrize("case", ["2x2_480x640", "4x4_480x640", "2x2_grid_256x320"])
def test_engine_on_small_zone_grids_vs_oracle(case):
    """The default numerics (f32x3) on the geometries `--zone_type` produces, inside the project's 1e-3 rel-L1 gate per image."""
    from cfpnet_amd.engine import Engine
    from oracle import cfpnet_oracle as O
    layers = spec.COMBINE1_LAYERS
    sd = weights.make_torch_state_dict(spec.model_manifest(layers))
    if case == "2x2_grid_256x320":
        inp = synthetic.make_inputs(2, 256, 320, 2, 56, seed=31, drop_hist=0.25)
        assert inp["additional"]["mask"].sum(1).tolist() == [3, 3]             # one zone dropped per image
        shape = (2, 1, 128, 160)
    else:
        inp = _block_inputs(case[:3], seed=33 if case[0] == "2" else 34)
        assert int(inp["additional"]["mask"].sum()) >= 1
        shape = (1, 1, 240, 320)
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    _, p0, _ = O.forward(sd, inp, layer_names=layers)
    eng = Engine(sd, layer_names=layers, device=DEV)
    assert eng.x3 and eng.dtype == torch.float32
    _, p1, _ = eng.forward(synthetic.to_device(inp, DEV))
    torch.cuda.synchronize()
    assert tuple(p1.shape) == shape and bool(torch.isfinite(p1).all())
    for b in range(shape[0]):
        r = float(np.abs(p1[b].cpu().numpy() - p0[b].numpy()).sum() / np.abs(p0[b].numpy()).sum())
        print(f"{case} image {b}: pred rel-L1 vs oracle = {r:.3e}")
        assert r < 1e-3, (case, b, r)


# ---- 4. the command line ---------------------------------------------------------------------------------------------------------------

BASE = ["@configs/cfpnet_combine1.txt", "--selected_epoch", "best", "--synthetic", "3", "--batch", "2", "--dtype", "f32"]
EDGES = (1.0, 2.0)


def _cli(argv):
    import evaluate_all
    out, err = io.StringIO(), io.StringIO()
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
            res = evaluate_all.main(list(argv))
    finally:
        os.chdir(cwd)
    return res, out.getvalue().splitlines()


@pytest.fixture(scope="module")
def chain():
    """The same three samples through the CPU oracles: ToF simulation, forward, then the reference per segment; running means with the
    images skipped where a segment is empty.  -> (means {region: {label: {key: value}}}, image counts)."""
    from oracle import cfpnet_oracle as O
    from oracle import tof_oracle as TO
    layers = spec.COMBINE1_LAYERS
    sd = weights.make_torch_state_dict(spec.model_manifest(layers))
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    tables, counts = [], []
    for img, dep, _ in data.batches(data.SyntheticEvalSamples(3), 2):
        B, _, H, W = img.shape
        sims = [TO.get_hist(dep[b, 0].numpy()) for b in range(B)]
        pi = geometry.collate_patch_info([geometry.patch_info_from_rect_data(s["fr"], (H, W)) for s in sims])
        pinfo = {s: {k: torch.from_numpy(v) for k, v in pi[s].items()} for s in (4, 8, 16)}
        pinfo["zone_num"] = torch.from_numpy(pi["zone_num"])
        inp = {"rgb": img, "additional": {"hist_data": torch.from_numpy(np.stack([s["pts"] for s in sims])),
                                          "rect_data": torch.from_numpy(np.stack([s["fr"] for s in sims])),
                                          "mask": torch.from_numpy(np.stack([s["mask"] for s in sims])), "patch_info": pinfo}}
        _, pred, _ = O.forward(sd, inp, layer_names=layers)
        for b in range(B):
            t, c = R.reference(pred[b, 0].numpy(), dep[b, 0].numpy(), 1e-3, 10.0, sims[b]["fr"], sims[b]["mask"], EDGES, 0)
            tables.append(t)
            counts.append(c)
    tables, counts = np.stack(tables), np.stack(counts)
    labels = metrics.range_labels(EDGES)
    means, images = {}, {}
    for ri, region in enumerate(metrics.REGIONS):
        means[region], images[region] = {}, {}
        for qi, label in enumerate(labels):
            keep = counts[:, ri, qi] > 0
            images[region][label] = int(keep.sum())
            means[region][label] = dict(zip(metrics.KEYS, tables[keep, ri, qi].mean(0))) if keep.any() else {}
    return means, images


def _near(got, want, what):
    """The bound of test_eval_pipeline.py: f32 engine against the oracle, printed values rounded to 3 decimals."""
    assert list(got) == list(want), what
    for k in want:
        assert abs(got[k] - want[k]) <= 2e-3 * max(abs(want[k]), 1e-2) + 6e-4, (what, k, got[k], want[k])


def test_cli_region_metrics_against_the_reference_chain(chain, tmp_path):
    means, images = chain
    plain, lines0 = _cli(BASE)
    res, lines = _cli(BASE + ["--region_metrics", "--range_edges", "1,2", "--save_dir", str(tmp_path)])
    assert len(lines0) == 2 and len(lines) == 3 and lines[:2] == lines0 and res == plain          # the first two lines do not change
    assert lines[2].startswith("Regions: {")
    printed = eval(lines[2][len("Regions: "):], {"nan": float("nan")})
    assert list(printed) == list(metrics.REGIONS)
    n_seg = 0
    for region in metrics.REGIONS:
        assert list(printed[region]) == ["all", "<1", "1-2", ">=2"]
        for label, want in means[region].items():
            _near(printed[region][label], want, (region, label))
            n_seg += bool(want)
    assert n_seg >= 15
    _near(plain, means["all"]["all"], "Metrics line")
    saved = json.load(open(os.path.join(str(tmp_path), "regions.json")))
    assert saved["regions"] == list(metrics.REGIONS) and saved["ranges"] == ["all", "<1", "1-2", ">=2"] and saved["range_edges"] == [1.0, 2.0]
    assert saved["metrics"] == list(metrics.KEYS) and np.array(saved["table"], dtype=object).shape == (5, 4, 9)
    assert saved["images"] == [[images[r][q] for q in saved["ranges"]] for r in saved["regions"]]
    for ri, region in enumerate(saved["regions"]):
        for qi, label in enumerate(saved["ranges"]):
            if printed[region][label]:
                assert [round(v, 3) for v in saved["table"][ri][qi]] == list(printed[region][label].values())
            else:
                assert saved["table"][ri][qi] == [None] * 9
    # after `Uncertainty:` when that is present
    _, lines3 = _cli(BASE + ["--region_metrics", "--unc_metrics"])
    assert len(lines3) == 4 and lines3[:2] == lines0 and lines3[2].startswith("Uncertainty: {") and lines3[3].startswith("Regions: {")
    assert eval(lines3[3][len("Regions: "):], {"nan": float("nan")})["fov_in"] == {"all": printed["fov_in"]["all"]}


def test_cli_area_flags_print_the_region_rows(chain):
    means, _ = chain
    res_in, lines_in = _cli(BASE + ["--zone_area_only"])
    res_out, lines_out = _cli(BASE + ["--outside_zone_area_only"])
    assert len(lines_in) == 2 and len(lines_out) == 2 and lines_in[0].startswith("Metrics: {")
    assert lines_in[1] == ",".join(str(v) for v in res_in.values())
    _near(res_in, means["fov_in"]["all"], "--zone_area_only")
    _near(res_out, means["fov_out"]["all"], "--outside_zone_area_only")
    assert res_in != res_out
    with pytest.raises(ValueError, match="exclude each other"):
        _cli(BASE + ["--zone_area_only", "--outside_zone_area_only"])
    with pytest.raises(ValueError, match="zone_type"):
        _cli(BASE + ["--zone_type", "5x5"])


def test_cli_zone_type_4x4_shrinks_the_fov():
    """`--zone_type 4x4 --zone_area_only` against the same pipeline by hand; the FoV of the kept zones is the central 224 x 224 square."""
    from cfpnet_amd.deltar import make_model
    res, lines = _cli(BASE + ["--zone_type", "4x4", "--zone_area_only"])
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        args = config.parse_args(list(BASE[:3]) + ["--zone_type", "4x4"])
    finally:
        os.chdir(cwd)
    model = make_model(args, dtype=torch.float32).to(torch.device(DEV)).eval()
    avg = metrics.RunningAverageDict()
    n4, n8, deps = [], [], []
    with torch.no_grad():
        for img, dep, _ in data.batches(data.SyntheticEvalSamples(3, 480, 640), 2):
            inp, gt = data.EvalInputBuilder(args, torch.device(DEV))(img, dep)
            assert inp["additional"]["rect_data"].shape[1] == 16
            _, pred, _, _ = model(inp)
            rows = metrics.region_metrics(pred, gt, 1e-3, 10.0, inp["additional"]["rect_data"], inp["additional"]["mask"])
            avg.update(rows[:, 1, 0])
            n4 += rows[:, 1, 0, 9].cpu().tolist()
            full, _ = data.EvalInputBuilder(_args("8x8"), torch.device(DEV))(img, dep)
            rows8 = metrics.region_metrics(pred, gt, 1e-3, 10.0, full["additional"]["rect_data"], full["additional"]["mask"])
            n8 += rows8[:, 1, 0, 9].cpu().tolist()
            # the same prediction: the all row keeps its counts; its sums are the same float32 terms added over another partition into
            # cells, so the metrics agree to float64 rounding (the 1e-10 of the all/all row against cfp_eval_metrics), not bit for bit
            a8, a4 = rows8[:, 0, 0].cpu().numpy(), rows[:, 0, 0].cpu().numpy()
            assert np.array_equal(a8[:, 9], a4[:, 9]) and (np.abs(a8[:, :9] - a4[:, :9]) <= 1e-10 * np.abs(a8[:, :9])).all()
            deps += [d[0].numpy() for d in dep]
    assert res == {k: round(v, 3) for k, v in avg.get_value().items()} and len(res) == 9
    for b, d in enumerate(deps):
        valid = (d > 1e-3) & (d < 10.0)
        assert n4[b] == valid[128:352, 208:432].sum() and n8[b] == valid[16:464, 96:544].sum() and 0 < n4[b] < n8[b]
