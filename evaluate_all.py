#!/usr/bin/env python3
"""Evaluation with the reference's CLI and protocol (`/root/reference/evaluate_all.py:44-167`):

    python evaluate_all.py @configs/cfpnet_combine1.txt --selected_epoch best [--synthetic 64] [--dtype f32x3|f32|f16|bf16] [--bs 8]

Per batch: ToF simulation from the ground-truth depth (GPU, `cfp_tof_hist_sim`), model forward (HIP engine), then
`np.clip` -> bilinear to full resolution -> `min_depth < gt < max_depth` mask -> the nine `compute_errors` metrics, all in
one device kernel (`cfp_eval_metrics`, mode 0); the per-image rows stay on the device and the running average is
formed once at the end -- the reference moves prediction and ground truth to the host for every image.
Prints `Metrics: {...}` rounded to 3 decimals and the comma-joined line, like `evaluate_all.py:88-90`.

`--save_entropy` (with `--save_dir D`, default `tmp`) also asks the model for its per-pixel uncertainty map and writes, per evaluated
batch, `D/unc_<index of the batch's first image>.npy`: float32 `[B,3,h,w]`, planes std of the bin distribution (m), entropy (nats), largest
bin probability.  The metrics and everything printed are the same with and without it.

`--unc_metrics [--unc_steps K]` (K = 20 by default, 1..100) rates that uncertainty map against the ground truth on the device
(`cfp_unc_sparsification`): sparsification curves of the three planes and of the two oracles at K removal fractions, AUSE and AURG per
image, averaged over the images with valid pixels.  It prints a third line `Uncertainty: {...}` with the twelve means rounded to 4 decimals
and, with `--save_dir D` given, writes `D/sparsification.json` with the mean curves.  The first two lines do not change.

`--zone_type 6x6|4x4|2x2` feeds the model the central block of the 8x8 zone grid only (the reference's zjuL5 loader).  `--zone_area_only` /
`--outside_zone_area_only` compute the two metric lines over the pixels inside / outside the field of view of the kept zones (the reference's
`my_mask`: the rectangle spanned by the first and the last zone); images without a valid pixel there are skipped; giving both is an error.
`--region_metrics [--range_edges 2,4]` splits the metrics by region (all, fov_in, fov_out, zone_valid, zone_invalid) and by ground-truth depth
range on the device (`cfp_eval_metrics_regions`); it prints one more line `Regions: {...}` (after `Uncertainty:` when that is present) and, with
`--save_dir D` given, writes `D/regions.json` with the labels, the table and the image counts.  With none of these flags the code path and the
output are what they were.

`--save_points` back-projects every prediction to 3-D points in the camera frame on the device (`cfp_depth_unproject`, the depth being the
clipped, bilinearly enlarged prediction the metrics evaluate), keeps the pixels of every `--points_stride N`-th row and column (N = 2 by
default) whose depth lies strictly inside (min_depth, max_depth) and -- with `--points_max_std S` -- whose predicted standard deviation (plane
0 of the uncertainty map, metres) is at most S (`cfp_points_compact`), and writes `D/points_<image index>.ply` per image into `--save_dir D`
(default `tmp`): binary PLY with x y z, the surface normal with `--points_normals`, and the de-normalised RGB.  `--intrinsics fx,fy,cx,cy`
(pixels of the full-resolution image) defaults to the ZJU-L5 sensor's.  One more stderr line reports the mean number of points kept; the
`Metrics:` lines do not change.  The `--points_*` switches without `--save_points`, and `--intrinsics` without `--save_points` or
`--normal_metrics`, are an error.

`--normal_metrics` rates the geometry on the device (`cfp_normal_metrics`): the angle between the surface normal of the prediction and that
of the ground-truth depth, both formed as `--save_points` forms its normals, over the pixels whose ground truth and its four neighbours are
valid.  It prints one more line `Normals: {...}` (after `Regions:` and `Uncertainty:` when those are present) with the means of mean_deg,
median_deg, rmse_deg and the shares below 11.25 / 22.5 / 30 degrees over the images with a valid pixel, rounded to 3 decimals, and the number
of those images; with `--save_dir D` given it writes `D/normals.json` with the names, the means and the 0.1-degree histogram summed over the
images.  `--intrinsics` applies.  The other lines do not change.

`--zone_consistency` asks whether the prediction agrees with what the sensor measured -- the check that needs no ground truth
(`cfp_tof_zone_consistency`): the ToF zones are re-simulated from the prediction with the sensor model of the simulation and compared with
the (mu, sigma) the model was fed from, per zone.  It prints one more line `ZoneConsistency: {...}` (after `Normals:` when that is present)
with the means over the images with a compared zone, rounded to 4 decimals, and the number of those images; with `--save_dir D` given it
writes `D/zone_consistency.json` with the names, the means and the zone table of every image.  It uses `--simu_max_distance`, the distance
the measurement was made with: with `--random_simu_max_d` that distance is not known afterwards and the switch is an error.  The other lines
do not change.

`--robust_drop a,b,...` and `--robust_sigma a,b,...` build a robustness table: for each listed value the same images go through the model
once more with that one degradation of the ToF input applied on the device (`cfp_tof_degrade`) -- a fraction of every image's
valid zones dropped at random (with replacement, like `--drop_hist` in training), or Gaussian noise of that standard deviation in metres
added to the mu of every valid zone.  The draws are keyed by `--robust_seed` (117010053 by default) and the index of the batch.  One more
line, `Robustness: {"drop": {"0.25": {...}}, "sigma": {...}}` (JSON; the nine metrics rounded to 3 decimals), is printed last on stdout, and
`<save_dir>/robustness.json` holds the same with the mean counts per image of valid zones, zones dropped and zones noised.  A listed value of
0 reproduces the `Metrics:` line.  The other lines do not change.

`--robust_frames N` (N >= 2, with `--robust_drop` or `--robust_sigma`) asks how much of a degradation fusing N frames recovers: every
degraded run is repeated with N - 1 further draws of the same degradation (frame 0 is the draw above, frame f is keyed by the index of the
batch + f * 2^20), the N predictions and their standard-deviation planes go through a `temporal.TemporalFilter` with the identity pose
(`cfp_depth_reproject`, `cfp_depth_fuse`) and the fused frame is evaluated like a prediction.  The `Robustness:` line and
`robustness.json` gain one key, `"fused": {"frames": N, "drop": {...}, "sigma": {...}}`; without the switch nothing changes.

`--save_pred`, `--save_gt`, `--save_rgb`, `--save_error_map` and `--save_for_demo` (the reference's picture switches) paint on the device
(`cfpnet_amd/render.py`: `cfp_render_depth`, `cfp_render_zones`, `cfp_render_rgb`) and write, per evaluated image index i, into `--save_dir D`
(default `tmp`): `D/pred_<i>.png` (colour) and `D/pred_<i>_mm.png` (16-bit millimetres of the clipped, enlarged prediction the metrics
evaluate); `D/gt_<i>.png` (invalid pixels white); `D/rgb_<i>.png`; `D/error_<i>.png` (absolute error over [0, `--error_max` = 1.0 m] in `jet`,
with `--error_rel` the relative error over [0, `--error_max`]); `D/demo_<i>.png` (image | image under the ToF zones / prediction | error).
`--vis_cmap NAME` (magma_r, magma, viridis, turbo, jet) and `--vis_range a,b` (default min_depth,max_depth) apply to the prediction, the
ground truth and the zones.  One more stderr line reports the number of files; stdout does not change.  `--vis_cmap`, `--vis_range`,
`--error_max` and `--error_rel` without one of the five switches, and an unknown table name, are errors raised before the model is built.

Differences on purpose: the xlsx report (openpyxl) is not written; `--synthetic N` evaluates N seeded synthetic samples
when the dataset is not on the box (without it a missing `filenames_file_eval` is an error); weights are the
deterministic key-addressed set unless `weights/<name>/<selected_epoch>.pt` (the reference's location) exists or
`--weight_path` names a checkpoint in the reference's state_dict layout.  There is no PyTorch fallback for the model,
the ToF simulation or the metrics.
"""
import os
import sys
import time

import torch


def _pop(argv, flag, default=None, cast=str):
    """Take `flag VALUE` out of argv (`cast=None`: a switch without a value -> True)."""
    if flag in argv:
        i = argv.index(flag)
        if cast is None:
            del argv[i]
            return True
        v = cast(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def _intrinsics(v):
    k = tuple(float(x) for x in v.split(","))
    if len(k) != 4:
        raise ValueError(f"--intrinsics takes fx,fy,cx,cy, got '{v}'")
    return k


def _vis_range(v):
    r = tuple(float(x) for x in v.split(","))
    if len(r) != 2 or not r[0] < r[1]:
        raise ValueError(f"--vis_range takes a,b with a < b, got '{v}'")
    return r


def _robust_values(v):
    r = tuple(float(x) for x in v.split(",") if x.strip())
    if not r or any(not x >= 0.0 for x in r) or len({f"{x:g}" for x in r}) != len(r):
        raise ValueError(f"--robust_drop / --robust_sigma take distinct non-negative values a,b,..., got '{v}'")
    return r


ROBUST_SEED = 117010053        # default of --robust_seed: the number the reference seeds everything with (train.py:218)
PICTURE_SWITCHES = ("save_pred", "save_gt", "save_rgb", "save_error_map", "save_for_demo")


def main(argv=None):
    from cfpnet_amd import config, data, geometry, metrics
    from cfpnet_amd.deltar import make_model
    from cfpnet_amd.model_io import load_weights

    argv = list(argv if argv is not None else sys.argv[1:])
    n_syn = _pop(argv, "--synthetic", 0, int)
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f32x3": "f32x3"}[_pop(argv, "--dtype", "f32x3")]
    bs = _pop(argv, "--batch", 8, int)
    unc_metrics = _pop(argv, "--unc_metrics", False, None)
    unc_steps = _pop(argv, "--unc_steps", 20, int)
    want_regions = _pop(argv, "--region_metrics", False, None)
    range_edges = _pop(argv, "--range_edges", (), lambda v: tuple(float(x) for x in v.split(",") if x.strip()))
    save_points = _pop(argv, "--save_points", False, None)
    points_stride = _pop(argv, "--points_stride", None, int)
    points_max_std = _pop(argv, "--points_max_std", None, float)
    points_normals = _pop(argv, "--points_normals", False, None)
    intrinsics = _pop(argv, "--intrinsics", None, _intrinsics)
    normal_metrics = _pop(argv, "--normal_metrics", False, None)
    zone_consistency = _pop(argv, "--zone_consistency", False, None)
    robust = {"drop": _pop(argv, "--robust_drop", (), _robust_values), "sigma": _pop(argv, "--robust_sigma", (), _robust_values)}
    robust_seed = _pop(argv, "--robust_seed", None, int)
    if robust_seed is not None and not (robust["drop"] or robust["sigma"]):
        raise ValueError("--robust_seed needs --robust_drop or --robust_sigma")
    if any(not 0.0 <= v <= 1.0 for v in robust["drop"]):
        raise ValueError("--robust_drop takes fractions in [0, 1]")
    robust_seed = ROBUST_SEED if robust_seed is None else robust_seed
    robust_frames = _pop(argv, "--robust_frames", None, int)
    if robust_frames is not None and robust_frames < 2:
        raise ValueError(f"--robust_frames takes N >= 2, got {robust_frames}")
    if robust_frames is not None and not (robust["drop"] or robust["sigma"]):
        raise ValueError("--robust_frames needs --robust_drop or --robust_sigma")
    if not save_points and (points_stride is not None or points_max_std is not None or points_normals or
                            (intrinsics is not None and not normal_metrics)):
        raise ValueError("--points_stride, --points_max_std, --points_normals and --intrinsics need --save_points"
                         " (--intrinsics also goes with --normal_metrics)")
    vis_cmap = _pop(argv, "--vis_cmap", None)
    vis_range = _pop(argv, "--vis_range", None, _vis_range)
    error_max = _pop(argv, "--error_max", None, float)
    error_rel = _pop(argv, "--error_rel", False, None)
    save_spars = "--save_dir" in argv
    args = config.parse_args(argv) if argv else config.defaults()
    pics = [k for k in PICTURE_SWITCHES if getattr(args, k, False)]
    if not pics and (vis_cmap is not None or vis_range is not None or error_max is not None or error_rel):
        raise ValueError("--vis_cmap, --vis_range, --error_max and --error_rel need one of --" + ", --".join(PICTURE_SWITCHES))
    if pics:
        from cfpnet_amd import render
        vis_cmap = vis_cmap or "magma_r"
        render.colormap_table(vis_cmap)                  # an unknown table is an error before anything is built
        if error_max is not None and not error_max > 0:
            raise ValueError(f"--error_max must be positive, got {error_max}")
        error_max = 1.0 if error_max is None else error_max
    area_in, area_out = bool(getattr(args, "zone_area_only", False)), bool(getattr(args, "outside_zone_area_only", False))
    if area_in and area_out:
        raise ValueError("--zone_area_only and --outside_zone_area_only exclude each other")
    area = metrics.REGIONS.index("fov_in") if area_in else metrics.REGIONS.index("fov_out") if area_out else None
    if range_edges and not want_regions:
        raise ValueError("--range_edges needs --region_metrics")
    if zone_consistency and getattr(args, "random_simu_max_d", False):
        raise ValueError("--zone_consistency re-simulates the zones with the distance the measurement was made with: not with --random_simu_max_d")
    geometry.central_zone_block(str(getattr(args, "zone_type", "8x8")))      # an unknown --zone_type is an error before anything is built
    device = torch.device("cuda:0")
    if n_syn > 0:
        samples = data.SyntheticEvalSamples(n_syn, 480, 640)
    else:
        fn = getattr(args, "filenames_file_eval", None)
        if not fn or not os.path.exists(fn):
            raise FileNotFoundError(f"filenames_file_eval '{fn}' not found -- pass --synthetic N to evaluate synthetic samples")
        samples = data.NYUEvalFiles(args)

    model = make_model(args, dtype=dtype)
    wp = getattr(args, "weight_path", "") or ""
    if not wp and str(getattr(args, "selected_epoch", "-1")) != "-1":
        cand = os.path.join("weights", str(args.name), f"{args.selected_epoch}.pt")
        wp = cand if os.path.exists(cand) else ""
    if wp:
        model = load_weights(model, wp)
    model = model.to(device).eval()
    build = data.EvalInputBuilder(args, device)
    avg = metrics.RunningAverageDict()
    save_unc = bool(getattr(args, "save_entropy", False))
    if save_unc:
        import numpy as np
        os.makedirs(args.save_dir, exist_ok=True)
    spars = metrics.RunningSparsification() if unc_metrics else None
    regions = metrics.RunningRegionAverage(range_edges) if want_regions else None
    normals_avg = metrics.RunningNormalAverage() if normal_metrics else None
    zones_avg = metrics.RunningZoneConsistency() if zone_consistency else None
    if save_points:
        from cfpnet_amd import pointcloud
        os.makedirs(args.save_dir, exist_ok=True)
        rgb_mean = torch.from_numpy(data.IMAGENET_MEAN).to(device)[None, :, None, None]
        rgb_std = torch.from_numpy(data.IMAGENET_STD).to(device)[None, :, None, None]
        n_points = 0
    if pics:
        os.makedirs(args.save_dir, exist_ok=True)
        vmin, vmax = vis_range or (float(args.min_depth), float(args.max_depth))
        n_pics = 0
    want_std = save_points and points_max_std is not None
    robust_runs = [(kind, v, metrics.RunningAverageDict()) for kind in ("drop", "sigma") for v in robust[kind]]
    robust_counts = {(kind, v): torch.zeros(3, dtype=torch.int64, device=device) for kind, v, _ in robust_runs}
    if robust_frames:
        from cfpnet_amd import pointcloud as _pc, temporal
        fused_avg = {(kind, v): metrics.RunningAverageDict() for kind, v, _ in robust_runs}
        fuser = None
    n_batch = 0
    n_img, t0 = 0, time.perf_counter()
    with torch.no_grad():
        for img, dep, names in data.batches(samples, bs):
            inp, gt = build(img, dep)
            if unc_metrics:
                _, pred, _, unc = model(inp, return_uncertainty=True, return_prob=False)
            elif save_unc or want_std:
                _, pred, _, unc = model(inp, return_uncertainty=True)
            else:
                _, pred, _, _ = model(inp)
            if save_unc:
                np.save(os.path.join(args.save_dir, f"unc_{n_img}.npy"), unc.cpu().numpy())
            if unc_metrics:
                spars.update(metrics.sparsification(pred, unc, gt, float(args.min_depth), float(args.max_depth), steps=unc_steps,
                                                    mode=metrics.EVALUATE_ALL))
            if want_regions or area is not None:
                add = inp["additional"]
                rows = metrics.region_metrics(pred, gt, float(args.min_depth), float(args.max_depth), add["rect_data"], add["mask"],
                                              range_edges, mode=metrics.EVALUATE_ALL)
                if want_regions:
                    regions.update(rows)
            if area is not None:
                avg.update(rows[:, area, 0])             # the region's "all depths" row; images without a valid pixel there are skipped
            else:
                avg.update(metrics.eval_metrics(pred, gt, float(args.min_depth), float(args.max_depth), mode=metrics.EVALUATE_ALL))
            if normal_metrics:
                normals_avg.update(*metrics.normal_metrics(pred, gt, float(args.min_depth), float(args.max_depth), intrinsics, hist=True))
            if zone_consistency:
                add = inp["additional"]
                zones_avg.update(*metrics.zone_consistency(pred, build.last_raw, add["rect_data"], add["mask"], float(args.min_depth),
                                                           float(args.max_depth), size=gt.shape[-2:],
                                                           max_distance=float(args.simu_max_distance)))
            if save_points:
                pc = pointcloud.point_cloud(pred, intrinsics or pointcloud.ZJUL5_INTRINSICS, size=gt.shape[-2:], lo=float(args.min_depth),
                                            hi=float(args.max_depth), depth_range=(float(args.min_depth), float(args.max_depth)),
                                            unc=unc if want_std else None, unc_range=(float("-inf"), points_max_std if want_std else float("inf")),
                                            stride=2 if points_stride is None else points_stride, normals=points_normals,
                                            colors=inp["rgb"] * rgb_std + rgb_mean)
                for b, one in enumerate(pc.split()):
                    n_points += pointcloud.write_ply(os.path.join(args.save_dir, f"points_{n_img + b}.ply"), one["points"], one["normals"],
                                                     one["colors"])
            if pics:
                lo, hi, add = float(args.min_depth), float(args.max_depth), inp["additional"]
                todo = []
                if "save_pred" in pics:
                    todo += [("pred_{}.png", render.depth_image(pred, gt.shape[-2:], lo, hi, vmin, vmax, vis_cmap)),
                             ("pred_{}_mm.png", render.depth_u16(pred, gt.shape[-2:], lo, hi))]
                if "save_gt" in pics:
                    todo.append(("gt_{}.png", render.gt_image(gt, lo, hi, vmin, vmax, vis_cmap)))
                if "save_rgb" in pics:
                    todo.append(("rgb_{}.png", render.rgb_image(inp["rgb"])))
                if "save_error_map" in pics:
                    todo.append(("error_{}.png", render.error_image(pred, gt, lo, hi, "rel" if error_rel else "abs", error_max)))
                if "save_for_demo" in pics:
                    todo.append(("demo_{}.png", render.demo_panel(inp["rgb"], pred, add["hist_data"], add["rect_data"], add["mask"], gt, lo, hi,
                                                                  vmin, vmax, vis_cmap, error_kind="rel" if error_rel else "abs",
                                                                  error_max=error_max)))
                for pattern, t in todo:                      # uint8 / uint16 leave the device, never the float32 prediction
                    for b, a in enumerate(t.cpu().numpy()):
                        render.write_png(os.path.join(args.save_dir, pattern.format(n_img + b)), a)
                        n_pics += 1
            for kind, value, r_avg in robust_runs:           # the same images again, one degradation each; step = index of the batch
                deg = dict(drop=value, seed=robust_seed, step=n_batch) if kind == "drop" else \
                    dict(sigma=value, prob=1.0, mean=0.0, seed=robust_seed, step=n_batch)
                r_inp, _ = build(img, dep, degrade=deg)
                if robust_frames:
                    _, r_pred, _, r_unc = model(r_inp, return_uncertainty=True)
                else:
                    _, r_pred, _, _ = model(r_inp)
                if area is not None:
                    r_add = r_inp["additional"]
                    r_avg.update(metrics.region_metrics(r_pred, gt, float(args.min_depth), float(args.max_depth), r_add["rect_data"], r_add["mask"],
                                                        range_edges, mode=metrics.EVALUATE_ALL)[:, area, 0])
                else:
                    r_avg.update(metrics.eval_metrics(r_pred, gt, float(args.min_depth), float(args.max_depth), mode=metrics.EVALUATE_ALL))
                robust_counts[kind, value] = robust_counts[kind, value] + build.last_counts.sum(0)
                if robust_frames:                            # further draws of the same degradation, fused with the identity pose
                    if fuser is None:
                        fuser = temporal.TemporalFilter(intrinsics or _pc.ZJUL5_INTRINSICS, size=gt.shape[-2:], lo=float(args.min_depth),
                                                        hi=float(args.max_depth))
                    fuser.reset()
                    f_pred, _ = fuser.update(r_pred, r_unc)
                    for f in range(1, robust_frames):
                        f_inp, _ = build(img, dep, degrade=dict(deg, step=n_batch + f * 2 ** 20))
                        _, n_pred, _, n_unc = model(f_inp, return_uncertainty=True)
                        f_pred, _ = fuser.update(n_pred, n_unc)
                    if area is not None:
                        fused_avg[kind, value].update(metrics.region_metrics(f_pred, gt, float(args.min_depth), float(args.max_depth),
                                                                             r_add["rect_data"], r_add["mask"], range_edges,
                                                                             mode=metrics.EVALUATE_ALL)[:, area, 0])
                    else:
                        fused_avg[kind, value].update(metrics.eval_metrics(f_pred, gt, float(args.min_depth), float(args.max_depth),
                                                                           mode=metrics.EVALUATE_ALL))
            n_img += img.shape[0]
            n_batch += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = {k: round(v, 3) for k, v in avg.get_value().items()}
    print(f"Metrics: {res}")
    print(",".join(str(v) for v in res.values()))
    if unc_metrics:
        sp = spars.get_value()
        print(f"Uncertainty: { {k: round(v, 4) for k, v in sp.items() if k != 'curves'} }")
        if save_spars:
            import json
            os.makedirs(args.save_dir, exist_ok=True)
            with open(os.path.join(args.save_dir, "sparsification.json"), "w") as f:
                json.dump({"steps": unc_steps, "rankings": list(metrics.RANKINGS), "metrics": list(metrics.SPARS_METRICS),
                           "curves": sp.get("curves", [])}, f)
    if want_regions:
        rv = regions.get_value()
        print(f"Regions: { {r: {q: {k: round(v, 3) for k, v in m.items()} for q, m in t.items()} for r, t in rv.items()} }")
        if save_spars:
            import json
            os.makedirs(args.save_dir, exist_ok=True)
            with open(os.path.join(args.save_dir, "regions.json"), "w") as f:
                json.dump({"regions": list(metrics.REGIONS), "ranges": list(regions.labels), "range_edges": list(range_edges),
                           "metrics": list(metrics.KEYS), "zone_type": str(getattr(args, "zone_type", "8x8")),
                           "table": [[[rv[r][q].get(k) for k in metrics.KEYS] for q in regions.labels] for r in metrics.REGIONS],
                           "images": [[regions.image_counts[r][q] for q in regions.labels] for r in metrics.REGIONS]}, f)
    if normal_metrics:
        nv = normals_avg.get_value()
        print(f"Normals: { {k: (v if k == 'images' else round(v, 3)) for k, v in nv.items()} }")
        if save_spars:
            import json
            os.makedirs(args.save_dir, exist_ok=True)
            with open(os.path.join(args.save_dir, "normals.json"), "w") as f:
                json.dump({"metrics": list(metrics.NORMAL_METRIC_NAMES), "means": [nv.get(k) for k in metrics.NORMAL_METRIC_NAMES],
                           "images": nv.get("images", 0), "bin_deg": 0.1, "histogram": normals_avg.histogram()}, f)
    if zone_consistency:
        zv = zones_avg.get_value()
        print(f"ZoneConsistency: { {k: (v if k == 'images' else round(v, 4)) for k, v in zv.items()} }")
        if save_spars:
            import json
            os.makedirs(args.save_dir, exist_ok=True)
            with open(os.path.join(args.save_dir, "zone_consistency.json"), "w") as f:
                json.dump({"metrics": list(metrics.ZONE_CONSISTENCY_NAMES), "means": [zv.get(k) for k in metrics.ZONE_CONSISTENCY_NAMES],
                           "images": zv.get("images", 0), "max_distance": float(args.simu_max_distance),
                           "zone_columns": list(metrics.ZONE_COLUMNS), "zones": zones_avg.tables()}, f)
    if robust_runs:
        import json
        line = {"drop": {}, "sigma": {}}
        full = {"seed": robust_seed, "images": n_img, "metrics": list(metrics.KEYS), "counts": ["valid", "dropped", "noised"], "drop": {}, "sigma": {}}
        for kind, v, r_avg in robust_runs:
            line[kind][f"{v:g}"] = {k: round(x, 3) for k, x in r_avg.get_value().items()}
            full[kind][f"{v:g}"] = {"metrics": line[kind][f"{v:g}"], "counts": [c / max(n_img, 1) for c in robust_counts[kind, v].cpu().tolist()]}
        if robust_frames:
            line["fused"] = {"frames": robust_frames, "drop": {}, "sigma": {}}
            for kind, v, _ in robust_runs:
                line["fused"][kind][f"{v:g}"] = {k: round(x, 3) for k, x in fused_avg[kind, v].get_value().items()}
            full["fused"] = line["fused"]
        print("Robustness: " + json.dumps(line))
        os.makedirs(args.save_dir, exist_ok=True)
        with open(os.path.join(args.save_dir, "robustness.json"), "w") as f:
            json.dump(full, f)
    if save_points:
        print(f"points: {n_points / max(n_img, 1):.1f} kept per image on average, written to {args.save_dir}/points_<index>.ply", file=sys.stderr)
    if pics:
        print(f"pictures: {n_pics} files written to {args.save_dir}", file=sys.stderr)
    print(f"{n_img} images in {dt:.2f} s ({n_img / dt:.1f} images/s incl. host-side sample generation/decoding)", file=sys.stderr)
    return res


if __name__ == "__main__":
    main()
