"""The evaluation loop - mirrors ``/root/reference/eval.py:10-99`` and ``configs/config_utils.py:3-35``.

Differences kept deliberately small: the YAML path is an argument instead of being hard-coded (eval.py:11) and
dataset / model classes can be passed as objects.  ``vis_depth: True`` writes the reference's
depth / normal panels (eval.py:58-62; ``harness/vis.py``).  ``eval_pcd`` (eval.py:66-83) scores
the model's world points, or those of its aligned depth, against the ground-truth cloud.
``eval_camera`` (eval.py:85-95) scores the model's camera poses, or those recovered from its world points, with ATE and
RPE (``harness/camera.py``, ``harness/pointmap.py``); the DepthCrafter / StableNormal plugins return
neither, so a configuration that asks them for it is an error at the first clip.  ``eval_temporal`` (not a key of the reference) scores
the aligned depth's temporal alignment error between neighbouring frames (``harness/temporal.py``).
"""
import importlib
import os

import numpy as np

from .camera import CAMERA_KEYS, camera_pose_evaluation, save_camera_trajectories
from .io_utils import prepare_gt_label
from .normals import NORMALS_MODES
from .pointmap import poses_from_pointmap
from .temporal import temporal_alignment_error
from .vis import save_depth_normal_maps, write_ply
from .metrics import (DEPTH_ALIGNMENTS, DEPTH_ALIGN_SPACES, PCD_KEYS, PCD_MAX_THRESHOLDS, PCD_MAX_VOXEL_SIZES, MetricsManager, check_disp_clip_min, depth_evaluation, depth_evaluation_in_global_coord, normal_evaluation,
                      pcd_evaluation, pcd_score_names, world_points_from_depth)


def import_class_from_module(module_name, class_name):
    return getattr(importlib.import_module(module_name), class_name)


def parse_dataset_config(config):
    out = {"root": config["root"], "clip_length": config.get("clip_length", 30),
           "clip_overlap": config.get("clip_overlap", 0), "input_size": (config["h"], config["w"]),
           "target_size": (config["h"], config["w"])}
    for k in ("split", "split_file", "scenes",       # optional: which scene list the loader walks (default: the split file)
              "prep",                                # optional: host | device clip preparation of the ScanNet++ / RGB-D loaders (DESIGN.md sections 16, 17)
              "register", "register_invalid",        # optional, 7-Scenes: host | device registration of raw depth, keep | drop of its 65535 marker (section 22)
              "normals", "normals_radius", "normals_edge", "normals_min_count"):   # optional, RGB-D loaders: normals fitted to the depth (section 30)
        if k in config:
            out[k] = config[k]
    if out.get("normals") not in NORMALS_MODES:
        raise ValueError(f"normals must be 'depth' or absent, not {out['normals']!r}")
    return out


def parse_metric_config(config):
    names = []
    for key in ("eval_depth", "eval_pcd", "eval_camera", "eval_normal", "eval_temporal"):
        if key in config:
            names.extend(config[key]["metric_names"])
    return names


def parse_depth_eval_config(config):
    """``eval_depth.depth_alignment`` (lstsq | median | scale | metric | l1, default lstsq), optional ``max_depth`` and the four clip keys ->
    (alignment, max_depth, clips).  An unknown alignment is a ``ValueError``."""
    cfg = config.get("eval_depth") or {}
    alignment = cfg.get("depth_alignment", "lstsq")
    if alignment not in DEPTH_ALIGNMENTS:
        raise ValueError(f"eval_depth.depth_alignment must be one of {list(DEPTH_ALIGNMENTS)}, not {alignment!r}")
    clips = {k: cfg[k] for k in ("pre_clip_min", "pre_clip_max", "post_clip_min", "post_clip_max") if cfg.get(k) is not None}
    return alignment, cfg.get("max_depth", 80), clips


def parse_depth_space_config(config):
    """``eval_depth.space``: ``depth`` (default: the prediction is a depth and is aligned against the ground-truth depth) or ``disparity`` (the
    prediction is a disparity: it is aligned against ``1 / gt``, inverted, and scored against the depth), and
    ``eval_depth.disp_clip_min`` (optional, disparity only: a floor under the aligned disparity before it is inverted) ->
    ``(space, disp_clip_min)``.  An unknown space, a floor that is not a finite positive number, a floor with ``space: depth``, and
    ``space: disparity`` together with ``coord: global`` are a ``ValueError``."""
    cfg = config.get("eval_depth") or {}
    space = cfg.get("space", "depth")
    if space not in DEPTH_ALIGN_SPACES:
        raise ValueError(f"eval_depth.space must be one of {list(DEPTH_ALIGN_SPACES)}, not {space!r}")
    floor = cfg.get("disp_clip_min")
    check_disp_clip_min(space, floor, "eval_depth.disp_clip_min")
    if space == "disparity" and cfg.get("coord", "camera") == "global":
        raise ValueError("eval_depth.space: disparity does not go with coord: global (the world-frame evaluation aligns the depth itself)")
    return space, (None if floor is None else float(floor))


DEPTH_COORDS = ("camera", "global")


def parse_depth_coord(config):
    """``eval_depth.coord``: ``camera`` (default: the metrics on the depth itself) or ``global`` (the aligned depth moved into the world
    frame and evaluated as distance from the world origin, ``depth_evaluation_in_global_coord``; least squares only).  An unknown value,
    or ``global`` with another ``depth_alignment``, is a ``ValueError``."""
    cfg = config.get("eval_depth") or {}
    coord = cfg.get("coord", "camera")
    if coord not in DEPTH_COORDS:
        raise ValueError(f"eval_depth.coord must be one of {list(DEPTH_COORDS)}, not {coord!r}")
    alignment = cfg.get("depth_alignment", "lstsq")
    if coord == "global" and alignment != "lstsq":
        raise ValueError(f"eval_depth.coord: global aligns with least squares only (depth_alignment: lstsq), not {alignment!r}")
    return coord


def parse_pcd_eval_config(config):
    """``eval_pcd`` (the reference's key, eval.py:66-83): ``pcd_downsample_num`` (default -1: every masked point), optional ``threshold``
    (ICP correspondence distance, default 0.1) and ``seed`` (default 0; a clip draws with ``seed + data index``) -> dict, or ``None`` without
    the key.  ``sampling`` is ``random`` (default: the seeded draw) or ``fps`` (farthest-point sampling; ``seed`` is not
    used).  ``search`` is ``brute`` (default) or ``grid`` (the exact search through a uniform grid, DESIGN.md section 20: the same numbers, and the
    one way to run ``pcd_downsample_num: -1`` on a full clip).  Optional ``fscore_thresholds`` (at most 8) and ``voxel_sizes`` (at most 4), lists
    of positive finite numbers, add ``prec@t`` / ``recall@t`` / ``fscore@t`` and ``iou@v`` to every row; the number in a
    key is ``format(x, "g")`` and no two entries may be written the same way.  Anything else, and ``vis_pcd`` without ``eval_pcd``, is a
    ``ValueError``."""
    if "eval_pcd" not in config:
        if config.get("vis_pcd"):
            raise ValueError("vis_pcd needs eval_pcd: the point clouds it writes are the ones eval_pcd aligns")
        return None
    cfg = config["eval_pcd"] or {}
    sampling = cfg.get("sampling", "random")
    if sampling not in ("random", "fps"):
        raise ValueError(f"eval_pcd.sampling must be 'random' or 'fps', not {sampling!r}")
    search = cfg.get("search", "brute")
    if search not in ("brute", "grid"):
        raise ValueError(f"eval_pcd.search must be 'brute' or 'grid', not {search!r}")
    res = {"downsample_num": int(cfg.get("pcd_downsample_num", -1)), "threshold": float(cfg.get("threshold", 0.1)), "seed": int(cfg.get("seed", 0)),
           "sampling": sampling, "search": search}
    for key, limit in (("fscore_thresholds", PCD_MAX_THRESHOLDS), ("voxel_sizes", PCD_MAX_VOXEL_SIZES)):      # absent: the dict is what it was
        if key in cfg:
            res[key] = pcd_score_names(cfg[key], f"eval_pcd.{key}", limit)[0]
    return res


CAMERA_EVAL_KEYS = ("metric_names", "reproj_px", "focal")


def parse_camera_eval_config(config):
    """``eval_camera`` (the reference's key, eval.py:85-95): optional ``reproj_px`` (the trim threshold of the pose recovery from point maps,
    default 8.0) and ``focal`` (given: the focal step is skipped) -> dict, or ``None`` without the key.  An unknown key, a value that is not a
    positive number, and ``vis_camera`` without ``eval_camera`` are a ``ValueError``."""
    if "eval_camera" not in config:
        if config.get("vis_camera"):
            raise ValueError("vis_camera needs eval_camera: the trajectories it writes are the ones eval_camera scores")
        return None
    cfg = config["eval_camera"] or {}
    unknown = sorted(set(cfg) - set(CAMERA_EVAL_KEYS))
    if unknown:
        raise ValueError(f"eval_camera: unknown key(s) {unknown}; known: {list(CAMERA_EVAL_KEYS)}")
    out = {"reproj_px": float(cfg.get("reproj_px", 8.0)), "focal": None if cfg.get("focal") is None else float(cfg["focal"])}
    if not out["reproj_px"] > 0 or (out["focal"] is not None and not out["focal"] > 0):
        raise ValueError("eval_camera: reproj_px and focal must be positive")
    return out


TEMPORAL_EVAL_KEYS = ("metric_names", "stride")
TEMPORAL_METRICS = ("TAE", "TAE gt")


def parse_temporal_eval_config(config):
    """``eval_temporal`` (not a key of the reference: the temporal alignment error of ``harness/temporal.py``):
    ``metric_names`` out of ``TAE`` (the clip's aligned prediction) and ``TAE gt`` (the ground-truth depth itself under the same poses: the
    floor the dataset allows), optional ``stride`` (default 1: consecutive frames) -> dict, or ``None`` without the key.  An unknown key, an
    unknown metric name, a stride that is not a positive integer, ``eval_temporal`` without ``eval_depth`` (whose ``(s, t)`` it aligns with)
    and ``eval_temporal`` with ``eval_depth.coord: global`` are a ``ValueError``."""
    if "eval_temporal" not in config:
        return None
    cfg = config["eval_temporal"] or {}
    unknown = sorted(set(cfg) - set(TEMPORAL_EVAL_KEYS))
    if unknown:
        raise ValueError(f"eval_temporal: unknown key(s) {unknown}; known: {list(TEMPORAL_EVAL_KEYS)}")
    names = list(cfg.get("metric_names") or [])
    bad = [n for n in names if n not in TEMPORAL_METRICS]
    if bad:
        raise ValueError(f"eval_temporal.metric_names: unknown name(s) {bad}; known: {list(TEMPORAL_METRICS)}")
    stride = cfg.get("stride", 1)
    if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or stride < 1:
        raise ValueError(f"eval_temporal.stride must be a positive integer, not {stride!r}")
    if "eval_depth" not in config:
        raise ValueError("eval_temporal needs eval_depth: it scores the depth aligned with that evaluation's scale and shift")
    if (config["eval_depth"] or {}).get("coord", "camera") == "global":
        raise ValueError("eval_temporal does not go with eval_depth.coord: global (its scale and shift belong to the camera-frame evaluation)")
    return {"stride": int(stride), "gt": "TAE gt" in names}


def evaluate(config, dataset=None, model=None, save_dir="./debug_output", rank=0, world=1, verbose=True,
             device_metrics=False, models=None, engine=None):
    """Run the reference's per-clip loop.  With ``world > 1`` this rank only evaluates clips
    ``rank, rank+world, ...`` (clips are independent samples); rows are merged by the caller.
    ``device_metrics=True`` evaluates depth / normal metrics on the GPU against the outputs still resident in HBM
    (``ug_eval_depth`` / ``ug_eval_normal``) instead of on the host copies.
    ``models`` = several instances of the plugin on ONE GPU (round 5): this rank's k-th clip runs on ``models[k % len(models)]``, each instance on its own host
    thread - independent clips in flight on one GPU, the sharding over GPUs one level down (+10 % aggregate frames/s with two DepthCrafter contexts: a second
    clip fills the CUs that one clip's tile tails and under-filled launches leave idle).  Rows / CSV come out in dataset order, identical to the serial loop.
    ``eval_depth.depth_alignment`` (lstsq | median | scale | metric | l1, default lstsq), ``eval_depth.max_depth`` and the four ``eval_depth.*_clip_*`` keys select
    the alignment of the depth metrics on both the host and the device path; an unknown value raises ``ValueError`` before the first clip runs.  A deliberate
    difference: the reference reads ``depth_alignment`` (eval.py:48) and always aligns with least squares.
    ``eval_depth.coord: global`` (default ``camera``) evaluates the depth in world coordinates instead: the radius
    ``|gt_world_pts|``, the poses of ``prepare_gt_label`` and the sample's intrinsics go to ``depth_evaluation_in_global_coord`` on the host and to
    ``ug_eval_depth_global`` on the device path; the row keys stay the same.  It goes with ``depth_alignment: lstsq`` only (``ValueError`` otherwise).
    ``eval_depth.space: disparity`` (default ``depth``) aligns in disparity space, the protocol of the published video-depth
    numbers: the model's ``pred_disps`` on the host path (``depth_evaluation(align_space="disparity")``; a model that returns none raises a
    ``ValueError`` at its first clip that names the clip, the plugin and ``return_disparity``), the resident disparity of the last run under
    ``device_metrics=True`` (``ug_eval_depth_ex2``; the plugin needs no option).  ``eval_depth.disp_clip_min`` floors the aligned disparity.
    Not with ``coord: global``; ``eval_pcd``'s world points keep coming from the least-squares-aligned depth.
    ``vis_depth: True`` (the reference's key, eval.py:58-62) writes ``save_dir/depth_{seq}/frame_%04d.webp`` after the clip's metrics: rgb | normals |
    coloured depth | colour bar, composed on the GPU from the resident outputs under ``device_metrics=True`` and by the numpy mirror otherwise
    (DESIGN.md section 15).  Rows and CSV do not change.
    ``eval_normal`` on a dataset without ground-truth normals (the RGB-D loaders of ``harness/rgbd.py``) raises ``ValueError`` at the first such clip,
    before the model runs on it.  ``normals: depth`` in the dataset keys (with ``normals_radius`` / ``normals_edge`` / ``normals_min_count``;
    DESIGN.md section 30) makes those loaders fit normals to their depth; the normal metrics then use ``gt_normal_masks`` (``mask`` and the fit's
    ``normal_mask``) on the host and on the device path, every other metric keeps ``gt_masks``.
    ``eval_pcd`` (eval.py:66-83) adds ``acc / comp / nc1 / nc2`` and their medians: the model's ``pred_world_pts`` when it
    returns them, else ``world_points_from_depth`` of its depth with ``eval_depth``'s ``max_depth`` and clips (on the resident depth under
    ``device_metrics=True``), against ``gt_world_pts`` on ``gt_masks`` through ``pcd_evaluation`` / ``ug_eval_pcd``
    (``sampling: fps``: farthest-point sampling of each cloud, ``ug_eval_pcd_fps``).  ``vis_pcd: True`` writes
    ``save_dir/pcd_{seq}/pred.ply`` and ``gt.ply`` (the aligned clouds before ICP).  ``vis_pcd`` without ``eval_pcd``, or a clip without
    ``intrinsics`` when the points have to come from the depth, raises ``ValueError`` before the first clip runs.
    ``eval_camera`` (eval.py:85-95) adds ``ATE / RPE trans / RPE rot`` through ``camera_pose_evaluation``
    (``harness/camera.py``): of the model's ``pred_poses`` when it returns them; else of the poses recovered from its ``pred_world_pts``
    (``harness/pointmap.py``; on the device through ``ug_pointmap_focal`` / ``ug_pointmap_poses`` under ``device_metrics=True``, with the
    model's own engine or with ``engine=`` for a model that has none); a model that returns neither raises a ``ValueError`` that names the
    clip and the plugin.  Optional keys ``eval_camera.reproj_px`` and ``eval_camera.focal``; an unknown key raises before the first clip.
    ``vis_camera: True`` writes ``save_dir/camera_{seq}/pred_traj.txt``, ``gt_traj.txt`` (TUM format) and, with matplotlib, ``traj.png``;
    without ``eval_camera`` it is a ``ValueError``.  A configuration without ``eval_camera`` gives the rows and bytes it gave before.
    ``eval_temporal`` (not in the reference) adds ``TAE``, the temporal alignment error of the clip's depth aligned with
    the ``(s, t)``, space, post-clips and ``max_depth`` of that clip's ``eval_depth``: ``temporal_alignment_error`` on the host,
    ``ug_eval_tae`` on the resident depth (or disparity) under ``device_metrics=True``.  ``TAE gt``, by name only, scores the ground-truth
    depth itself.  The row also carries ``TAE pairs`` / ``TAE pairs total`` / ``TAE pixels``; frames that pad a clip's tail are scored like
    any other.  Needs ``eval_depth`` in camera coordinates and a sample with ``intrinsics`` (``ValueError`` otherwise); optional ``stride``."""
    alignment, max_depth, clips = parse_depth_eval_config(config)
    coord = parse_depth_coord(config)
    space, disp_clip_min = parse_depth_space_config(config)
    space_kw = {} if space == "depth" else {"disp_clip_min": disp_clip_min}
    pcd_cfg = parse_pcd_eval_config(config)
    cam_cfg = parse_camera_eval_config(config)
    tae_cfg = parse_temporal_eval_config(config)
    host_mode = {"lstsq": {"align_with_lstsq": True}, "median": {}, "scale": {"align_with_scale": True}, "metric": {"metric_scale": True},
                 "l1": {"align_with_l1": True}}[alignment]
    if dataset is None:
        dataset = import_class_from_module("unigeo_amd.harness", config["dataset"])(**parse_dataset_config(config))
    if model is None and not models:
        model = import_class_from_module("unigeo_amd.model", config["model_name"])(**config["model_params"])
    mm = MetricsManager(metric_names=parse_metric_config(config))
    os.makedirs(save_dir, exist_ok=True)
    save_path = os.path.join(save_dir, "metrics.csv")
    def one_clip(data_idx, mdl):
        data = dataset[data_idx]
        seq = f"{data_idx:03d}_{data['scene_name']}"
        if "eval_normal" in config and "cam_normal" not in data:
            raise ValueError(f"eval_normal: clip {seq} of dataset {data.get('_dataset', type(dataset).__name__)!r} has no ground-truth normals "
                             f"(the sample lacks 'cam_normal'); remove eval_normal from the configuration, or set normals: depth on an RGB-D "
                             f"dataset to fit them from its depth")
        if pcd_cfg is not None and "intrinsics" not in data and not getattr(mdl, "predicts_world_points", False):
            raise ValueError(f"eval_pcd: clip {seq} has no 'intrinsics' to turn the predicted depth into world points")
        if tae_cfg is not None and "intrinsics" not in data:
            raise ValueError(f"eval_temporal: clip {seq} has no 'intrinsics' to carry a frame's depth into its neighbour's camera")
        if verbose:
            print("processing seq:", seq)
        output = mdl.forward(data)
        gt = prepare_gt_label(data)
        metric = {"seq_name": seq}
        eng = getattr(getattr(mdl, "pipeline", None), "engine", None) if device_metrics else None
        if "eval_depth" in config and coord == "global":
            gt_radius = np.linalg.norm(gt["gt_world_pts"].numpy().astype(np.float64), axis=-1).astype(np.float32)      # one rounding
            K = np.stack([np.asarray(k, dtype=np.float32).reshape(3, 3) for k in data["intrinsics"]], 0)
            poses = gt["gt_poses"].numpy()
            if eng is not None:
                res = eng.eval_depth_global(gt["gt_depths"].numpy(), gt_radius, poses, K, gt["gt_masks"].numpy(), max_depth=max_depth, **clips)
            else:
                res = depth_evaluation_in_global_coord(output["pred_depths"], gt["gt_depths"], gt_radius, poses, K, max_depth=max_depth,
                                                       custom_mask=gt["gt_masks"], align_with_lstsq=True, **clips)
            metric.update(res[0])
        elif "eval_depth" in config and space == "disparity":
            if eng is not None:
                res = eng.eval_depth(gt["gt_depths"].numpy(), gt["gt_masks"].numpy(), max_depth=max_depth, alignment=alignment, space="disparity",
                                     **space_kw, **clips)
            else:
                if output.get("pred_disps") is None:
                    raise ValueError(f"eval_depth.space: disparity: clip {seq}: the model {type(mdl).__name__!r} returns no 'pred_disps'; "
                                     f"construct it with return_disparity=True (model_params), or evaluate with space: depth")
                res = depth_evaluation(output["pred_disps"], gt["gt_depths"], max_depth=max_depth, custom_mask=gt["gt_masks"],
                                       align_space="disparity", **space_kw, **host_mode, **clips)
            metric.update(res[0])
        elif "eval_depth" in config:
            if eng is not None:
                res = eng.eval_depth(gt["gt_depths"].numpy(), gt["gt_masks"].numpy(), max_depth=max_depth, alignment=alignment, **clips)
            else:
                res = depth_evaluation(output["pred_depths"], gt["gt_depths"], max_depth=max_depth, custom_mask=gt["gt_masks"], **host_mode, **clips)
            metric.update(res[0])
        if tae_cfg is not None:
            K = np.stack([np.asarray(k, dtype=np.float32).reshape(3, 3) for k in data["intrinsics"]], 0)
            gt_d, poses, cm = gt["gt_depths"].numpy(), gt["gt_poses"].numpy(), gt["gt_masks"].numpy()
            kw = {"max_depth": max_depth, "stride": tae_cfg["stride"]}
            pkw = {"space": space, **space_kw, **{k: v for k, v in clips.items() if k.startswith("post_")}}
            fit = (np.float32(res[1][0]), np.float32(res[1][1]))      # the (s, t) of this clip's eval_depth
            if eng is not None:
                tae = eng.eval_tae(gt_d, poses, K, fit, cm, **kw, **pkw)
            else:
                tae = temporal_alignment_error(output["pred_disps" if space == "disparity" else "pred_depths"], gt_d, poses, K, fit,
                                               custom_mask=cm, **kw, **pkw)
            metric.update(tae)
            if tae_cfg["gt"]:
                if eng is not None:
                    metric["TAE gt"] = eng.eval_tae(gt_d, poses, K, (1.0, 0.0), cm, pred=gt_d, **kw)["TAE"]
                else:
                    metric["TAE gt"] = temporal_alignment_error(gt_d, gt_d, poses, K, (1.0, 0.0), custom_mask=cm, **kw)["TAE"]
        if "eval_normal" in config:
            nmask = gt.get("gt_normal_masks", gt["gt_masks"])      # fitted normals bring their own validity (normals: depth)
            if eng is not None:
                metric.update(eng.eval_normal(gt["gt_normals"].numpy(), nmask.numpy()))
            else:
                metric.update(normal_evaluation(output["pred_normals"], gt["gt_normals"], custom_mask=nmask))
        if pcd_cfg is not None:
            kw = {"threshold": pcd_cfg["threshold"], "downsample_num": pcd_cfg["downsample_num"], "seed": pcd_cfg["seed"] + data_idx,
                  "sampling": pcd_cfg["sampling"], "search": pcd_cfg["search"]}
            kw.update({k: pcd_cfg[k] for k in ("fscore_thresholds", "voxel_sizes") if k in pcd_cfg})
            pts = output.get("pred_world_pts")
            if hasattr(pts, "detach"):
                pts = pts.detach().cpu().numpy()
            if pts is None:
                K = np.stack([np.asarray(k, dtype=np.float32).reshape(3, 3) for k in data["intrinsics"]], 0)
                if eng is not None:        # the points are made from the resident depth and stay on the device
                    eng.pcd_world_points(gt["gt_depths"].numpy(), gt["gt_poses"].numpy(), K, max_depth=max_depth, return_points=False, **clips)
                else:
                    pts = world_points_from_depth(output["pred_depths"], gt["gt_depths"], gt["gt_poses"], K, max_depth=max_depth, **clips)[0]
            if eng is not None:
                res = eng.eval_pcd(pts, gt["gt_world_pts"].numpy(), gt["gt_masks"].numpy(), gt["gt_rgbs"].numpy(), **kw)
            else:
                res = pcd_evaluation(pts, gt["gt_world_pts"], gt["gt_masks"], gt["gt_rgbs"], **kw)
            metric.update({k: res[k] for k in PCD_KEYS})
            metric.update({k: v for k, v in res.items() if "@" in k})      # prec@t, recall@t, fscore@t, iou@v
            if config.get("vis_pcd"):
                pcd_dir = os.path.join(save_dir, f"pcd_{seq}")
                os.makedirs(pcd_dir, exist_ok=True)
                write_ply(os.path.join(pcd_dir, "pred.ply"), *res["pred_pcd"])
                write_ply(os.path.join(pcd_dir, "gt.ply"), *res["gt_pcd"])
        if cam_cfg is not None:
            poses = output.get("pred_poses")
            if poses is None and output.get("pred_world_pts") is not None:
                pm_eng = eng if eng is not None else (engine if device_metrics else None)
                poses = poses_from_pointmap(output["pred_world_pts"], focal=cam_cfg["focal"], reproj_px=cam_cfg["reproj_px"], engine=pm_eng)[0]
            if poses is None:
                raise ValueError(f"eval_camera: clip {seq}: the model {type(mdl).__name__!r} returns neither 'pred_poses' nor 'pred_world_pts'; "
                                 f"remove eval_camera from the configuration")
            metric.update(zip(CAMERA_KEYS, camera_pose_evaluation(poses, gt["gt_poses"])))
            if config.get("vis_camera"):
                save_camera_trajectories(poses, gt["gt_poses"], os.path.join(save_dir, f"camera_{seq}"))
        if config.get("vis_depth"):
            vis_dir = os.path.join(save_dir, f"depth_{seq}")
            os.makedirs(vis_dir, exist_ok=True)
            if eng is not None:          # depth and normals are still resident: only the bytes of the panels come back
                save_depth_normal_maps(None, None, vis_dir, rgbs=gt["gt_rgbs"], engine=eng)
            else:
                save_depth_normal_maps(output["pred_depths"], output["pred_normals"], vis_dir, rgbs=gt["gt_rgbs"])
        return metric

    mine = list(range(rank, len(dataset), world))
    rows = []
    if models and len(models) > 1:
        import threading
        out, errs = [None] * len(mine), []

        def worker(j):
            try:
                for k in range(j, len(mine), len(models)):
                    out[k] = one_clip(mine[k], models[j])
            except Exception as ex:
                errs.append(ex)
        th = [threading.Thread(target=worker, args=(j,)) for j in range(len(models))]
        [t.start() for t in th]; [t.join() for t in th]
        if errs:
            raise errs[0]
        for metric in out:                     # dataset order, as the serial loop writes them
            rows.append(metric)
            mm.update_metrics(metric)
        mm.export_to_csv(save_path)
        return rows, mm
    for data_idx in mine:
        metric = one_clip(data_idx, models[0] if models else model)
        rows.append(metric)
        mm.update_metrics(metric)
        mm.export_to_csv(save_path)
    return rows, mm
