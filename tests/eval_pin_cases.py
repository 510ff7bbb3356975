"""The cases of the evaluation pins (tests/golden/eval_pins.npz): every on-device evaluation entry point on seeded inputs, at the sizes at
which the fixed-order reduction of kernels/eval_reduce.h can go wrong.  tests/golden/make_eval_pins.py records what a build returns,
tests/test_eval_pins_gpu.py compares the in-tree build with the record byte for byte; both run ``CASES[name](engine)``.

Sizes: 1 pixel (one block, 255 idle threads), 257 (two blocks, a ragged one), 256 * 1024 + 37 (the grid is capped at 1024 blocks and the
stride loop takes a second, partial round), and 1000 pixels without a valid ground truth.  Every prediction is finite.  A case returns a
dict of arrays; an array of more than MAP_RAW elements travels as the SHA-256 of its bytes."""
import ctypes as C
import functools
import hashlib
import importlib.util
import os

import numpy as np

from camera_fixtures import pointmap_scene
from pcd_fixtures import depth_scene, wavy_grid

_spec = importlib.util.spec_from_file_location("time_depth_disp", os.path.join(os.path.dirname(__file__), "..", "tools", "time_depth_disp.py"))
_tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_tool)
synthetic_clip = _tool.synthetic_clip      # the disparity clip of the timing tool

BIG = 256 * 1024 + 37
SIZES = {"n1": 1, "n257": 257, "big": BIG, "novalid": 1000}
ALIGNMENTS = ("lstsq", "median", "scale", "metric", "l1")
CLIPS = dict(pre_clip_min=0.5, pre_clip_max=5.0, post_clip_min=0.6, post_clip_max=4.0)
DISP_CLIPS = dict(pre_clip_min=0.05, pre_clip_max=1.5, post_clip_min=0.6, post_clip_max=4.0)
MAP_RAW = 300


def _pack(a):
    a = np.ascontiguousarray(a)
    return a if a.size <= MAP_RAW else np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8)


def _out11(res, st):
    from unigeo_amd._lib import Engine
    return np.array([res[k] for k in Engine.DEPTH_KEYS] + [res["valid_pixels"], *st], np.float64)


@functools.lru_cache(maxsize=None)
def depth_input(tag):
    """The generator of the frame-size alignment tests on n pixels: pred = 0.7 gt + 0.3 + noise, 2 % outliers, 5 % invalid gt, a custom mask."""
    n = SIZES[tag]
    rng = np.random.default_rng(100 + n)
    gt = rng.uniform(0.5, 6.0, n).astype(np.float32)
    gt[rng.uniform(size=n) < 0.05] = 0.0
    gt[0] = 1.0
    pred = (0.7 * gt + 0.3 + 0.2 * rng.standard_normal(n)).astype(np.float32)
    out = rng.uniform(size=n) < 0.02
    pred[out] *= rng.uniform(3.0, 10.0, int(out.sum())).astype(np.float32)
    mask = rng.uniform(size=n) > 0.2
    mask[0] = True
    if tag == "novalid":
        gt[:] = 0.0
    return pred, gt, mask


@functools.lru_cache(maxsize=None)
def disp_input(tag):
    pred, gt, mask = synthetic_clip((SIZES[tag],), seed=200 + SIZES[tag])
    if tag == "novalid":
        gt[:] = 0.0
    else:
        gt[0], mask[0] = 1.0, True
    return pred, gt, mask


def radius(depth, K, poses):
    """distance of every back-projected pixel from the world origin, float32 [T,H,W]"""
    T, H, W = depth.shape
    col, row = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
    z, k, p = depth.astype(np.float64), K.astype(np.float64), poses.astype(np.float64)
    x = (col - k[:, None, None, 0, 2]) * z / k[:, None, None, 0, 0]
    y = (row - k[:, None, None, 1, 2]) * z / k[:, None, None, 1, 1]
    world = np.einsum("tij,thwj->thwi", p[:, :3, :3], np.stack([x, y, z], -1)) + p[:, None, None, :3, 3]
    return np.linalg.norm(world, axis=-1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene_input(tag):
    """depth_scene on one row of n pixels (two frames of 500 for the input without valid ground truth) and the ground-truth radius."""
    shape = (2, 20, 25) if tag == "novalid" else (1, 1, SIZES[tag])
    pred, gt, poses, K = depth_scene(shape, 300 + SIZES[tag])
    if tag == "novalid":
        gt[:] = 0.0
    mask = np.random.default_rng(7).uniform(size=shape) > 0.2
    return pred, gt, radius(gt, K, poses), poses, K, mask


@functools.lru_cache(maxsize=None)
def normal_input(tag):
    n = SIZES[tag]
    rng = np.random.default_rng(400 + n)
    gt = rng.standard_normal((n, 3)).astype(np.float32)
    pred = (gt + 0.3 * rng.standard_normal((n, 3))).astype(np.float32)
    mask = rng.uniform(size=n) > 0.2
    mask[0] = True
    if tag == "novalid":
        mask[:] = False
    return pred, gt, mask


def eval_depth(engine, tag):
    """ug_eval_depth: the defaults of Engine.eval_depth"""
    pred, gt, mask = depth_input(tag)
    return {"out11": _out11(*engine.eval_depth(gt, mask, pred=pred))}


def _ex(engine, pred, gt, mask, alignment, max_depth, clips, want_map):
    """ug_eval_depth_ex itself: Engine.eval_depth sends the default options to ug_eval_depth"""
    from unigeo_amd._lib import _depth_opts, _f32, _ptr
    o = _depth_opts(alignment, max_depth, clips)
    m = np.ascontiguousarray(mask.astype(np.uint8))
    out = np.full(11, -1.0, np.float64)
    emap = np.full(gt.shape, -1.0, np.float32) if want_map else None
    rc = engine.lib.ug_eval_depth_ex(engine.ctx, _ptr(_f32(pred)), _ptr(_f32(gt)), _ptr(m), gt.size, C.byref(o), _ptr(out), _ptr(emap))
    assert rc == 0, engine.lib.ug_last_error(engine.ctx).decode()
    return out, emap


def eval_depth_ex(engine, tag, alignment):
    """ug_eval_depth_ex: with and without the four clips, with and without the error map, and once without a depth bound"""
    pred, gt, mask = depth_input(tag)
    got = {}
    for cname, clips in (("noclip", (None,) * 4), ("clip", tuple(CLIPS.values()))):
        for want_map in (False, True):
            out, emap = _ex(engine, pred, gt, mask, alignment, 80.0, clips, want_map)
            got[f"{cname}_map{int(want_map)}_out11"] = out
            if want_map:
                got[f"{cname}_map"] = _pack(emap)
    got["nobound_out11"] = _ex(engine, pred, gt, mask, alignment, None, (None,) * 4, False)[0]
    return got


def eval_depth_ex2(engine, tag):
    """ug_eval_depth_ex2 with UG_DEPTH_ALIGN_DISPARITY: lstsq and l1, with and without disp_clip_min, and once with the four clips"""
    pred, gt, mask = disp_input(tag)
    got = {}
    for alignment in ("lstsq", "l1"):
        for floor in (None, 0.3):
            res, st, emap = engine.eval_depth(gt, mask, pred=pred, alignment=alignment, space="disparity", disp_clip_min=floor, return_error_map=True)
            got[f"{alignment}_floor{floor}_out11"] = _out11(res, st)
            got[f"{alignment}_floor{floor}_map"] = _pack(emap)
    res, st = engine.eval_depth(gt, mask, pred=pred, space="disparity", disp_clip_min=0.3, **DISP_CLIPS)
    got["lstsq_clip_out11"] = _out11(res, st)
    return got


def eval_depth_global(engine, tag):
    """ug_eval_depth_global with the radius map, and with the clips"""
    pred, gt, gr, poses, K, mask = scene_input(tag)
    got = {}
    for cname, clips in (("noclip", {}), ("clip", CLIPS)):
        res, fit_r, fit_d, rmap = engine.eval_depth_global(gt, gr, poses, K, mask, pred=pred, return_radius_map=True, **clips)
        got[f"{cname}_out13"] = np.concatenate([_out11(res, fit_r), np.array(fit_d, np.float64)])
        got[f"{cname}_map"] = _pack(rmap)
    return got


def pcd_world_points(engine, tag):
    pred, gt, _, poses, K, _ = scene_input(tag)
    got = {}
    for cname, clips in (("noclip", {}), ("clip", CLIPS)):
        pts, fit = engine.pcd_world_points(gt, poses, K, pred=pred, **clips)
        got[f"{cname}_fit"] = np.array(fit, np.float32)
        got[f"{cname}_pts"] = _pack(pts)
    return got


def eval_normal(engine, tag):
    pred, gt, mask = normal_input(tag)
    res = engine.eval_normal(gt, mask, pred=pred)
    return {"out8": np.array([res[k] for k in engine.NORMAL_KEYS], np.float64)}


def pointmap(engine):
    """ug_pointmap_focal and ug_pointmap_poses on 2 x 24 x 32"""
    pts, _ = pointmap_scene(2, 24, 32, 30.0, seed=1)
    res = engine.pointmap_poses(pts, 30.0)
    got = {"focal": np.array([engine.pointmap_focal(pts[0])], np.float64), "extrinsics": res["extrinsics"], "depth": _pack(res["depth"]),
           "n_inliers": res["n_inliers"], "iterations": res["iterations"], "reproj_rms": res["reproj_rms"],
           "inliers": _pack(res["inliers"].astype(np.uint8))}
    return got


def eval_pcd_ex(engine, flags):
    """ug_eval_pcd_ex on the masked points of one 24 x 32 frame (about 600), every one of them taken"""
    from unigeo_amd._lib import PcdOptsC, _f32, _ptr
    pred, gt, mask, _ = wavy_grid(1, 24, 32, seed=1, keep=0.78)
    p, g = _f32(pred).reshape(-1, 3), _f32(gt).reshape(-1, 3)
    m = np.ascontiguousarray(mask.reshape(-1).astype(np.uint8))
    ns = int(m.sum())
    assert 550 <= ns <= 650
    out = np.zeros(32, np.float64)
    pc, gc = np.empty((ns, 3), np.float32), np.empty((ns, 3), np.float32)
    o = PcdOptsC(0.1, 30, 30)
    rc = engine.lib.ug_eval_pcd_ex(engine.ctx, _ptr(p), _ptr(g), _ptr(m), m.size, None, 0, C.byref(o), flags, _ptr(out), _ptr(pc), _ptr(gc), None,
                                   None, None)
    assert rc == 0, engine.lib.ug_last_error(engine.ctx).decode()
    return {"out32": out, "pred_cloud": _pack(pc), "gt_cloud": _pack(gc)}


CASES = {}
for _tag in SIZES:
    CASES[f"eval_depth-{_tag}"] = functools.partial(eval_depth, tag=_tag)
    for _a in ALIGNMENTS:
        CASES[f"eval_depth_ex-{_a}-{_tag}"] = functools.partial(eval_depth_ex, tag=_tag, alignment=_a)
    CASES[f"eval_depth_ex2-disparity-{_tag}"] = functools.partial(eval_depth_ex2, tag=_tag)
    CASES[f"eval_depth_global-{_tag}"] = functools.partial(eval_depth_global, tag=_tag)
    CASES[f"pcd_world_points-{_tag}"] = functools.partial(pcd_world_points, tag=_tag)
    CASES[f"eval_normal-{_tag}"] = functools.partial(eval_normal, tag=_tag)
CASES["pointmap-2x24x32"] = pointmap
CASES["eval_pcd_ex-brute"] = functools.partial(eval_pcd_ex, flags=0)
CASES["eval_pcd_ex-grid"] = functools.partial(eval_pcd_ex, flags=2)      # UG_PCD_SEARCH_GRID
