#!/usr/bin/env python
"""Golden vectors for depth evaluation in global coordinates, made like make_depth_alignment_golden.py: the
REFERENCE's own ``metrics/eval_depth.py`` (``depth_evaluation_in_global_coord``, lines 250-441) is imported by path from /root/reference
(read-only; ``cv2`` and ``tqdm`` stubbed, ``utils/geometry_utils.py`` registered as the top-level module ``geometry_utils`` it imports) and
run on seeded synthetic inputs.  Writes tests/golden/depth_global_golden.npz - data only; the other fixtures keep their bytes.

Input at 3 x 20 x 28 (non-square: a swapped row / column shows): a float32 prediction with some negative values, a ground-truth depth
with zeros and one 90, a custom mask, a DIFFERENT K and a DIFFERENT rotated and translated camera-to-world pose per frame (a wrong frame
index or a transposed R changes the answer), ground-truth radius = the same geometry applied to the ground-truth depth, at least 0.3 on
every valid pixel (the reference divides by it without a guard).  Two cases: no clips, and (pre_min, pre_max, post_min, post_max) =
(1.0, 4.0, 0.8, 5.0).  Stored per case: the reference's result dict and its radius map.

Also computed here, stored and printed: an emulation of the DEVICE's arithmetic on the CPU - both least-squares fits as float64 normal
equations solved by the determinant formula, (s, t) cast to float32, everything else as the reference does it - its (s, t) pairs, where its
radius map equals the reference's bit for bit, and its largest relative distance from the reference: ``metric_distance`` over the eight
metrics and ``map_distance`` over the radius map.  tests/test_depth_global_*.py bound the code under test by twice these distances.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

for name in ["cv2", "tqdm"]:
    if name not in sys.modules:
        try:
            __import__(name)
        except Exception:
            m = types.ModuleType(name)
            m.__path__ = []
            m.tqdm = lambda x, *a, **k: x
            sys.modules[name] = m


def load_by_path(modname, relpath):
    spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


align = load_by_path("metrics.alignment", "metrics/alignment.py")
sys.modules.setdefault("metrics", types.ModuleType("metrics")).__path__ = [os.path.join(REF, "metrics")]
sys.modules["metrics.alignment"] = align
sys.modules["geometry_utils"] = load_by_path("geometry_utils", "utils/geometry_utils.py")
ev_depth = load_by_path("metrics.eval_depth", "metrics/eval_depth.py")

CLIPS = {"pre_clip_min": 1.0, "pre_clip_max": 4.0, "post_clip_min": 0.8, "post_clip_max": 5.0}
KEYS = ["Abs Rel", "Sq Rel", "RMSE", "Log RMSE", "delta < 1.", "delta < 1.25", "delta < 1.25^2", "delta < 1.25^3", "valid_pixels"]
f32, f64 = np.float32, np.float64

rng = np.random.default_rng(20261018)
Nf, h, w = 3, 20, 28


def rotation(axis, angle):
    a = np.asarray(axis, f64); a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def radius_f64(depth, K, poses):
    """|R p + t| of the back-projected depth, float64 from the float32 inputs, [Nf,h,w]"""
    col, row = np.meshgrid(np.arange(w), np.arange(h), indexing="xy")
    out = np.empty(depth.shape, f64)
    for i in range(Nf):
        z = depth[i].astype(f64)
        x = (col - f64(K[i, 0, 2])) * z / f64(K[i, 0, 0])
        y = (row - f64(K[i, 1, 2])) * z / f64(K[i, 1, 1])
        R, t = poses[i, :3, :3].astype(f64), poses[i, :3, 3].astype(f64)
        wx = R[0, 0] * x + R[0, 1] * y + R[0, 2] * z + t[0]
        wy = R[1, 0] * x + R[1, 1] * y + R[1, 2] * z + t[1]
        wz = R[2, 0] * x + R[2, 1] * y + R[2, 2] * z + t[2]
        out[i] = np.sqrt(wx * wx + wy * wy + wz * wz)
    return out


def normal_equations(p, g):
    """(s, t) as the device gets them: float64 sums n, sum p, sum p^2, sum g, sum p g and the determinant formula, cast to float32"""
    p, g = p.astype(f64), g.astype(f64)
    a = [float(p.size), p.sum(), (p * p).sum(), g.sum(), (p * g).sum()]
    det = a[2] * a[0] - a[1] * a[1]
    assert a[0] >= 2 and abs(det) > 1e-12 * max(1.0, a[2] * a[0])          # the regular branch; the degenerate ones are not part of this fixture
    return f32((a[4] * a[0] - a[1] * a[3]) / det), f32((a[2] * a[3] - a[1] * a[4]) / det)


def metrics_f32(p, g):
    """the reference's metric expressions (eval_depth.py:384-408) on float32 torch tensors"""
    p, g = torch.from_numpy(p), torch.from_numpy(g)
    out = [torch.mean(torch.abs(p - g) / g).item(), torch.mean(((p - g) ** 2) / g).item(), torch.sqrt(torch.mean((p - g) ** 2)).item()]
    p = torch.clamp(p, min=1e-5)
    out.append(torch.sqrt(torch.mean((torch.log(p) - torch.log(g)) ** 2)).item())
    ratio = torch.maximum(p / g, g / p)
    return out + [torch.mean((ratio < k).float()).item() for k in (1.0, 1.25, 1.25 ** 2, 1.25 ** 3)]


def emulate_device(pred, gt, gr, poses, K, mask, clips):
    m1 = (gt > 0) & (gt < 80)
    p = pred[m1]
    if clips:
        p = np.minimum(np.maximum(p, f32(clips["pre_clip_min"])), f32(clips["pre_clip_max"]))
    s_d, t_d = normal_equations(p, gt[m1])
    d = s_d * pred + t_d                                                  # float32, two roundings
    if clips:
        d = np.minimum(np.maximum(d, f32(clips["post_clip_min"])), f32(clips["post_clip_max"]))
    r = radius_f64(d, K, poses).astype(f32)
    s_r, t_r = normal_equations(r[m1], gr[m1])
    rmap = s_r * r + t_r
    sel = m1 & mask
    return metrics_f32(rmap[sel], gr[sel]), rmap, (s_r, t_r), (s_d, t_d)


gt = rng.uniform(0.5, 6.0, (Nf, h, w)).astype(f32)
gt[0, :3] = 0.0; gt[1, 5, 5] = 90.0
pred = (0.7 * gt + 0.3 + 0.2 * rng.standard_normal(gt.shape)).astype(f32)
pred *= (1.0 + 0.15 * np.arange(Nf, dtype=f32))[:, None, None]          # bent per frame: global and camera coordinates disagree
neg = rng.uniform(size=gt.shape) < 0.03
pred[neg] = -pred[neg]
mask = rng.uniform(size=gt.shape) > 0.2
K = np.stack([np.array([[30.0 + 3.0 * k, 0, 13.5 + 0.7 * k], [0, 27.0 + 2.0 * k, 9.5 - 0.4 * k], [0, 0, 1]], f32) for k in range(Nf)], 0)
poses = np.tile(np.eye(4, dtype=f32), (Nf, 1, 1))
for k, (axis, angle, t) in enumerate([((0.2, 1.0, 0.1), 0.35, (1.0, -0.8, 1.5)), ((1.0, -0.3, 0.4), -0.5, (-0.6, 1.2, 2.0)),
                                      ((-0.4, 0.5, 1.0), 0.8, (0.3, 0.7, -2.6))]):
    poses[k, :3, :3] = rotation(axis, angle).astype(f32)
    poses[k, :3, 3] = np.asarray(t, f32)
gr = radius_f64(gt, K, poses).astype(f32)
m1 = (gt > 0) & (gt < 80)
print(f"valid pixels {int(m1.sum())} of {gt.size}; ground-truth radius on them: min {gr[m1].min():.4f} max {gr[m1].max():.4f}")
assert gr[m1].min() >= 0.3 and (pred < 0).any() and not mask.all()

G = {"keys": np.array(KEYS), "clips": np.array([CLIPS[k] for k in ("pre_clip_min", "pre_clip_max", "post_clip_min", "post_clip_max")], f32),
     "pred": pred, "gt": gt, "gt_radius": gr, "mask": mask, "K": K, "poses": poses}
metric_distance = map_distance = 0.0
for cname, ckw in (("noclip", {}), ("clip", CLIPS)):
    res, rmap = ev_depth.depth_evaluation_in_global_coord(torch.from_numpy(pred.copy()), torch.from_numpy(gt.copy()), torch.from_numpy(gr.copy()),
                                                          poses.copy(), K.copy(), custom_mask=torch.from_numpy(mask.copy()),
                                                          align_with_lstsq=True, **ckw)
    rmap = rmap.numpy().reshape(gt.shape).astype(f32)
    G[cname + "_vals"] = np.array([float(res[x]) for x in KEYS], f64)
    G[cname + "_map"] = rmap
    cam, _, _, _ = ev_depth.depth_evaluation(torch.from_numpy(pred.copy()), torch.from_numpy(gt.copy()), custom_mask=torch.from_numpy(mask.copy()),
                                             align_with_lstsq=True, **ckw)
    print(f"{cname}: reference Abs Rel in global coordinates {res['Abs Rel']:.6f}, in camera coordinates {cam['Abs Rel']:.6f}")
    vals, emap, (s_r, t_r), (s_d, t_d) = emulate_device(pred, gt, gr, poses, K, mask, ckw)
    G[cname + "_emu_fits"] = np.array([s_r, t_r, s_d, t_d], f32)
    G[cname + "_map_equal"] = emap.view(np.uint32) == rmap.view(np.uint32)
    md = max(abs(v - float(res[x])) / max(abs(float(res[x])), 1e-12) for v, x in zip(vals, KEYS[:8]))
    pd = float((np.abs(emap.astype(f64) - rmap) / np.abs(rmap)).max())
    for v, x in zip(vals, KEYS[:8]):
        print(f"{cname} {x:16s} reference {float(res[x]):.9g} emulation {v:.9g}")
    print(f"{cname}: emulation (s_r, t_r) = ({s_r:.9g}, {t_r:.9g}), (s_d, t_d) = ({s_d:.9g}, {t_d:.9g}); largest relative distance from the "
          f"reference: metrics {md:.3e}, radius map {pd:.3e}; map bit-equal on {int(G[cname + '_map_equal'].sum())} of {gt.size} pixels")
    metric_distance, map_distance = max(metric_distance, md), max(map_distance, pd)
G["metric_distance"] = f64(metric_distance)
G["map_distance"] = f64(map_distance)
print(f"metric_distance {metric_distance:.3e}  map_distance {map_distance:.3e}")
np.savez_compressed(os.path.join(OUT, "depth_global_golden.npz"), **G)
print("wrote", os.path.join(OUT, "depth_global_golden.npz"), len(G), "arrays")
