#!/usr/bin/env python
"""Golden vectors for the point-cloud evaluation, made like make_depth_global_golden.py: the REFERENCE's own code is
loaded by path from /root/reference (read-only) and run on seeded synthetic inputs.  Writes tests/golden/pcd_golden.npz - data only; the
other fixtures keep their bytes.

* Alignment: ``metrics/pcd_alignment.py`` (``Regr3D_t_ScaleShiftInv``) as ``metrics/eval_pcd.py`` drives it.  That file imports open3d,
  which is not installed, so its lines 23-82 (criterion, z shift, masked selection) are read from the file at run time and executed here
  on a 3 x 12 x 16 cloud with about a quarter of the pixels masked out.  Stored: inputs, the four monitoring scalars, the masked clouds.
  Also stored and printed: how far the closed form of ``harness.metrics.pcd_align`` lies from it (``scale_distance`` on ``pred_scale``,
  ``point_distance`` on the points); tests/test_pcd_cpu.py bounds the code under test by max(1e-6, 2 x these).
* Scores: ``accuracy`` / ``completion`` of ``metrics/utils.py`` (an empty stand-in module for ``cv2``) on two clouds of 300 points with
  unit normals.  Stored: clouds, normals and the eight numbers.
"""
import importlib.util
import os
import sys
import textwrap
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

if "cv2" not in sys.modules:
    try:
        import cv2  # noqa: F401
    except Exception:
        sys.modules["cv2"] = types.ModuleType("cv2")


def load_by_path(modname, relpath):
    spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[modname] = mod
    spec.loader.exec_module(mod)
    return mod


sys.modules.setdefault("metrics", types.ModuleType("metrics")).__path__ = [os.path.join(REF, "metrics")]
load_by_path("metrics.misc", "metrics/misc.py")
align = load_by_path("metrics.pcd_alignment", "metrics/pcd_alignment.py")
utils = load_by_path("metrics.utils", "metrics/utils.py")

f32 = np.float32
rng = np.random.default_rng(20261019)
G = {}

# ---- alignment: lines 23-82 of the reference's eval_pcd.py, executed on seeded inputs
Nf, h, w = 3, 12, 16
u, v = np.meshgrid(np.linspace(-1, 1, w), np.linspace(-1, 1, h), indexing="xy")
gt = np.stack([np.broadcast_to(u, (Nf, h, w)) + rng.normal(0, 0.02, (Nf, h, w)), np.broadcast_to(v, (Nf, h, w)) + rng.normal(0, 0.02, (Nf, h, w)),
               2.5 + 0.3 * np.sin(2 * u) * np.cos(v) + 0.2 * np.arange(Nf)[:, None, None] + rng.normal(0, 0.01, (Nf, h, w))], -1).astype(f32)
pred = (1.3 * gt + np.array([0.05, -0.02, 0.4]) + rng.normal(0, 0.01, gt.shape)).astype(f32)
mask = rng.uniform(size=(Nf, h, w)) < 0.75
rgb = rng.uniform(size=(Nf, h, w, 3)).astype(f32)
G.update(align_pred=pred, align_gt=gt, align_mask=mask, align_rgb=rgb)

with open(os.path.join(REF, "metrics/eval_pcd.py")) as f:
    body = textwrap.dedent("".join(f.readlines()[22:82]))
ns = {"Regr3D_t_ScaleShiftInv": align.Regr3D_t_ScaleShiftInv, "np": np, "torch": torch,
      "predicted_pcd_original": torch.from_numpy(pred.copy()), "ground_truth_pcd_original": torch.from_numpy(gt.copy()),
      "masks": torch.from_numpy(mask.copy()), "rgbs": torch.from_numpy(rgb.copy())}
exec(compile(body, "eval_pcd.py:23-82", "exec"), ns)
scal = np.array([ns[k].item() for k in ("pred_scale", "gt_scale", "pred_shift_z", "gt_shift_z")], f32)
G.update(align_scalars=scal, align_pts=ns["pts_all_masked"].astype(f32), align_pts_gt=ns["pts_gt_all_masked"].astype(f32),
         align_rgb_masked=ns["images_all_masked"].astype(f32))

from unigeo_amd.harness.metrics import pcd_align, pcd_scores  # noqa: E402

m = mask.reshape(-1)
p, g, (ps, gs, pz, gz) = pcd_align(pred.reshape(-1, 3)[m], gt.reshape(-1, 3)[m])
print("reference scalars (pred_scale, gt_scale, pred_shift_z, gt_shift_z):", scal.tolist())
print("closed form                                                        :", [float(ps), float(gs), float(pz), float(gz)])
G["scale_distance"] = np.float64(abs(float(ps) - float(scal[0])))
G["point_distance"] = np.float64(max(np.abs(p - G["align_pts"]).max(), np.abs(g - G["align_pts_gt"]).max()))
print("bit-equal: gt_scale", gs == scal[1], "pred_shift_z", pz == scal[2], "gt_shift_z", gz == scal[3],
      "| pred_scale distance", G["scale_distance"], "| point distance", G["point_distance"])

# ---- scores: accuracy / completion of metrics/utils.py
n = 300
a = np.concatenate([rng.uniform(-1, 1, (n, 2)), rng.normal(0, 0.05, (n, 1))], 1)
b = a + rng.normal(0, 0.02, a.shape)
rng.shuffle(b)
unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
na, nb = unit(rng.normal(size=(n, 3)) * 0.2 + [0, 0, 1]), unit(rng.normal(size=(n, 3)) * 0.2 + [0, 0, 1])
acc = utils.accuracy(a, b, na, nb)
comp = utils.completion(a, b, na, nb)
G.update(score_gt=a, score_pred=b, score_gt_normals=na, score_pred_normals=nb,
         score_vals=np.array([acc[0], comp[0], acc[2], comp[2], acc[1], comp[1], acc[3], comp[3]], np.float64))
mine = pcd_scores(a, b, na, nb)
print("scores: largest relative distance of the mirror:",
      max(abs(mine[k] - r) / abs(r) for k, r in zip(("acc", "comp", "nc1", "nc2", "acc_med", "comp_med", "nc1_med", "nc2_med"), G["score_vals"])))

np.savez_compressed(os.path.join(OUT, "pcd_golden.npz"), **G)
print("wrote", os.path.join(OUT, "pcd_golden.npz"), len(G), "arrays")
