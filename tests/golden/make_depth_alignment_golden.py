#!/usr/bin/env python
"""Golden vectors for the depth alignment modes, made like make_goldens.py: the REFERENCE's own
``metrics/eval_depth.py`` / ``metrics/alignment.py`` are imported by path from /root/reference (read-only; ``cv2`` and ``tqdm`` stubbed)
and run on seeded synthetic inputs.  Writes tests/golden/depth_alignment_golden.npz - data only; the other fixtures keep their bytes.

Inputs at the G5 size 3 x 20 x 28 with invalid pixels (gt = 0, one gt = 90), a custom mask and some negative predictions:
  a  continuous predictions, odd count of valid pixels
  q  predictions quantised to 8 levels - the median's bin is full of ties
  e  an even count of valid pixels (the LOWER median differs from the mean of the middle pair)
For each input, each of metric / median / scale / lstsq, without clips and with (pre_min, pre_max, post_min, post_max) =
(1.0, 4.0, 0.8, 5.0): the reference's result dict, its error map, and s recovered from its third return value (pred * s) where
the mode has no shift.  Also stored and printed: the distance between the reference's float32 ``scale`` results and this project's
float64 restatement on these inputs - tests/test_depth_alignment_*.py bound ``scale`` by twice that distance.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

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
ev_depth = load_by_path("metrics.eval_depth", "metrics/eval_depth.py")

from unigeo_amd.harness.metrics import depth_evaluation as restated  # noqa: E402

MODES = {"metric": {"metric_scale": True}, "median": {}, "scale": {"align_with_scale": True}, "lstsq": {"align_with_lstsq": True}}
CLIPS = {"pre_clip_min": 1.0, "pre_clip_max": 4.0, "post_clip_min": 0.8, "post_clip_max": 5.0}
KEYS = ["Abs Rel", "Sq Rel", "RMSE", "Log RMSE", "delta < 1.", "delta < 1.25", "delta < 1.25^2", "delta < 1.25^3", "valid_pixels"]

rng = np.random.default_rng(20261017)
Nf, h, w = 3, 20, 28
G = {"keys": np.array(KEYS), "clips": np.array([CLIPS[k] for k in ("pre_clip_min", "pre_clip_max", "post_clip_min", "post_clip_max")], np.float32)}


def make_input(tag):
    gt = rng.uniform(0.5, 6.0, (Nf, h, w)).astype(np.float32)
    gt[0, :3] = 0.0; gt[1, 5, 5] = 90.0
    if tag == "e":
        gt[2, 7, 7] = 0.0
    pred = (0.7 * gt + 0.3 + 0.2 * rng.standard_normal(gt.shape)).astype(np.float32)
    neg = rng.uniform(size=gt.shape) < 0.03
    pred[neg] = -pred[neg]
    if tag == "q":
        pred = (np.round(np.clip(pred, 0.5, 4.0) * 2.0) / 2.0).astype(np.float32)      # 0.5, 1.0 ... 4.0: 8 levels
        assert len(np.unique(pred)) == 8
    mask = rng.uniform(size=gt.shape) > 0.2
    return pred, gt, mask


def recover_s(pred, scaled):
    """The float32 s with pred * s == scaled everywhere: the ratio at the largest |pred|, then its float32 neighbours."""
    i = int(np.argmax(np.abs(pred)))
    c = np.float32(scaled.reshape(-1)[i] / pred.reshape(-1)[i])
    cands = [c]
    for _ in range(4):
        cands = [np.nextafter(cands[0], np.float32(-np.inf))] + cands + [np.nextafter(cands[-1], np.float32(np.inf))]
    ok = [x for x in cands if np.array_equal(pred * x, scaled)]
    assert len(ok) == 1, (c, ok)
    return ok[0]


dist = 0.0
for tag in ("a", "q", "e"):
    pred, gt, mask = make_input(tag)
    nvalid = int(((gt > 0) & (gt < 80)).sum())
    assert nvalid % 2 == (0 if tag == "e" else 1), nvalid
    G[f"{tag}_pred"], G[f"{tag}_gt"], G[f"{tag}_mask"] = pred, gt, mask
    for mode, kw in MODES.items():
        for cname, ckw in (("noclip", {}), ("clip", CLIPS)):
            res, emap, scaled, _ = ev_depth.depth_evaluation(torch.from_numpy(pred.copy()), torch.from_numpy(gt.copy()),
                                                             custom_mask=torch.from_numpy(mask.copy()), **kw, **ckw)
            k = f"{tag}_{mode}_{cname}"
            G[k + "_vals"] = np.array([float(res[x]) for x in KEYS], np.float64)
            G[k + "_emap"] = emap.numpy().reshape(gt.shape).astype(np.float32)
            G[k + "_s"] = np.float32(np.nan) if mode == "lstsq" else recover_s(pred.reshape(-1, w), scaled.numpy())
            if mode == "scale":
                mine, (s_mine, _) = restated(pred, gt, custom_mask=mask, **kw, **ckw)
                case = 0.0
                for x in KEYS[:8]:
                    d = abs(mine[x] - float(res[x])) / max(abs(float(res[x])), 1e-12)
                    case = max(case, d)
                    print(f"scale {k:16s} {x:16s} reference {float(res[x]):.9g} restated {mine[x]:.9g} rel {d:.3e}")
                G[k + "_distance"] = np.float64(case)      # informational; the tests use the largest one
                dist = max(dist, case)
                print(f"scale {k:16s} s reference {float(G[k + '_s']):.9g} restated {s_mine:.12g} rel {abs(s_mine - float(G[k + '_s'])) / s_mine:.3e}")
G["scale_distance"] = np.float64(dist)
print(f"largest relative distance of a scale-mode metric, reference (float32) vs restatement (float64): {dist:.3e}")
np.savez_compressed(os.path.join(OUT, "depth_alignment_golden.npz"), **G)
print("wrote", os.path.join(OUT, "depth_alignment_golden.npz"), len(G), "arrays")
