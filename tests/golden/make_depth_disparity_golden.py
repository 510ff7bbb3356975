#!/usr/bin/env python
"""Golden vectors for the depth evaluation in disparity space, made like make_depth_alignment_golden.py: the
REFERENCE's own ``metrics/eval_depth.py`` / ``metrics/alignment.py`` are imported by path from /root/reference (read-only; ``cv2`` and
``tqdm`` stubbed) and run with ``disp_input=True`` on seeded synthetic inputs.  That branch calls ``depth2disparity``, which the reference
defines nowhere; the three lines below - this project's own definition, y = 1 / x where x > 0, else 0 - are assigned into the loaded
module, and with them the reference's code path runs.  Writes tests/golden/depth_disparity_golden.npz - data only.

Inputs at the G5 size 3 x 20 x 28: gt ~ U(0.5, 4); the prediction is a disparity, 0.5 / gt + 0.2 + 0.01 N(0, 1), made BEFORE the invalid
pixels (three zeroed rows, one gt = 90) are written, so every prediction is finite; the sign of 3 % of the predictions is flipped (aligned
disparity <= 0 -> depth 0); a custom mask.
  a  continuous predictions, odd count of valid pixels
  q  predictions quantised to eighths in [0.25, 1] - the median's bin is full of ties
  e  an even count of valid pixels
For each input, each of metric / median / scale / lstsq, without clips and with (pre_min, pre_max, post_min, post_max) =
(0.3, 1.0, 0.8, 5.0): the reference's result dict, its error map, and s recovered from its third return value (the inverted pred * s)
where the mode has no shift.  Also stored and printed: the distance between the reference's float32 ``scale`` results and this project's
float64 restatement on these inputs - tests/test_depth_disparity_*.py bound ``scale`` by twice that distance.

GUARD.  d = 1 / a turns a relative change of the aligned disparity a into the same relative change of d, so where a approaches 0 the
metrics depend on the last bits of (s, t).  Every stored case must keep |a| >= 0.1 on mask1 - for the pre-clipped prediction the metrics
see and for the original one the error map sees, with the restated (s, t) - and the reference's own depth map (made from the original
prediction) must hold no value in (10, inf).  An input that fails is changed; the guard is not.  That happened once: with gt ~ U(0.5, 6)
and noise 0.02 N(0, 1), least squares with the pre-clip on fits so well that a follows 1 / gt down to 1 / 6 less 0.1 of noise, 0.03 ..
0.09 on eight seeds out of eight; hence the range U(0.5, 4) and the noise 0.01 N(0, 1), the values of the frame-size GPU input.
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


def depth2disparity(x):
    y = torch.zeros_like(x)
    y[x > 0] = 1 / x[x > 0]
    return y


ev_depth.depth2disparity = depth2disparity      # the name the reference calls and never defines

from unigeo_amd.harness.metrics import depth_evaluation as restated  # noqa: E402

MODES = {"metric": {"metric_scale": True}, "median": {}, "scale": {"align_with_scale": True}, "lstsq": {"align_with_lstsq": True}}
CLIPS = {"pre_clip_min": 0.3, "pre_clip_max": 1.0, "post_clip_min": 0.8, "post_clip_max": 5.0}
KEYS = ["Abs Rel", "Sq Rel", "RMSE", "Log RMSE", "delta < 1.", "delta < 1.25", "delta < 1.25^2", "delta < 1.25^3", "valid_pixels"]
GUARD = 0.1

rng = np.random.default_rng(20261020)
Nf, h, w = 3, 20, 28
G = {"keys": np.array(KEYS), "clips": np.array([CLIPS[k] for k in ("pre_clip_min", "pre_clip_max", "post_clip_min", "post_clip_max")], np.float32)}


def make_input(tag):
    gt = rng.uniform(0.5, 4.0, (Nf, h, w)).astype(np.float32)
    pred = (0.5 / gt + 0.2 + 0.01 * rng.standard_normal(gt.shape)).astype(np.float32)      # before the invalid pixels: finite everywhere
    gt[0, :3] = 0.0; gt[1, 5, 5] = 90.0
    if tag == "e":
        gt[2, 7, 7] = 0.0
    neg = rng.uniform(size=gt.shape) < 0.03
    pred[neg] = -pred[neg]
    if tag == "q":
        pred = (np.round(np.clip(pred, 0.25, 1.0) * 8.0) / 8.0).astype(np.float32)
        assert set(np.unique(pred)) <= {np.float32(k / 8) for k in range(2, 9)}
    mask = rng.uniform(size=gt.shape) > 0.2
    assert np.isfinite(pred).all()
    return pred, gt, mask


def invert(a):
    out = np.zeros(a.shape, np.float32)
    out[a > 0] = np.float32(1) / a[a > 0]
    return out


def recover_s(pred, inverted):
    """The float32 s with invert(pred * s) == inverted everywhere: 1 / (pred * depth) at the largest positive prediction, then its
    float32 neighbours."""
    pred, inverted = pred.reshape(-1), inverted.reshape(-1)
    i = int(np.argmax(pred))
    c = np.float32(1.0 / (float(inverted[i]) * float(pred[i])))
    cands = [c]
    for _ in range(8):
        cands = [np.nextafter(cands[0], np.float32(-np.inf))] + cands + [np.nextafter(cands[-1], np.float32(np.inf))]
    ok = [x for x in cands if np.array_equal(invert(pred * x), inverted)]
    assert len(ok) == 1, (c, ok)
    return ok[0]


dist, min_a, min_a0, nonpos = 0.0, np.inf, np.inf, {}
for tag in ("a", "q", "e"):
    pred, gt, mask = make_input(tag)
    m1 = (gt > 0) & (gt < 80)
    nvalid = int(m1.sum())
    assert nvalid % 2 == (0 if tag == "e" else 1), nvalid
    G[f"{tag}_pred"], G[f"{tag}_gt"], G[f"{tag}_mask"] = pred, gt, mask
    for mode, kw in MODES.items():
        for cname, ckw in (("noclip", {}), ("clip", CLIPS)):
            res, emap, inverted, _ = ev_depth.depth_evaluation(torch.from_numpy(pred.copy()), torch.from_numpy(gt.copy()),
                                                               custom_mask=torch.from_numpy(mask.copy()), disp_input=True, **kw, **ckw)
            k = f"{tag}_{mode}_{cname}"
            inverted = inverted.numpy().reshape(gt.shape)
            mine, (s_mine, t_mine) = restated(pred, gt, custom_mask=mask, align_space="disparity", **kw, **ckw)
            # the guard: the aligned disparity of the metrics (pre-clipped prediction) and of the error map (original prediction) on mask1
            s32, t32 = np.float32(s_mine), np.float32(t_mine)
            pc = np.clip(pred, np.float32(ckw["pre_clip_min"]), np.float32(ckw["pre_clip_max"])) if ckw else pred
            case_min, map_min = float(np.abs(s32 * pc[m1] + t32).min()), float(np.abs(pred[m1] * s32 + t32).min())
            assert case_min >= GUARD, (k, case_min)
            assert map_min >= GUARD, (k, map_min)
            min_a0 = min(min_a0, map_min)
            assert not ((inverted[m1] > 10) & np.isfinite(inverted[m1])).any() and np.isfinite(inverted[m1]).all(), k
            min_a = min(min_a, case_min)
            nonpos[k] = int((pred[m1] * s32 + t32 <= 0).sum())
            G[k + "_vals"] = np.array([float(res[x]) for x in KEYS], np.float64)
            G[k + "_emap"] = emap.numpy().reshape(gt.shape).astype(np.float32)
            G[k + "_s"] = np.float32(np.nan) if mode == "lstsq" else recover_s(pred, inverted)
            case = 0.0
            for x in KEYS[:8]:
                d = abs(mine[x] - float(res[x])) / max(abs(float(res[x])), 1e-12)
                case = max(case, d)
                if mode == "scale":
                    print(f"scale {k:16s} {x:16s} reference {float(res[x]):.9g} restated {mine[x]:.9g} rel {d:.3e}")
            if mode == "scale":
                G[k + "_distance"] = np.float64(case)      # informational; the tests use the largest one
                dist = max(dist, case)
                print(f"scale {k:16s} s reference {float(G[k + '_s']):.9g} restated {s_mine:.12g} rel {abs(s_mine - float(G[k + '_s'])) / s_mine:.3e}")
            else:
                print(f"{k:22s} largest relative distance of a metric, reference vs restatement {case:.3e}; min |a| {case_min:.4f}; "
                      f"a <= 0 on {nonpos[k]} pixels")
G["scale_distance"] = np.float64(dist)
G["min_abs_aligned_disparity"] = np.float64(min_a)
G["min_abs_aligned_disparity_map"] = np.float64(min_a0)
print(f"largest relative distance of a scale-mode metric, reference (float32) vs restatement (float64): {dist:.3e}")
print(f"smallest |aligned disparity| over all cases: {min_a:.4f} (guard {GUARD}); of the error map's: {min_a0:.4f} (same guard)")
np.savez_compressed(os.path.join(OUT, "depth_disparity_golden.npz"), **G)
print("wrote", os.path.join(OUT, "depth_disparity_golden.npz"), len(G), "arrays")
