#!/usr/bin/env python
"""Golden vectors for the exact L1 alignment, made like make_depth_alignment_golden.py: the REFERENCE's own
``metrics/eval_depth.py`` / ``metrics/alignment.py`` are imported by path from /root/reference (read-only; ``cv2`` and ``tqdm`` stubbed)
and run on the inputs ``a``, ``q``, ``e`` of depth_alignment_golden.npz.  Writes tests/golden/depth_l1_golden.npz - data only; the other
fixtures keep their bytes.

For each input, without clips and with the clips of that fixture, under ``align_with_lad=True`` (scipy BFGS) and under
``align_with_lad2=True`` (1000 Adam steps): the reference's ``(s, t)`` as its solver returned them (float64), its result dict, and per
metric the spread ``|lad - lad2|`` - the reference's own disagreement about the answer, which tests/test_depth_l1_cpu.py uses as the
yardstick for this project's exact fit.  Also one integer-valued degenerate input (6-level predictions, 12-level ground truth, 150
points, seeded): vertices of its objective carry many collinear points, the case the vertex check exists for.
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

from unigeo_amd.harness.metrics import depth_evaluation as restated, l1_fit, l1_objective  # noqa: E402

# the reference's depth_evaluation does not return (s, t): record what its two solvers hand back
FITS = []


def recording(fn):
    def wrapped(*a, **k):
        s, t = fn(*a, **k)
        FITS.append((float(s), float(t)))
        return s, t
    return wrapped


ev_depth.absolute_value_scaling_torch = recording(ev_depth.absolute_value_scaling_torch)
ev_depth.absolute_value_scaling2_torch = recording(ev_depth.absolute_value_scaling2_torch)

KEYS = ["Abs Rel", "Sq Rel", "RMSE", "Log RMSE", "delta < 1.", "delta < 1.25", "delta < 1.25^2", "delta < 1.25^3", "valid_pixels"]
src = np.load(os.path.join(OUT, "depth_alignment_golden.npz"))
CLIPS = dict(zip(("pre_clip_min", "pre_clip_max", "post_clip_min", "post_clip_max"), (float(v) for v in src["clips"])))
G = {"keys": np.array(KEYS), "clips": src["clips"].astype(np.float32)}

for tag in ("a", "q", "e"):
    pred, gt, mask = src[f"{tag}_pred"], src[f"{tag}_gt"], src[f"{tag}_mask"]
    for cname, ckw in (("noclip", {}), ("clip", CLIPS)):
        vals = {}
        for mode in ("lad", "lad2"):
            res = ev_depth.depth_evaluation(torch.from_numpy(pred.copy()), torch.from_numpy(gt.copy()), custom_mask=torch.from_numpy(mask.copy()),
                                            **{"align_with_" + mode: True}, **ckw)[0]
            k = f"{tag}_{mode}_{cname}"
            vals[mode] = G[k + "_vals"] = np.array([float(res[x]) for x in KEYS], np.float64)
            G[k + "_st"] = np.array(FITS.pop(), np.float64)
            assert not FITS
        G[f"{tag}_{cname}_spread"] = np.abs(vals["lad"] - vals["lad2"])
        # informational: where the exact fit lands
        m1 = (gt > 0) & (gt < 80)
        p = pred[m1]
        if ckw:
            p = np.minimum(np.maximum(p, np.float32(ckw["pre_clip_min"])), np.float32(ckw["pre_clip_max"]))
        s, t, info = l1_fit(p, gt[m1])
        mine = restated(pred, gt, custom_mask=mask, align_with_l1=True, **ckw)[0]
        F = {m: l1_objective(p, gt[m1], *G[f"{tag}_{m}_{cname}_st"]) for m in ("lad", "lad2")}
        print(f"{tag}_{cname}: n {p.size} exact F {l1_objective(p, gt[m1], s, t):.9g} lad {F['lad']:.9g} lad2 {F['lad2']:.9g} steps {info['steps']} "
              f"s exact {s:.9g} lad {G[f'{tag}_lad_{cname}_st'][0]:.9g} rel {abs(s - G[f'{tag}_lad_{cname}_st'][0]) / abs(s):.2e}")
        for i, x in enumerate(KEYS[:8]):
            print(f"    {x:16s} lad {vals['lad'][i]:.9g} lad2 {vals['lad2'][i]:.9g} spread {abs(vals['lad'][i] - vals['lad2'][i]):.3e} "
                  f"|l1 - lad| {abs(mine[x] - vals['lad'][i]):.3e}")

rng = np.random.default_rng(20261020)
G["int_pred"] = rng.integers(0, 6, 150).astype(np.float32)
G["int_gt"] = rng.integers(1, 13, 150).astype(np.float32)
np.savez_compressed(os.path.join(OUT, "depth_l1_golden.npz"), **G)
print("wrote", os.path.join(OUT, "depth_l1_golden.npz"), len(G), "arrays")
