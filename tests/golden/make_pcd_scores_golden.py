#!/usr/bin/env python
"""Golden vectors for recall at a distance threshold, made like make_pcd_golden.py: the REFERENCE's own
``completion_ratio`` (``metrics/utils.py:7-11``, loaded by path from /root/reference, read-only, with an empty stand-in module for ``cv2``)
is run on two seeded cloud pairs with its default ``dist_th=0.05``.  Writes tests/golden/pcd_scores_golden.npz - data only: the clouds and
the float32 values it returned.  tests/test_pcd_scores_cpu.py asserts ``np.float32(recall@0.05)`` of the mirror equal to them bit for bit."""
import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

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
utils = load_by_path("metrics.utils", "metrics/utils.py")

rng = np.random.default_rng(20261021)
G = {}
for name, n, noise in (("a", 300, 0.03), ("b", 1000, 0.05)):
    gt = np.concatenate([rng.uniform(-1, 1, (n, 2)), rng.normal(0, 0.05, (n, 1))], 1)
    rec = gt + rng.normal(0, noise, gt.shape)
    rec[rng.choice(n, n // 10, replace=False)] += rng.uniform(-0.5, 0.5, (n // 10, 3))
    rng.shuffle(rec)
    ratio = utils.completion_ratio(gt, rec)
    assert isinstance(ratio, np.float32)
    G[f"gt_{name}"], G[f"rec_{name}"], G[f"ratio_{name}"] = gt, rec, np.float32(ratio)
    print(f"pair {name}: n {n} completion_ratio {float(ratio)!r}")

np.savez_compressed(os.path.join(OUT, "pcd_scores_golden.npz"), **G)
print("wrote", os.path.join(OUT, "pcd_scores_golden.npz"), len(G), "arrays")
