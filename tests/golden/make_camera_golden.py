#!/usr/bin/env python
"""Golden vectors for the camera branch, made like make_pcd_golden.py: the REFERENCE's own code is loaded by path from
/root/reference (read-only; an empty stand-in module for ``cv2``) and run on seeded synthetic inputs.  Writes tests/golden/camera_golden.npz -
data only; the other fixtures keep their bytes.

* TUM rows: ``get_tum_poses`` of ``metrics/utils.py:169-192`` on 9 camera-to-world matrices, one of them slightly off orthonormal (scipy's
  ``from_matrix`` repairs it).  Stored: the matrices, the rows, the stamps.
* Focal: ``estimate_focal_knowing_depth(pts[None], pp = (W/2, H/2), 'weiszfeld')`` of ``metrics/utils.py:68-117`` (float32, as the reference
  runs it) on two point maps: 24 x 32 with noise, and 17 x 23 with NaN pixels, pixels at z = 0 and a few far outliers.  Stored: the point maps,
  the reference's values, and ``focal_distance`` - how far the float64 restatement ``harness.pointmap.pointmap_focal`` lies from them,
  relative; tests/test_pointmap_cpu.py bounds the code under test by 2 x these.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from scipy.spatial.transform import Rotation

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
utils = load_by_path("metrics.utils", "metrics/utils.py")

rng = np.random.default_rng(20261019)
G = {}

# ---- TUM rows
N = 9
c2w = np.tile(np.eye(4), (N, 1, 1))
c2w[:, :3, :3] = Rotation.from_rotvec(rng.normal(0, 0.8, (N, 3))).as_matrix()
c2w[:, :3, 3] = rng.normal(0, 1.5, (N, 3))
c2w[4, :3, :3] += rng.normal(0, 1e-4, (3, 3))          # slightly off orthonormal
c2w[7, :3, :3] = Rotation.from_rotvec([0, np.pi - 1e-3, 0]).as_matrix()      # close to a half turn: small qw
rows, stamps = utils.get_tum_poses([m for m in c2w])
G.update(tum_c2w=c2w, tum_rows=np.asarray(rows, np.float64), tum_stamps=np.asarray(stamps, np.float64))

# ---- focal
from unigeo_amd.harness.pointmap import pointmap_focal  # noqa: E402


def point_map(H, W, f, holes):
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    z = 2.2 + 0.5 * np.sin(u / 6.0) * np.cos(v / 5.0) + rng.uniform(-0.05, 0.05, (H, W))
    p = np.stack([(u - W / 2) * z / f, (v - H / 2) * z / f, z], -1) + rng.normal(0, 0.004, (H, W, 3))
    if holes:
        p[rng.uniform(size=(H, W)) < 0.06] = np.nan
        p[rng.uniform(size=(H, W)) < 0.03, 2] = 0.0
        far = rng.uniform(size=(H, W)) < 0.03
        p[far] += rng.normal(0, 1.0, (int(far.sum()), 3))
    return p.astype(np.float32)


maps = [point_map(24, 32, 30.0, False), point_map(17, 23, 21.0, True)]
ref, dist = [], []
for k, p in enumerate(maps):
    H, W = p.shape[:2]
    with torch.no_grad():
        f_ref = utils.estimate_focal_knowing_depth(torch.from_numpy(p)[None], torch.tensor((W / 2, H / 2)), focal_mode="weiszfeld")
    f_ref = float(f_ref.reshape(-1)[0])
    f_mine = pointmap_focal(p)
    G[f"focal_pts_{k}"] = p
    ref.append(f_ref)
    dist.append(abs(f_mine - f_ref) / abs(f_ref))
    print(f"focal {k}: reference (float32) {f_ref!r}  restatement (float64) {f_mine!r}  relative distance {dist[-1]:.3g}")
G.update(focal_ref=np.array(ref, np.float64), focal_distance=np.array(dist, np.float64))

np.savez_compressed(os.path.join(OUT, "camera_golden.npz"), **G)
print("wrote", os.path.join(OUT, "camera_golden.npz"), len(G), "arrays")
