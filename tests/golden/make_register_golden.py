#!/usr/bin/env python
"""python tests/golden/make_register_golden.py --reference <UniGeo checkout>
Golden for the 7-Scenes depth registration (unigeo_amd/harness/rgbd.py ``register_depth``, ``ug_prep_register_depth``):
writes two synthetic 480 x 640 raw depth frames into a temporary scene folder laid out as 7-Scenes is downloaded, runs the REFERENCE's own
``process_scene`` of ``dataset/sevenScenes/preprocess.py`` on it and stores the raw frames and the ``*.depth.proj.png`` files it wrote in
tests/golden/register_golden.npz (``raw``, ``expected``: uint16 [2,480,640]).  Runs where the reference is checked out, never in a test.

That module runs over a hard-coded folder when it is imported, through ``joblib``, and reads and writes images through ``skimage.io``.  Both
are stubbed in ``sys.modules`` before the import - ``skimage.io`` by Pillow, ``joblib.Parallel`` by a callable that runs nothing - and
``process_scene`` is then called directly.

The frames are piecewise-smooth integer millimetres: a slanted back wall between 1.9 and 3.3 m with a step, a nearer box (occlusion edges, which
the per-pixel minimum resolves), about 2 % zeros, about 5 % scattered 65535 (7-Scenes' marker of an invalid pixel, which the reference
accepts as 65.535 m) and six full columns of 65535 at each side border, whose points come out beyond 65.535 m and wrap in the reference's
16-bit cast.  The second frame differs in every part.  No per-pixel noise: it would not compress."""
import argparse
import importlib.util
import os
import shutil
import sys
import tempfile
import types

import numpy as np
from PIL import Image

OUT = os.path.dirname(os.path.abspath(__file__))
H, W = 480, 640


def make_frame(k, rng):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    wall = 1900 + 2.0 * xx + 0.3 * yy * (1 + k)                                   # slanted: neighbouring sources fold onto one target
    wall[yy > 300 + 40 * k] += 180                                                 # a step
    box = (yy > 140 - 30 * k) & (yy < 330) & (xx > 200 + 50 * k) & (xx < 430 + 20 * k)
    wall[box] = 900 + 60 * k + 0.2 * xx[box]                                       # the nearer box
    raw = np.floor(wall).astype(np.uint16)
    u = rng.random((H, W))
    raw[u < 0.02] = 0
    raw[u > 0.95] = 65535
    raw[:, :6] = 65535
    raw[:, -6:] = 65535
    return raw


def stub_modules():
    io = types.ModuleType("skimage.io")
    io.imread = lambda path: np.array(Image.open(path))
    io.imsave = lambda path, arr: Image.fromarray(arr).save(path)
    sk = types.ModuleType("skimage")
    sk.io = io
    sk.__path__ = []
    jl = types.ModuleType("joblib")
    jl.Parallel = lambda *a, **k: (lambda jobs: None)                              # the import-time run over the hard-coded folder: nothing
    jl.delayed = lambda f: f
    sys.modules.update({"skimage": sk, "skimage.io": io, "joblib": jl})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    a = ap.parse_args()
    stub_modules()
    spec = importlib.util.spec_from_file_location("ref_preprocess", os.path.join(a.reference, "dataset", "sevenScenes", "preprocess.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(7)
    raw = np.stack([make_frame(k, rng) for k in range(2)])
    tmp = tempfile.mkdtemp(prefix="ug_register_golden_")
    try:
        scene = os.path.join(tmp, "chess")
        os.makedirs(os.path.join(scene, "seq-01"))
        with open(os.path.join(scene, "TestSplit.txt"), "w") as f:
            f.write("sequence1\n")
        for k in range(2):
            Image.fromarray(raw[k]).save(os.path.join(scene, "seq-01", f"frame-{k:06d}.depth.png"))
        mod.process_scene(scene)
        expected = np.stack([np.array(Image.open(os.path.join(scene, "seq-01", f"frame-{k:06d}.depth.proj.png"))) for k in range(2)])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert expected.dtype == np.uint16 and expected.shape == raw.shape
    path = os.path.join(OUT, "register_golden.npz")
    np.savez_compressed(path, raw=raw, expected=expected)
    print(f"{path}: {os.path.getsize(path)} bytes; zeros {np.mean(raw == 0):.3f}, 65535 {np.mean(raw == 65535):.3f}, "
          f"registered holes {np.mean(expected == 0):.3f}")


if __name__ == "__main__":
    main()
