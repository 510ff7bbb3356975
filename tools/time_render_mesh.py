#!/usr/bin/env python
"""python tools/time_render_mesh.py [--grid 159] [--frames 2] [--reps 3] [--inner 5] [--device 0]
Seconds per call of the ScanNet++ mesh renderer on one synthetic mesh, host mirror against device, interleaved in
one process.  Needs a GPU: the device path has no fallback.

The mesh: a bumpy sheet of (grid - 1)^2 * 2 triangles, 4 m x 3 m at z ~ 2 m (cells of 25 mm at the default, 5 to 10 pixels each), in front of
a two-triangle wall at z = 4 m, with a two-triangle floor 1.2 m below the camera that runs from behind it to the wall (it straddles the
camera plane: the whole-frame path).  Rendered at 690 x 920 with a focal length of 700 pixels from --frames cameras that step sideways.

What is timed, per repetition and in this order:
  host      harness.render.render_mesh, the numpy mirror
  device    Engine.prep_render_mesh, wall clock around --inner calls in a row (each one mesh and camera upload, four kernels, synchronise,
            download of depth, normals and index), per call
  kernels   --inner more calls under ug_profile_begin / ug_profile_end: HIP events around the four launches, per call
The device path's first call (code-object load) is reported on its own and not averaged.  The two results are compared at the end."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unigeo_amd._lib import Engine
from unigeo_amd.harness.render import render_mesh

H, W = 690, 920
K = (700.0, 700.0, 460.3, 345.2)


def make_mesh(n, seed=0):
    rng = np.random.default_rng(seed)
    xx, yy = np.meshgrid(np.linspace(-2.0, 2.0, n), np.linspace(-1.5, 1.5, n))
    zz = 2.0 + 0.15 * np.sin(3 * xx) * np.cos(2 * yy) + 0.01 * rng.random((n, n))
    v = np.stack([xx, yy, zz], -1).reshape(-1, 3)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel(), idx[1:, :-1].ravel()
    f = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    extra = np.array([[-6, -6, 4], [6, -6, 4], [6, 6, 4], [-6, 6, 4], [-6, 1.2, -3], [6, 1.2, -3], [6, 1.2, 4], [-6, 1.2, 4]], np.float64)
    o = n * n
    f = np.concatenate([f, [[o, o + 1, o + 2], [o, o + 2, o + 3], [o + 4, o + 5, o + 6], [o + 4, o + 6, o + 7]]])
    return np.concatenate([v, extra]).astype(np.float32), f.astype(np.int32)


def make_poses(T):
    poses = np.tile(np.eye(4), (T, 1, 1))
    poses[:, 0, 3] = np.linspace(-0.3, 0.3, T) if T > 1 else 0.0
    return poses


def clock(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=159); ap.add_argument("--frames", type=int, default=2); ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5); ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    v, f = make_mesh(a.grid)
    poses = make_poses(a.frames)
    eng = Engine(a.device, workspace_bytes=512 << 20, persist_bytes=1 << 20)
    print(f"# mesh renderer, {len(f)} triangles / {len(v)} vertices, {a.frames} frames of {H} x {W}; device figures are per call over {a.inner} calls in a row")
    t_first, dev = clock(lambda: eng.prep_render_mesh(v, f, poses, K, H, W))
    print(f"device, first call (code load included): {t_first * 1e3:.2f} ms")
    rows = []
    for r in range(a.reps):
        t_host, host = clock(lambda: render_mesh(v, f, poses, K, H, W))
        t_dev, dev = clock(lambda: [eng.prep_render_mesh(v, f, poses, K, H, W) for _ in range(a.inner)][-1])
        t_dev /= a.inner
        eng.profile_begin()
        for _ in range(a.inner):
            eng.prep_render_mesh(v, f, poses, K, H, W)
        prof = eng.profile_end()["render_mesh"]
        assert prof["calls"] == a.inner
        t_k = prof["ms"] * 1e-3 / a.inner
        rows.append((t_host, t_dev, t_k))
        print(f"rep {r}: host mirror {t_host * 1e3:9.1f} ms | device call {t_dev * 1e3:7.2f} ms | kernels (HIP events) {t_k * 1e3:6.3f} ms", flush=True)
    m, lo = np.mean(rows, 0), np.min(rows, 0)
    print(f"mean of {a.reps}: host mirror {m[0] * 1e3:.1f} ms/call ({m[0] / a.frames * 1e3:.1f} ms/frame), device call {m[1] * 1e3:.2f} ms/call "
          f"({m[1] / a.frames * 1e3:.2f} ms/frame), kernels {m[2] * 1e3:.3f} ms/call; host / device call = {m[0] / m[1]:.0f}")
    print(f"min  of {a.reps}: host mirror {lo[0] * 1e3:.1f} ms/call, device call {lo[1] * 1e3:.2f} ms/call, kernels {lo[2] * 1e3:.3f} ms/call")
    same = all(np.array_equal(x, y) for x, y in zip(host, dev))
    print(f"same images from both: {'equal' if same else 'DIFFER'}; pixels covered {np.mean(dev[2] >= 0):.3f}, triangles that win a pixel {len(np.unique(dev[2]))}")
    eng.close()


if __name__ == "__main__":
    main()
