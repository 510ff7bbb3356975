#!/usr/bin/env python
"""python tools/time_gt_normals.py [--frames 17] [--reps 3] [--inner 5] [--device 0] [--radii 2 8]
Seconds per clip of the normals fitted from depth on one synthetic native-size clip (480 x 640), per radius, with and
without a 384 x 512 target, in one process.  Needs a GPU: the device path has no fallback.

What is timed, per radius:
  host      harness.normals.fit_normals + world_normals on every full native frame, the numpy mirror, ONCE (the fit does not depend on the
            target: with one the host then picks the target's pixels, which is timed on its own)
  device    Engine.prep_gt_normals per target, wall clock around --inner calls in a row (each one upload, kernel, synchronise, three downloads),
            per call; --reps repetitions, mean and minimum
  kernel    --inner more calls under ug_profile_begin / ug_profile_end: HIP events around the launch, per call
The device path's first call (code-object load) is reported on its own and not averaged.  The frames are a slanted wall with a nearer box
(depth steps), 2 % zeros and millimetre noise, a different one per frame; the two results are compared bit for bit at the end."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unigeo_amd._lib import Engine
from unigeo_amd.harness.normals import fit_normals, world_normals
from unigeo_amd.harness.scannetpp import _backproject_gl, resize_pick

H, W = 480, 640
TARGET = (384, 512)
K = np.float32([[525, 0, 320], [0, 525, 240], [0, 0, 1]])
MAX_DEPTH = 20.0


def make_clip(T, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    clip = np.empty((T, H, W), np.uint16)
    for t in range(T):
        wall = 1900 + 2.0 * xx + 0.3 * yy + 15 * t
        box = (yy > 140) & (yy < 330) & (xx > 200 + 6 * t) & (xx < 430 + 6 * t)
        wall[box] = 900 + 0.2 * xx[box]
        raw = np.floor(wall + rng.normal(0, 1, (H, W))).astype(np.uint16)
        raw[rng.random((H, W)) < 0.02] = 0
        clip[t] = raw
    return clip


def clock(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def host_fit(clip, M, radius):
    cn, wn, nm = [], [], []
    for t in range(clip.shape[0]):
        c = _backproject_gl(clip[t].astype(np.float32) / np.float32(1000), K)
        d = -c[2]
        bad = (d < 1e-3) | (d > MAX_DEPTH)
        c[:, bad] = 0
        n, valid = fit_normals(c, ~bad, radius=radius)
        cn.append(n); wn.append(world_normals(n, M[t])); nm.append(valid)
    return np.stack(cn), np.stack(wn), np.stack(nm)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=17); ap.add_argument("--reps", type=int, default=3); ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--device", type=int, default=0); ap.add_argument("--radii", type=int, nargs="+", default=[2, 8])
    a = ap.parse_args()
    T = a.frames
    clip = make_clip(T)
    ang = 0.01 * np.arange(T)
    M = np.tile(np.eye(4, dtype=np.float32), (T, 1, 1))
    M[:, 0, 0] = M[:, 2, 2] = np.cos(ang); M[:, 0, 2] = np.sin(ang); M[:, 2, 0] = -np.sin(ang)
    K0 = np.broadcast_to(K, (T, 3, 3))
    eng = Engine(a.device, workspace_bytes=256 << 20, persist_bytes=1 << 20)
    print(f"# normals fitted from depth, one clip of {T} frames {H} x {W}; device figures are per call over {a.inner} calls in a row, {a.reps} repetitions")
    tables = {"native": (np.arange(H), np.arange(W), False), f"target {TARGET[0]} x {TARGET[1]}": (resize_pick(H, TARGET[0]), resize_pick(W, TARGET[1]), True)}
    t_first, _ = clock(lambda: eng.prep_gt_normals(clip, K0, M, *tables["native"][:2], max_depth=MAX_DEPTH, zoomed=False, radius=a.radii[0]))
    print(f"device, first call (code load included): {t_first * 1e3:.2f} ms")
    for radius in a.radii:
        t_host, host = clock(lambda: host_fit(clip, M, radius))
        print(f"radius {radius}: host mirror, fit on the full frames {t_host:.2f} s/clip ({t_host / T * 1e3:.0f} ms/frame); valid {host[2].mean():.3f}")
        for name, (rows, cols, zoomed) in tables.items():
            t_pick, want = clock(lambda: [np.ascontiguousarray(x[..., rows, :][..., cols]) + np.float32(0) if zoomed else x for x in host])
            call = lambda: eng.prep_gt_normals(clip, K0, M, rows, cols, max_depth=MAX_DEPTH, zoomed=zoomed, radius=radius)
            obs = []
            for _ in range(a.reps):
                t_dev, dev = clock(lambda: [call() for _ in range(a.inner)][-1])
                eng.profile_begin()
                for _ in range(a.inner):
                    call()
                prof = eng.profile_end()["gt_normals"]
                obs.append((t_dev / a.inner, prof["ms"] * 1e-3 / a.inner))
            m, lo = np.mean(obs, 0), np.min(obs, 0)
            same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(dev, want))
            print(f"radius {radius}, {name}: host pick {t_pick * 1e3:.1f} ms | device call mean {m[0] * 1e3:.2f} ms/clip ({m[0] / T * 1e3:.3f} ms/frame), "
                  f"min {lo[0] * 1e3:.2f} | kernel (HIP events) mean {m[1] * 1e3:.3f} ms, min {lo[1] * 1e3:.3f} | host fit / device call = "
                  f"{t_host / m[0]:.0f} | {'equal bit for bit' if same else 'DIFFER'}")
    eng.close()


if __name__ == "__main__":
    main()
