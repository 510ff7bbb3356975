#!/usr/bin/env python
"""python tools/time_register_depth.py [--frames 17] [--reps 5] [--inner 20] [--device 0]
Seconds per clip of the 7-Scenes depth registration on one synthetic clip of 480 x 640 raw frames, interleaved in one
process.  Needs a GPU: the device path has no fallback.

What is timed, per repetition and in this order:
  host      harness.rgbd.register_depth, the numpy mirror
  device    Engine.prep_register_depth, wall clock around --inner calls in a row (each one upload, kernels, synchronise, download), per call
  kernels   --inner more calls under ug_profile_begin / ug_profile_end: HIP events around the fill, splat and finalize launches, per call
The device path's first call (code-object load) is reported on its own and not averaged.  The frames are a slanted wall with a nearer box, 2 %
zeros, 5 % scattered 65535 and 65535 borders, a different one per frame; the two results are compared at the end."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unigeo_amd._lib import Engine
from unigeo_amd.harness.rgbd import register_depth

H, W = 480, 640


def make_clip(T, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    clip = np.empty((T, H, W), np.uint16)
    for t in range(T):
        wall = 1900 + 2.0 * xx + 0.3 * yy + 15 * t
        box = (yy > 140) & (yy < 330) & (xx > 200 + 6 * t) & (xx < 430 + 6 * t)
        wall[box] = 900 + 0.2 * xx[box]
        raw = np.floor(wall + rng.normal(0, 2, (H, W))).astype(np.uint16)
        u = rng.random((H, W))
        raw[u < 0.02] = 0
        raw[u > 0.95] = 65535
        raw[:, :6] = 65535
        raw[:, -6:] = 65535
        clip[t] = raw
    return clip


def clock(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=17); ap.add_argument("--reps", type=int, default=5); ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    clip = make_clip(a.frames)
    eng = Engine(a.device, workspace_bytes=256 << 20, persist_bytes=1 << 20)
    print(f"# 7-Scenes depth registration, one clip of {a.frames} raw frames {H} x {W}; device figures are per call over {a.inner} calls in a row")
    t_first, dev = clock(lambda: eng.prep_register_depth(clip))
    print(f"device, first call (code load included): {t_first * 1e3:.2f} ms")
    rows = []
    for r in range(a.reps):
        t_host, host = clock(lambda: register_depth(clip))
        t_dev, dev = clock(lambda: [eng.prep_register_depth(clip) for _ in range(a.inner)][-1])
        t_dev /= a.inner
        eng.profile_begin()
        for _ in range(a.inner):
            eng.prep_register_depth(clip)
        prof = eng.profile_end()["register_depth"]
        assert prof["calls"] == a.inner
        t_k = prof["ms"] * 1e-3 / a.inner
        rows.append((t_host, t_dev, t_k))
        print(f"rep {r}: host mirror {t_host * 1e3:8.2f} ms | device call {t_dev * 1e3:7.2f} ms | kernels (HIP events) {t_k * 1e3:6.3f} ms")
    m, lo = np.mean(rows, 0), np.min(rows, 0)
    print(f"mean of {a.reps}: host mirror {m[0] * 1e3:.2f} ms/clip ({m[0] / a.frames * 1e3:.2f} ms/frame), device call {m[1] * 1e3:.2f} ms/clip "
          f"({m[1] / a.frames * 1e3:.3f} ms/frame), kernels {m[2] * 1e3:.3f} ms/clip; host / device call = {m[0] / m[1]:.1f}")
    print(f"min  of {a.reps}: host mirror {lo[0] * 1e3:.2f} ms/clip, device call {lo[1] * 1e3:.2f} ms/clip, kernels {lo[2] * 1e3:.3f} ms/clip")
    print(f"same clip from both: {'equal' if np.array_equal(host, dev) else 'DIFFER'}; pixels filled {np.mean(dev > 0):.3f}")
    eng.close()


if __name__ == "__main__":
    main()
