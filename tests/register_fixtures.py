"""Inputs shared by tests/test_register_depth_cpu.py and tests/test_register_depth_gpu.py: the golden, the hand-built
tie / collision / identity cases with their options, a scalar restatement of the registration for tiny frames, and a temporary 7-Scenes
scene written from the golden."""
import os

import numpy as np
from PIL import Image

from unigeo_amd.harness.rgbd import RegisterOpts

G = os.path.join(os.path.dirname(__file__), "golden")
SCENE = "chess/seq-01"


def golden():
    with np.load(os.path.join(G, "register_golden.npz")) as f:
        return f["raw"], f["expected"]


def identity_opts(focal, dst_focal=None, half_pixel=True, divisor=1000.0):
    """The identity rotation without translation.  The definition back-projects the pixel CENTRE (0.5 + col) and projects without taking the
    half back, so under the plain identity every projection lands on col + .5 - the tie case.  ``half_pixel=True`` puts -0.5 / dst_focal into
    the third column (x3 = X - 0.5 Z / f, y3 likewise), which moves the projection onto col."""
    f2 = focal if dst_focal is None else dst_focal
    s = -0.5 / f2 if half_pixel else 0.0
    return RegisterOpts(src_focal=focal, dst_focal=f2, src2dst=(1, 0, s, 0, 0, 1, s, 0, 0, 0, 1, 0), divisor=divisor, max_valid=100.0)


def all_values_frame():
    """37 x 53 (no multiple of a wave or a block), every valid raw depth class: 0, the 65535 marker, and values spread over 1 .. 65534."""
    rng = np.random.default_rng(3)
    raw = rng.integers(1, 65535, (37, 53)).astype(np.uint16)
    raw[3, 4:9] = 0
    raw[20, 30:33] = 65535
    return raw


def millimetre_round_trip(raw):
    """uint16(trunc(fl32(1000f * fl32(raw / 1000f)))): what an unmoved pixel comes out as.  It is raw itself for all but 739 of the 65534
    values 1 .. 65534 (the product rounds below the integer and the cast truncates)."""
    return (np.float32(1000.0) * (raw.astype(np.float32) / np.float32(1000.0))).astype(np.int64).astype(np.uint16)


def tie_case():
    """1 x 8, focal 1, divisor 1024 and depths that are powers of two, so that every step is exact: column c projects to exactly c + .5 and
    rounds to even - 0 -> 0, 1 and 2 -> 2, 3 and 4 -> 4, 5 and 6 -> 6, 7 -> 8 (outside, dropped).  -> (raw, opts, expected)."""
    raw = np.array([[1024, 2048, 512, 4096, 8192, 256, 128, 64]], np.uint16)       # d = 1, 2, .5, 4, 8, .25, .125, .0625
    expected = np.array([[1000, 0, 500, 0, 4000, 0, 125, 0]], np.uint16)           # 1000 * min of the depths that share a target
    return raw, identity_opts(1.0, half_pixel=False, divisor=1024.0), expected


def collision_case():
    """24 x 32 with the target focal a quarter of the source focal: about 16 sources land on each target, the smallest depth wins."""
    rng = np.random.default_rng(5)
    raw = rng.integers(500, 6000, (24, 32)).astype(np.uint16)
    raw[rng.random((24, 32)) < 0.1] = 0
    return raw, identity_opts(40.0, dst_focal=10.0)


def loop_reference(raw, opts, drop=False):
    """The definition one pixel at a time in Python floats (IEEE double, no fused operation) and numpy float32 scalars, with Python's
    ``round``: for tiny frames only.  Independent of the vectorised mirror."""
    H, W = raw.shape
    m = [float(x) for x in opts.src2dst]
    zbuf = np.full((H, W), np.float32(2000.0), np.float32)
    for r in range(H):
        for c in range(W):
            d32 = np.float32(raw[r, c]) / np.float32(opts.divisor)
            if not (d32 > 0 and d32 < np.float32(opts.max_valid)) or (drop and raw[r, c] == 65535):
                continue
            d = float(d32)
            X = (((0.5 + c) - W / 2) / opts.src_focal) * d
            Y = (((0.5 + r) - H / 2) / opts.src_focal) * d
            x3 = ((m[0] * X + m[1] * Y) + m[2] * d) + m[3]
            y3 = ((m[4] * X + m[5] * Y) + m[6] * d) + m[7]
            z3 = ((m[8] * X + m[9] * Y) + m[10] * d) + m[11]
            x, y = round(((x3 / z3) * opts.dst_focal) + W / 2), round(((y3 / z3) * opts.dst_focal) + H / 2)
            if x < 0 or y < 0 or y >= H or x >= W:
                continue
            zbuf[y, x] = min(zbuf[y, x], np.float32(z3))
    zbuf[zbuf > 1000] = 0
    return ((np.float32(1000.0) * zbuf).astype(np.int64) % 65536).astype(np.uint16)


def write_scene(root, raw, expected, size=None):
    """<root>/chess/seq-01 with ``frame-*.depth.png`` from raw, ``frame-*.depth.proj.png`` from expected, colour and pose files.
    ``size=(h, w)``: the top-left corner of that size of every image instead."""
    d = os.path.join(root, SCENE)
    os.makedirs(d)
    T, H, W = raw.shape
    h, w = size or (H, W)
    yy, xx = np.mgrid[0:h, 0:w]
    for t in range(T):
        rgb = np.stack([(xx + 3 * t) % 256, (yy * 2 + t) % 256, (xx + yy) % 256], -1).astype(np.uint8)
        Image.fromarray(rgb).save(os.path.join(d, f"frame-{t:06d}.color.png"), compress_level=1)
        Image.fromarray(np.ascontiguousarray(raw[t, :h, :w])).save(os.path.join(d, f"frame-{t:06d}.depth.png"), compress_level=1)
        Image.fromarray(np.ascontiguousarray(expected[t, :h, :w])).save(os.path.join(d, f"frame-{t:06d}.depth.proj.png"), compress_level=1)
        pose = np.eye(4)
        a = 0.02 * t
        pose[0, 0] = pose[2, 2] = np.cos(a)
        pose[0, 2], pose[2, 0] = np.sin(a), -np.sin(a)
        pose[:3, 3] = (0.05 * t, 0.0, 0.01 * t)
        np.savetxt(os.path.join(d, f"frame-{t:06d}.pose.txt"), pose)
    return root


def assert_same_sample(a, b):
    """Two loader samples equal in every key; arrays bit for bit."""
    assert list(a.keys()) == list(b.keys())
    for k in a:
        if isinstance(a[k], list) and len(a[k]) and isinstance(a[k][0], np.ndarray):
            x, y = np.stack(a[k]), np.stack(b[k])
            assert x.dtype == y.dtype and x.shape == y.shape, k
            assert x.tobytes() == y.tobytes(), k
        else:
            assert a[k] == b[k], k
