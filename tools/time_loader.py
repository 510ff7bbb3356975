#!/usr/bin/env python
"""python tools/time_loader.py [--layout scannetpp] [--frames 25] [--height H] [--width W] [--out-h 384] [--out-w 512] [--reps 2] [--device 0]
Seconds per clip of a loader with prep="host" and prep="device" (DESIGN.md sections 16 and 17), interleaved in one process on one
synthetic scene written at the dataset's native size into a temp directory.  Needs a GPU: the device path has no fallback.
--layout: scannetpp (default, 1168 x 1752) or one of the RGB-D layouts of harness/rgbd.py - 7scenes, bonn, neuralrgbd (480 x 640), replica
(680 x 1200, cropped to 680 x 906) and scannetv2 (968 x 1296 JPEG colour next to 480 x 640 depth); --height / --width override the size.

What is timed, per repetition and in this order:
  decode       decode_clip alone (PIL: 2 webp + 1 png per frame; the RGB-D layouts: 1 png / jpg + 1 png, and ScanNetv2's Pillow resize) - the
               stage that stays on the host in both modes
  host         dataset[0] with prep="host"; its split: gt = load_clip alone - decode, resize = dataset[0] - load_clip alone
  device       dataset[0] with prep="device"; its split is the dataset's own last_timing (decode / resize / gt)
The device path's first sample (engine creation, code-object load) is reported on its own and not averaged.
The scene is smooth shading plus noise; webp / png decode time depends on the content, so "decode" is indicative only."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unigeo_amd.harness import rgbd
from unigeo_amd.harness.scannetpp import FRAME_GAP, ScannetPPDataset, decode_clip, load_clip

NATIVE = {"scannetpp": (1168, 1752), "7scenes": (480, 640), "bonn": (480, 640), "neuralrgbd": (480, 640), "replica": (680, 1200), "scannetv2": (480, 640)}


def write_scene(root, scene, T, H, W, seed=0):
    """T frames on disk; the metadata lists FRAME_GAP x as many names, of which the loader reads every FRAME_GAP-th."""
    rng = np.random.default_rng(seed)
    d = os.path.join(root, scene)
    for sub in ("images", "normal", "depth"):
        os.makedirs(os.path.join(d, sub))
    n_all = (T - 1) * FRAME_GAP + 1
    names = [f"frame_{i:06d}" for i in range(n_all)]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    for t in range(T):
        base = 127 + 80 * np.sin(xx / 97.0 + t * 0.1) * np.cos(yy / 61.0)
        rgb = np.clip(base[..., None] + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
        nrm = np.stack([np.sin(xx / 150.0), np.cos(yy / 130.0), np.full_like(xx, 0.8)], -1)
        nrm = ((nrm / np.linalg.norm(nrm, axis=-1, keepdims=True) + 1) * 127.5).astype(np.uint8)
        nrm[:8, :8] = 0                                                         # invalid normals
        dep = (2000 + 1500 * np.sin(xx / 300.0 + t * 0.05) + 500 * np.cos(yy / 200.0)).astype(np.uint16)
        dep[-8:, -8:] = 0                                                       # missing depth
        name = names[t * FRAME_GAP]
        Image.fromarray(rgb).save(os.path.join(d, "images", name + ".webp"), quality=90, method=0)
        Image.fromarray(nrm).save(os.path.join(d, "normal", name + ".webp"), quality=90, method=0)
        Image.fromarray(dep).save(os.path.join(d, "depth", name + ".png"), compress_level=1)
    pose = np.tile(np.eye(4), (n_all, 1, 1))                                    # a slow pan: rotation about y, drift along x
    ang = np.arange(n_all) * 0.004
    pose[:, 0, 0] = pose[:, 2, 2] = np.cos(ang)
    pose[:, 0, 2], pose[:, 2, 0] = np.sin(ang), -np.sin(ang)
    pose[:, 0, 3] = np.arange(n_all) * 0.01
    K = np.tile(np.array([[W * 0.6, 0, W / 2], [0, W * 0.6, H / 2], [0, 0, 1]]), (n_all, 1, 1))
    np.savez(os.path.join(d, "scene_metadata.npz"), trajectories=pose, intrinsics=K, images=np.array(names))


def _pan(n):
    """n camera-to-world matrices of a slow pan: rotation about y, drift along x."""
    pose = np.tile(np.eye(4), (n, 1, 1))
    ang = np.arange(n) * 0.004
    pose[:, 0, 0] = pose[:, 2, 2] = np.cos(ang)
    pose[:, 0, 2], pose[:, 2, 0] = np.sin(ang), -np.sin(ang)
    pose[:, 0, 3] = np.arange(n) * 0.01
    return pose


def write_rgbd_scene(root, scene, layout, T, H, W, seed=0):
    """One scene in an RGB-D layout of harness/rgbd.py: gap x as many frames as the loader reads; the ones it skips are 1 x 1 placeholders."""
    rng = np.random.default_rng(seed)
    gap = rgbd.LAYOUTS[layout].layout.gap
    n_all = (T - 1) * gap + 1
    d = os.path.join(root, scene)
    sub_rgb, sub_dep, f_rgb, f_dep = {"7scenes": ("", "", "frame-{:06d}.color.png", "frame-{:06d}.depth.proj.png"),
                                      "bonn": ("rgb_110", "depth_110", "{:06d}.png", "{:06d}.png"),
                                      "neuralrgbd": ("images", "depth", "img{}.png", "depth{}.png"),
                                      "replica": ("imap/00/rgb", "imap/00/depth", "rgb_{}.png", "depth_{}.png"),
                                      "scannetv2": ("color_270", "depth_270", "{:06d}.jpg", "{:06d}.png")}[layout]
    for sub in (sub_rgb, sub_dep):
        os.makedirs(os.path.join(d, sub), exist_ok=True)
    Hc, Wc = (968, 1296) if layout == "scannetv2" else (H, W)                 # ScanNetv2: the colour is larger than the depth
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    yc, xc = np.mgrid[0:Hc, 0:Wc].astype(np.float32)
    unit = 5.0 if layout == "bonn" else 1.0                                    # Bonn: 1/5000 m
    for i in range(n_all):
        t, used = i // gap, i % gap == 0
        if used:
            base = 127 + 80 * np.sin(xc / 97.0 + t * 0.1) * np.cos(yc / 61.0)
            rgb = np.clip(base[..., None] + rng.normal(0, 12, (Hc, Wc, 3)), 0, 255).astype(np.uint8)
            dep = ((2000 + 1500 * np.sin(xx / 300.0 + t * 0.05) + 500 * np.cos(yy / 200.0)) * unit).astype(np.uint16)
            dep[-8:, -8:] = 0                                                  # missing depth
        else:
            rgb, dep = np.zeros((1, 1, 3), np.uint8), np.full((1, 1), 1000, np.uint16)
        kw = dict(quality=90) if layout == "scannetv2" else dict(compress_level=1)
        Image.fromarray(rgb).save(os.path.join(d, sub_rgb, f_rgb.format(i)), **kw)
        Image.fromarray(dep).save(os.path.join(d, sub_dep, f_dep.format(i)), compress_level=1)
    pose = _pan(n_all)
    if layout == "7scenes":
        for i in range(n_all):
            np.savetxt(os.path.join(d, f"frame-{i:06d}.pose.txt"), pose[i])
    elif layout == "bonn":                                                     # rotation about y by a: q = (0, sin a/2, 0, cos a/2)
        a = np.arange(n_all) * 0.004
        np.savetxt(os.path.join(d, "groundtruth_110.txt"), np.stack([np.arange(n_all) / 30.0, pose[:, 0, 3], pose[:, 1, 3], pose[:, 2, 3],
                                                                      0 * a, np.sin(a / 2), 0 * a, np.cos(a / 2)], 1), header="timestamp tx ty tz qx qy qz qw")
    elif layout == "neuralrgbd":
        np.savetxt(os.path.join(d, "poses.txt"), pose.reshape(-1, 4))
    elif layout == "replica":
        np.savetxt(os.path.join(d, "imap", "00", "traj_w_cgl.txt"), pose.reshape(-1, 16), delimiter=" ")
    else:
        np.savetxt(os.path.join(d, "pose_270.txt"), pose.reshape(-1, 4))
        os.makedirs(os.path.join(d, "intrinsic"))
        np.savetxt(os.path.join(d, "intrinsic", "intrinsic_depth.txt"), np.array([[577.6, 0, 318.9, 0], [0, 578.7, 242.7, 0], [0, 0, 1, 0], [0, 0, 0, 1]]))


def clock(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", choices=sorted(NATIVE), default="scannetpp")
    ap.add_argument("--frames", type=int, default=25); ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--width", type=int, default=None); ap.add_argument("--out-h", type=int, default=384)
    ap.add_argument("--out-w", type=int, default=512); ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    a.height, a.width = a.height or NATIVE[a.layout][0], a.width or NATIVE[a.layout][1]
    if a.layout == "scannetpp":
        write, cls, dec, load, exact = write_scene, ScannetPPDataset, decode_clip, load_clip, ("cam_normal", "cam_coord", "mask")
    else:
        write = lambda root, scene, T, H, W: write_rgbd_scene(root, scene, a.layout, T, H, W)
        cls, dec, load, exact = rgbd.LAYOUTS[a.layout], rgbd.decode_clip, rgbd.load_clip, ("cam_coord", "mask")
    tmp = tempfile.mkdtemp(prefix="ug_time_loader_")
    try:
        t_write, _ = clock(lambda: write(tmp, "sceneT", a.frames, a.height, a.width))
        size = (a.out_h, a.out_w)
        kw = dict(scenes=["sceneT"], clip_length=a.frames, clip_overlap=0, input_size=size, target_size=size)
        host = cls(tmp, **kw)
        dev = cls(tmp, prep="device", device_id=a.device, **kw)
        seq, _, ids = host.samples[0]
        assert len(ids) == a.frames
        print(f"# {a.layout} loader prep, one clip of {a.frames} frames {a.height} x {a.width} -> {a.out_h} x {a.out_w}; scene written in {t_write:.1f} s")
        t_first, s_dev = clock(lambda: dev[0])
        print(f"device, first sample (engine creation + code load included): {t_first:.3f} s")
        rows = []
        for r in range(a.reps):
            t_dec, _ = clock(lambda: dec(tmp, seq, ids))
            t_lc, _ = clock(lambda: load(tmp, seq, ids))
            t_host, s_host = clock(lambda: host[0])
            t_dev, s_dev = clock(lambda: dev[0])
            lt = dev.last_timing
            rows.append((t_dec, t_host, t_lc - t_dec, t_host - t_lc, t_dev, lt["decode"], lt["resize"], lt["gt"]))
            print(f"rep {r}: decode alone {t_dec:.3f} s | host total {t_host:.3f} s = decode + gt {t_lc - t_dec:.3f} + resize {t_host - t_lc:.3f}"
                  f" | device total {t_dev:.3f} s = decode {lt['decode']:.3f} + resize {lt['resize']:.3f} + gt {lt['gt']:.3f}")
        m = np.mean(rows, 0)
        print(f"mean of {a.reps}: host {m[1]:.3f} s/clip (decode {m[0]:.3f}, gt {m[2]:.3f}, resize {m[3]:.3f}); "
              f"device {m[4]:.3f} s/clip (decode {m[5]:.3f}, resize {m[6]:.3f}, gt {m[7]:.3f}); host / device = {m[1] / m[4]:.1f}")
        img_h, img_d = np.stack(s_host["images"]), np.stack(s_dev["images"])
        same = all(np.array_equal(np.stack(s_host[k]), np.stack(s_dev[k])) for k in exact)
        print(f"same clip from both: max |images host - device| = {np.abs(img_h - img_d).max():.2e} (0..255); {' / '.join(exact)} "
              f"{'equal' if same else 'DIFFER'}; max |world_coord host - device| = "
              f"{np.abs(np.stack(s_host['world_coord']) - np.stack(s_dev['world_coord'])).max():.2e}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
