#!/usr/bin/env python
"""python tools/render_scannetpp.py ROOT OUT --scenes SCENE ... [--device [ID]] [--target-resolution 920] [--frames-per-call 8] [--lossless] [--overwrite]
Makes the processed ScanNet++ layout that ``ScannetPPDataset`` reads - ``OUT/<scene>/{scene_metadata.npz, images/*.webp, depth/*.png,
normal/*.webp}`` - from the raw dataset, for the iPhone stream: what the reference's ``dataset/scannetpp/preprocess_scannetpp_imu.py``
(``process_scenes``) writes, without pyrender, trimesh, OpenGL or OpenCV.  Depth and normals are rendered from the scan mesh by the
project's own rasteriser: the numpy mirror without --device, the GPU with it (no fallback).

Reads, per scene, ``ROOT/data/<scene>/iphone/pose_intrinsic_imu.json`` (``aligned_pose``, ``intrinsic`` per frame),
``iphone/rgb/frame_*.jpg``, ``iphone/rgb_masks/frame_*.png`` and ``scans/mesh_aligned_0.05.ply``.  Every frame is rescaled so that it covers
(target, target * 3 / 4) - LANCZOS when shrinking, BICUBIC otherwise, the mask by nearest neighbour - its intrinsics follow, the mesh is
rendered with them, the depth is zeroed where the mask is below 255.  ``scene_metadata.npz`` holds ``trajectories`` (camera-to-world),
``intrinsics`` (colmap convention: pixel centres at halves) and ``images`` (the frame names).  The images and normals are WebP at Pillow's
default (lossy) setting, as the script's; --lossless writes them without loss.  ``depth_vis/`` (colour previews) is not written.
A scene whose metadata exists is skipped unless --overwrite is given."""
import argparse
import json
import os
import sys

import numpy as np
from PIL import Image, features

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unigeo_amd.harness.ply import read_ply_mesh
from unigeo_amd.harness.render import nearest_resize, render_mesh, rescaled_size_and_intrinsics

try:
    LANCZOS, BICUBIC = Image.Resampling.LANCZOS, Image.Resampling.BICUBIC
except AttributeError:                                            # Pillow < 9.1
    LANCZOS, BICUBIC = Image.LANCZOS, Image.BICUBIC


def load_imu(path):
    """``pose_intrinsic_imu.json`` -> {frame name: (cam_to_world 4x4, intrinsic 3x3)} (the script's ``load_imu``)."""
    with open(path) as f:
        data = json.load(f)
    return {k: (np.array(v["aligned_pose"], np.float64), np.array(v["intrinsic"], np.float64)) for k, v in data.items()}


def colmap_intrinsics(K):
    k = K.copy()
    k[0, 2] += 0.5; k[1, 2] += 0.5
    return k


def prepare_frame(rgb, mask, K, target_resolution):
    """One raw frame -> (PIL image, mask uint8 [H,W], intrinsics 3x3 in the colmap convention) at the output size."""
    h, w = rgb.shape[:2]
    if mask.shape[:2] != (h, w):
        raise ValueError("the mask and the image differ in size")
    (wo, ho), k, scale = rescaled_size_and_intrinsics((w, h), K, (target_resolution, target_resolution * 3.0 / 4))
    image = Image.fromarray(rgb).resize((wo, ho), resample=LANCZOS if scale < 1 else BICUBIC)
    return image, nearest_resize(mask, (wo, ho)), colmap_intrinsics(k)


def process_scene(root, out, scene, render, target_resolution, frames_per_call, save_kw):
    data = os.path.join(root, "data", scene)
    rgb_dir, mask_dir = os.path.join(data, "iphone", "rgb"), os.path.join(data, "iphone", "rgb_masks")
    ply = os.path.join(data, "scans", "mesh_aligned_0.05.ply")
    for p in (ply, rgb_dir, mask_dir):
        if not os.path.exists(p):
            raise FileNotFoundError(f"raw ScanNet++ scene {scene}: {p} is missing")
    verts, faces = read_ply_mesh(ply)
    if len(faces) == 0:
        raise ValueError(f"{ply}: the mesh has no faces")
    imu = load_imu(os.path.join(data, "iphone", "pose_intrinsic_imu.json"))
    names = [n for n in sorted(f[:-4] for f in os.listdir(rgb_dir) if f.startswith("frame_") and f.endswith(".jpg")) if n in imu]
    if not names:
        raise ValueError(f"raw ScanNet++ scene {scene}: no frame of iphone/rgb has a pose")
    dst = os.path.join(out, scene)
    for sub in ("images", "depth", "normal"):
        os.makedirs(os.path.join(dst, sub), exist_ok=True)
    intrinsics, pending = [], []

    def flush():
        if not pending:
            return
        poses = np.stack([imu[n][0] for n, _, _ in pending])
        ks = np.stack([k for _, k, _ in pending])
        masks = np.stack([m for _, _, m in pending])
        depth, normal, _ = render(verts, faces, poses, ks, masks.shape[1], masks.shape[2], masks)
        for (n, _, _), d, nm in zip(pending, depth, normal):
            Image.fromarray(d).save(os.path.join(dst, "depth", n + ".png"))
            Image.fromarray(nm).save(os.path.join(dst, "normal", n + ".webp"), **save_kw)
        pending.clear()

    for n in names:
        rgb = np.array(Image.open(os.path.join(rgb_dir, n + ".jpg")).convert("RGB"))
        mask = np.array(Image.open(os.path.join(mask_dir, n + ".png")))
        if mask.ndim != 2 or mask.dtype != np.uint8:
            raise ValueError(f"{scene}/{n}: the mask must be one 8-bit channel")
        image, mask, k = prepare_frame(rgb, mask, imu[n][1], target_resolution)
        image.save(os.path.join(dst, "images", n + ".webp"), **save_kw)
        intrinsics.append(k)
        if pending and pending[0][2].shape != mask.shape or len(pending) >= max(frames_per_call, 1):
            flush()
        pending.append((n, k, mask))
    flush()
    np.savez(os.path.join(dst, "scene_metadata.npz"), trajectories=np.stack([imu[n][0] for n in names]), intrinsics=np.stack(intrinsics),
             images=names)
    return len(names)


def main(argv=None, engine=None):
    """``engine``: with --device, an ``Engine`` to render on in place of one of the tool's own (it is left open)."""
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[1])
    ap.add_argument("root"); ap.add_argument("out")
    ap.add_argument("--scenes", nargs="+", required=True)
    ap.add_argument("--device", nargs="?", type=int, const=0, default=None)
    ap.add_argument("--target-resolution", type=int, default=920); ap.add_argument("--frames-per-call", type=int, default=8)
    ap.add_argument("--lossless", action="store_true"); ap.add_argument("--overwrite", action="store_true")
    a = ap.parse_args(argv)
    if not features.check("webp"):
        raise RuntimeError("this Pillow was built without WebP: the ScanNet++ loader reads only images/*.webp and normal/*.webp")
    if a.device is None:
        render, eng = render_mesh, None
    else:
        eng = None
        if engine is None:
            from unigeo_amd._lib import Engine                # raises without the library or a GPU
            engine = eng = Engine(a.device, workspace_bytes=512 << 20, persist_bytes=1 << 20)
        render = engine.prep_render_mesh
    total = 0
    try:
        for sc in a.scenes:
            if os.path.isfile(os.path.join(a.out, sc, "scene_metadata.npz")) and not a.overwrite:
                print(f"{sc}: scene_metadata.npz exists, kept")
                continue
            n = process_scene(a.root, a.out, sc, render, a.target_resolution, a.frames_per_call, {"lossless": True} if a.lossless else {})
            print(f"{sc}: {n} frames rendered")
            total += n
    finally:
        if eng is not None:
            eng.close()
    return total


if __name__ == "__main__":
    main()
