#!/usr/bin/env python
"""python tests/golden/make_rgbd_golden.py --reference <UniGeo checkout>
Golden for the RGB-D loaders of unigeo_amd/harness/rgbd.py: writes one tiny seeded scene per layout under
tests/golden/rgbd_scenes/<layout>/ in the file layout the reference reads, runs the REFERENCE's own ``*Sequence`` (metadata, gap, clip
split) and ``*Sample.load`` / ``postprocess`` classes on them and stores what they return in tests/golden/rgbd_golden.npz.  Third-party
modules the reference imports but these paths never call are stubbed.  Runs where the reference is checked out, never in a test.

Frames are 24 x 32, except Replica (24 x 40, so that the 4:3 crop removes four columns on each side) and ScanNetv2 (30 x 40 JPEG colour next
to 480 x 640 depth: the reference resizes the colour to 640 x 480 whatever its size).  Every scene holds a depth-0 pixel and one beyond the
20 m bound (65 m; not Bonn, whose 16-bit depth in 1/5000 m ends at 13.1 m); NeuralRGBD also holds raw 10000 and 10001 around its 10 m
pre-clamp and one invalid pose block.  The frame counts make the gap and the padded last clip show with clip_length = 3.

Per layout L the file holds L_ext, L_K, L_rgb, L_depth (paths relative to the scene), L_clip_keys, L_clip_ids - what the Sequence returns;
not for Bonn, whose ``boonSequence`` needs ``evo`` - and, for the first and the last clip (c0, c1), L_c<i>_<key> for every array of the
sample, L_c<i>_names, L_c<i>_scene and L_c<i>_keys (the sample's key order).  Bonn's sample is loaded by the reference's ``bonnSample`` on
the poses of this project's own TUM reader.  ScanNetv2's arrays are 480 x 640: the file keeps every 16th row and column of them (the two
special pixels lie on that grid) and the SHA-256 of the full images / cam_coord / mask bytes as L_c<i>_<key>_sha256."""
import argparse
import hashlib
import importlib.abc
import importlib.machinery
import os
import shutil
import sys
import types

import numpy as np
from PIL import Image

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(OUT, "rgbd_scenes")
SCENES = {"7scenes": "chess/seq-03", "bonn": "rgbd_bonn_balloon2", "neuralrgbd": "breakfast_room", "replica": "room_0", "scannetv2": "scene0707_00"}
CLIP = dict(clip_length=3, clip_overlap=0)
STRIDE = 16                                             # ScanNetv2: the sub-grid of the 480 x 640 arrays the golden keeps


class _Dummy:
    def __call__(self, *a, **k): return _Dummy()
    def __getattr__(self, k): return _Dummy()
    def __mro_entries__(self, bases): return (object,)


class _Any(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return _Dummy()


PREF = ("cv2", "open3d", "torchvision", "h5py", "skimage", "pytoml", "roma", "imageio", "matplotlib", "tensorboard",
        "wandb", "torch.utils.tensorboard", "evo", "trimesh", "pyrender")


class _Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path, target=None):
        if name.startswith(PREF):
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
    def create_module(self, spec):
        m = _Any(spec.name); m.__path__ = []; return m
    def exec_module(self, m): pass


def _pose(i, gl=False):
    """A slow pan: rotation about y and a little about x, drift along all axes; camera-to-world."""
    a, b = 0.05 * i, 0.02 * i
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    P = np.eye(4)
    P[:3, :3] = Ry @ Rx
    P[:3, 3] = [0.1 * i, 0.02 * i, (0.05 if gl else -0.05) * i]
    return P


def _rgb(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def _depth(rng, h, w, hi=6000, zero=(5, 5), far=(6, 6)):
    d = rng.integers(300, hi, (h, w)).astype(np.uint16)
    d[zero] = 0
    if far is not None:
        d[far] = 65000                                  # 65 m: beyond the 20 m bound
    return d


def write_7scenes(rng):
    d = os.path.join(ROOT, "7scenes", SCENES["7scenes"]); os.makedirs(d)
    for i in range(5):                                  # gap 1 -> 5 frames -> clips [0,1,2], [3,4,4]
        Image.fromarray(_rgb(rng, 24, 32)).save(os.path.join(d, f"frame-{i:06d}.color.png"))
        Image.fromarray(_depth(rng, 24, 32)).save(os.path.join(d, f"frame-{i:06d}.depth.proj.png"))
        np.savetxt(os.path.join(d, f"frame-{i:06d}.pose.txt"), _pose(i), fmt="%.7e", delimiter="\t")


def write_bonn(rng):
    from scipy.spatial.transform import Rotation
    d = os.path.join(ROOT, "bonn", SCENES["bonn"])
    for sub in ("rgb_110", "depth_110"):
        os.makedirs(os.path.join(d, sub))
    lines = ["# ground truth trajectory", "# timestamp tx ty tz qx qy qz qw"]
    for i in range(5):
        t = 1548266531.51903 + i / 30
        Image.fromarray(_rgb(rng, 24, 32)).save(os.path.join(d, "rgb_110", f"{t:.5f}.png"))
        Image.fromarray(_depth(rng, 24, 32, hi=60000, far=None)).save(os.path.join(d, "depth_110", f"{t + 0.011:.5f}.png"))
        P = _pose(i)
        q = Rotation.from_matrix(P[:3, :3]).as_quat() * 1.25                     # (x, y, z, w), deliberately not unit length
        lines.append(" ".join([f"{t:.4f}"] + [f"{v:.6f}" for v in P[:3, 3]] + [f"{v:.6f}" for v in q]))
    with open(os.path.join(d, "groundtruth_110.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def write_neuralrgbd(rng):
    d = os.path.join(ROOT, "neuralrgbd", SCENES["neuralrgbd"])
    for sub in ("images", "depth"):
        os.makedirs(os.path.join(d, sub))
    lines = []
    for i in range(13):                                 # block 4 invalid -> 12 valid -> every 3rd: img0, img3, img7, img10 -> clips [0,1,2], [3,3,3]
        Image.fromarray(_rgb(rng, 24, 32)).save(os.path.join(d, "images", f"img{i}.png"))
        dep = _depth(rng, 24, 32)
        dep[7, 7], dep[7, 8] = 10000, 10001             # the pre-clamp: 10.000 m stays, 10.001 m goes
        Image.fromarray(dep).save(os.path.join(d, "depth", f"depth{i}.png"))
        for row in _pose(i, gl=True):
            lines.append(" ".join(["nan"] * 4 if i == 4 else [f"{v:.8f}" for v in row]))
    with open(os.path.join(d, "poses.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def write_replica(rng):
    d = os.path.join(ROOT, "replica", SCENES["replica"], "imap", "00")
    for sub in ("rgb", "depth"):
        os.makedirs(os.path.join(d, sub))
    rows = []
    for i in range(11):                                 # unpadded numbers: rgb_10 sorts before rgb_2 by name; every 3rd: 0, 3, 6, 9
        Image.fromarray(_rgb(rng, 24, 40)).save(os.path.join(d, "rgb", f"rgb_{i}.png"))
        dep = _depth(rng, 24, 40, zero=(5, 9), far=(6, 10))
        dep[8, 1] = 0                                   # a hole the crop removes
        Image.fromarray(dep).save(os.path.join(d, "depth", f"depth_{i}.png"))
        rows.append(" ".join(f"{v:.8f}" for v in _pose(i, gl=True).reshape(-1)))
    with open(os.path.join(d, "traj_w_cgl.txt"), "w") as f:
        f.write("\n".join(rows) + "\n")


def write_scannetv2(rng):
    d = os.path.join(ROOT, "scannetv2", SCENES["scannetv2"])
    for sub in ("color_270", "depth_270", "intrinsic"):
        os.makedirs(os.path.join(d, sub))
    yy, xx = np.mgrid[0:480, 0:640]
    poses = []
    for i in range(7):                                  # gap 2 -> 0, 2, 4, 6 -> clips [0,1,2], [3,3,3]
        small = np.clip(127 + 90 * np.sin(np.mgrid[0:30, 0:40][1] / 6.0 + i)[..., None] + rng.normal(0, 20, (30, 40, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(small).save(os.path.join(d, "color_270", f"{i * 10:06d}.jpg"), quality=90)
        dep = (500 + 4 * xx + 3 * yy + 10 * i).astype(np.uint16)                 # a smooth ramp: a few KB as PNG
        dep[16, 32], dep[32, 48] = 0, 65000
        Image.fromarray(dep).save(os.path.join(d, "depth_270", f"{i * 10:06d}.png"))
        poses.append(_pose(i))
    np.savetxt(os.path.join(d, "pose_270.txt"), np.concatenate(poses, 0), fmt="%.8f")
    K = np.eye(4); K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 577.590698, 578.729797, 320.0, 240.0     # integer cy: y = -0 on row 240
    np.savetxt(os.path.join(d, "intrinsic", "intrinsic_depth.txt"), K, fmt="%.6f")


def _store(G, L, ci, out, root):
    sub = (lambda a: a[..., ::STRIDE, ::STRIDE]) if L == "scannetv2" else (lambda a: a)
    for k in ("images", "extrinsics", "intrinsics", "cam_coord", "world_coord", "mask"):
        a = np.stack([np.asarray(x) for x in out[k]])
        if L == "scannetv2" and k in ("images", "cam_coord", "mask"):
            G[f"{L}_c{ci}_{k}_sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())
        G[f"{L}_c{ci}_{k}"] = a if k in ("extrinsics", "intrinsics") else np.ascontiguousarray(sub(a))
    G[f"{L}_c{ci}_names"] = np.array(out["image_names"])
    G[f"{L}_c{ci}_scene"] = np.array(out["scene_name"])
    G[f"{L}_c{ci}_keys"] = np.array(list(out.keys()))
    assert out["_base"] == root and out["keyview_idx"] == 0 and out["caption"] == "" and "cam_normal" not in out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("UNIGEO_REFERENCE"), required="UNIGEO_REFERENCE" not in os.environ,
                    help="a checkout of the reference (UniGeo); it is only read")
    ref = ap.parse_args().reference
    shutil.rmtree(ROOT, ignore_errors=True)
    rng = np.random.default_rng(17)
    for w in (write_7scenes, write_bonn, write_neuralrgbd, write_replica, write_scannetv2):
        w(rng)
    sys.meta_path.insert(0, _Finder())
    sys.path.insert(0, ref)
    sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
    import dataset.bonn.bonn as bonn
    import dataset.neuralRGBD.neuralRGBD as nrgbd
    import dataset.replica.replica as replica
    import dataset.scannetv2.scannetv2 as sv2
    import dataset.sevenScenes.sevenScenes as seven
    from unigeo_amd.harness.rgbd import BonnLayout, RGBDSequence
    G = {}
    for L, seq_cls, sample_cls in (("7scenes", seven.SevenScenesSequence, seven.SevenScenesSample), ("bonn", None, bonn.bonnSample),
                                   ("neuralrgbd", nrgbd.neuralRGBDSequence, nrgbd.neuralRGBDSample),
                                   ("replica", replica.replicaSequence, replica.replicaSample), ("scannetv2", sv2.ScannetV2Sequence, sv2.ScannetV2Sample)):
        root, scene = os.path.join(ROOT, L), SCENES[L]
        if seq_cls is None:
            mine = RGBDSequence(root, scene, BonnLayout(), **CLIP)
            ext, K, rgb, depth, clips = mine.extrinsics, mine.intrinsics, mine.rgb_paths, mine.depth_paths, mine.clips
        else:
            seq = seq_cls(root, scene, **CLIP)
            ext, K, clips = seq.extrinsics, seq.intrinsics, seq.source_ids
            rgb, depth = ([os.path.relpath(p, os.path.join(root, scene)) for p in lst] for lst in (seq.rgb_path_list, seq.depth_path_list))
            G.update({f"{L}_ext": np.stack(ext), f"{L}_K": np.stack(K), f"{L}_rgb": np.array(rgb), f"{L}_depth": np.array(depth),
                      f"{L}_clip_keys": np.array(list(clips.keys())), f"{L}_clip_ids": np.array(list(clips.values()))})
        ids_all = list(clips.values())
        for ci, ids in enumerate((ids_all[0], ids_all[-1])):
            s = sample_cls(base=root, name=scene)
            s.data = {"images": [rgb[i] for i in ids], "poses": [ext[i] for i in ids], "intrinsics": [K[i] for i in ids],
                      "depth": [depth[i] for i in ids], "keyview_idx": 0}
            _store(G, L, ci, s.load(root), root)
    np.savez_compressed(os.path.join(OUT, "rgbd_golden.npz"), **G)
    print({k: v.shape for k, v in G.items()})


if __name__ == "__main__":
    main()
