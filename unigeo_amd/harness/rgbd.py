"""RGB-D clip loaders for 7-Scenes, Bonn, NeuralRGBD, Replica and ScanNetv2: one generic clip dataset and five
layout descriptions.

The reference has one loader per dataset (``dataset/{sevenScenes,bonn,neuralRGBD,replica,scannetv2}/*.py``), which are one algorithm with
five file layouts: read a 16-bit depth PNG, divide by a constant, back-project with VIEW 0's intrinsics in OpenGL convention
(``utils/geometry_utils.py:246-253`` + the y/z flip), move the points into the key view, mask ``nan | d < 1e-3 | d > 20``.  There are no
ground-truth normals: the samples carry no ``cam_normal`` / ``world_normal`` (the reference comments them out) unless ``normals="depth"``
asks for normals fitted to the depth (``harness/normals.py``).  A ``Layout`` supplies what
differs: file discovery and ordering, poses and intrinsics, the frame gap, the depth divisor, float32 or float64 depth arithmetic, an
optional depth pre-clamp, an optional colour pre-resize and an optional aspect-ratio crop.

Pinned by ``tests/golden/rgbd_golden.npz`` (what the reference's own ``*Sequence`` and ``*Sample`` classes return on the scenes under
``tests/golden/rgbd_scenes``): the sequence tables of four layouts and the native-size samples of all five.  UNPINNED: the Bonn TUM
trajectory reader (the reference reads it through ``evo``; restated here and tested against scipy) and, as for ScanNet++, the resize step.

Deliberate differences from the reference:
* the scene list is an argument (``scenes=[...]`` or ``split_file=``); the reference's ``splits/*.txt`` are not shipped with the package;
* a 7-Scenes / ScanNetv2 frame whose pose has a non-finite entry is dropped with its colour file, its depth file AND its pose
  (``sevenScenes.py:65-68`` drops the two files but keeps the pose, so its own length assertion fails);
* the TUM reader does not need ``evo``;
* Hypersim is not covered (its loader needs ``h5py``; no DepthCrafter configuration names it).

7-Scenes ships raw Kinect depth (``*.depth.png``), not the ``*.depth.proj.png`` files the reference's loader reads: its
``dataset/sevenScenes/preprocess.py`` writes those, offline.  ``sevenScenesDataset(register="host" | "device")`` reads the raw files and warps
them into the colour camera per clip (``register_depth`` here, ``ug_prep_register_depth`` on the GPU), bit-equal to the
reference's files (``tests/golden/register_golden.npz``).  Without ``register`` nothing changes.

``prep="device"`` keeps the file decode, ScanNetv2's Pillow pre-resize and the small tables on the host and runs the pixel arithmetic on the
GPU (``ug_prep_resize_frames`` / ``ug_prep_gt_ex``).  A crop needs no device code of its own: the tables carry its origin.
"""
import dataclasses
import glob
import os
import re
import threading
import time

import numpy as np
from PIL import Image

from .dataset import split_clips
from .normals import NORMALS_MODES, check_fit_options, fit_normals, world_normals
from .scannetpp import PREP_MODES, _backproject_gl, _resize, resize_pick, resize_taps

_GL_CV = np.float32([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]])
MAX_DEPTH = 20.0                   # "indoor scene": the mask bound of all five loaders
REGISTER_MODES = (None, "host", "device")
REGISTER_INVALID = ("keep", "drop")
RAW_SENTINEL = 65535               # 7-Scenes marks an invalid raw depth pixel with it
SEVEN_SCENES_SIZE = (480, 640)


@dataclasses.dataclass
class RegisterOpts:
    """``ug_register_opts`` of include/unigeo_hip.h without its flags.  The defaults are the 7-Scenes calibration: the depth focal length from
    the dataset's page, the colour focal length and the depth-to-colour transform from the Kinect calibration the reference's
    ``dataset/sevenScenes/preprocess.py`` cites, https://projet.liris.cnrs.fr/voir/activities-dataset/kinect-calibration.html"""
    src_focal: float = 585.0
    dst_focal: float = 525.0
    src2dst: tuple = (9.9996518012567637e-01, 2.6765126468950343e-03, -7.9041012313000904e-03, -2.5558943178152542e-02,
                      -2.7409311281316700e-03, 9.9996302803027592e-01, -8.1504520778013286e-03, 1.0109636268061706e-04,
                      7.8819942130445332e-03, 8.1718328771890631e-03, 9.9993554558014031e-01, 2.0318321729487039e-03)    # row-major 3x4
    divisor: float = 1000.0
    max_valid: float = 100.0


def _register_zbuf(frame, drop, o):
    """The z-buffer of one frame before the conversion to millimetres: float32 [H,W], 2000 where no point landed."""
    H, W = frame.shape
    m = [float(x) for x in np.asarray(o.src2dst, np.float64).reshape(-1)]
    sf, df = float(o.src_focal), float(o.dst_focal)
    d32 = frame.astype(np.float32) / np.float32(o.divisor)
    ok = (d32 > 0) & (d32 < np.float32(o.max_valid))
    if drop:
        ok &= frame != RAW_SENTINEL
    row, col = np.nonzero(ok)
    d = d32[ok].astype(np.float64)
    X = (((0.5 + col) - W / 2) / sf) * d
    Y = (((0.5 + row) - H / 2) / sf) * d
    x3 = ((m[0] * X + m[1] * Y) + m[2] * d) + m[3]
    y3 = ((m[4] * X + m[5] * Y) + m[6] * d) + m[7]
    z3 = ((m[8] * X + m[9] * Y) + m[10] * d) + m[11]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        xi = np.rint(((x3 / z3) * df) + W / 2)                   # ties to even, as Python's round
        yi = np.rint(((y3 / z3) * df) + H / 2)
        keep = (xi >= 0) & (yi >= 0) & (yi < H) & (xi < W)       # as float64, before any integer cast; a NaN is dropped
        zbuf = np.full(H * W, 2000.0, np.float32)
        np.minimum.at(zbuf, yi[keep].astype(np.int64) * W + xi[keep].astype(np.int64), z3[keep].astype(np.float32))
    return zbuf.reshape(H, W)


def register_depth(raw_u16, invalid="keep", opts=None):
    """Raw depth warped into the colour camera: the host mirror of ``ug_prep_register_depth`` (the arithmetic is documented operation by
    operation in include/unigeo_hip.h) and a restatement of ``preprocess.py:82-140`` without its loop over the pixels.  ``raw_u16``: uint16
    ``[H,W]`` or ``[T,H,W]`` -> uint16 of the same shape.  Element-wise float64 steps in the reference's order - its one matrix product is
    written out left to right, which reproduces its files -, ``np.minimum.at`` for the z-buffer, and its ``astype(uint16)`` of values past
    65535 as the modulo it is.  ``invalid="drop"`` leaves raw 65535 out (UNPINNED: the reference has no such mode); ``"keep"`` lets it take
    part as 65.535 m, as the reference does."""
    if invalid not in REGISTER_INVALID:
        raise ValueError(f"invalid must be one of {list(REGISTER_INVALID)}, not {invalid!r}")
    o = RegisterOpts() if opts is None else opts
    raw = np.asarray(raw_u16)
    if raw.dtype != np.uint16 or raw.ndim not in (2, 3):
        raise ValueError("register_depth: raw depth must be uint16 [H,W] or [T,H,W]")
    if np.asarray(o.src2dst).size != 12:
        raise ValueError("register_depth: src2dst holds 12 numbers, the top three rows of the transform")
    clip = raw if raw.ndim == 3 else raw[None]
    out = np.empty(clip.shape, np.uint16)
    for t, frame in enumerate(clip):
        zbuf = _register_zbuf(frame, invalid == "drop", o)
        zbuf[zbuf > np.float32(1000.0)] = 0
        with np.errstate(over="ignore", invalid="ignore"):
            v = np.float32(1000.0) * zbuf
            v = np.where((v > -2.0 ** 31) & (v < 2.0 ** 31), v, np.float32(0))     # outside int32: 0 (custom options only)
        out[t] = (v.astype(np.int64) % 65536).astype(np.uint16)
    return out if raw.ndim == 3 else out[0]


def _sorted_glob(base, pattern, number=None):
    """Paths relative to ``base``; sorted by name, or by the integer ``number`` (a regex with one group) finds in them (0 without a match)."""
    files = glob.glob(os.path.join(base, pattern))
    if number is None:
        files = sorted(files)
    else:
        def key(f):
            m = re.search(number, f)
            return int(m.group(1)) if m else 0
        files = sorted(files, key=key)
    return [os.path.relpath(f, base) for f in files]


def _cv_c2w_to_gl_w2c(c2w):
    """OpenCV camera-to-world -> OpenGL world-to-camera: ``inv(F c2w F)``, ``F = diag(1,-1,-1,1)`` in float32 (sevenScenes.py:57-63)."""
    return np.linalg.inv(np.einsum("ij,njk,kl->nil", _GL_CV, c2w, _GL_CV))


def _drop_bad_poses(c2w, *lists):
    """Frames whose pose has a non-finite entry leave all the lists together (a deliberate difference, see the module docstring)."""
    ok = np.isfinite(c2w).all(axis=(1, 2))
    return (c2w[ok],) + tuple([x for x, m in zip(lst, ok) if m] for lst in lists)


def _same_length(base, **named):
    lens = {k: len(v) for k, v in named.items()}
    if len(set(lens.values())) != 1:
        raise ValueError(f"{base}: {lens} disagree in length")


def read_tum_trajectory(path):
    """TUM trajectory file (``t tx ty tz qx qy qz qw`` per line, ``#`` comments) -> (timestamps [N], camera-to-world [N,4,4]), float64.
    UNPINNED: the reference reads the file through ``evo``; this restates it - the quaternion is normalised and the rotation built from
    ``(qw, qx, qy, qz)`` - and is tested against ``scipy.spatial.transform.Rotation.from_quat``."""
    rows = []
    with open(path) as f:
        for ln in f:
            ln = ln.strip()
            if not ln or ln.startswith("#"):
                continue
            v = [float(x) for x in ln.replace(",", " ").split()]
            if len(v) != 8:
                raise ValueError(f"{path}: a TUM pose line has 8 numbers, not {len(v)}: {ln!r}")
            rows.append(v)
    if not rows:
        raise ValueError(f"{path}: no poses")
    a = np.array(rows, np.float64)
    q = a[:, 4:] / np.linalg.norm(a[:, 4:], axis=1, keepdims=True)
    x, y, z, w = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    T = np.tile(np.eye(4), (len(a), 1, 1))
    T[:, :3, :3] = R
    T[:, :3, 3] = a[:, 1:4]
    return a[:, 0], T


def crop_to_aspect(h, w, aspect):
    """``crop_image_and_adjust_intrinsics`` of utils/geometry_utils.py:257-291: the centred crop box (x1, y1, x2, y2) of aspect ``w / h``."""
    if w / h > aspect:
        nw = int(h * aspect)
        x1 = (w - nw) // 2
        return x1, 0, x1 + nw, h
    nh = int(w / aspect)
    y1 = (h - nh) // 2
    return 0, y1, w, y1 + nh


class Layout:
    """What differs between the five loaders.  ``discover(base)`` -> (world-to-camera OpenGL [N,4,4], intrinsics [N,3,3], colour paths,
    depth paths), the paths relative to ``base = <root>/<scene>``, before the frame gap is applied."""

    base_dataset = None
    gap = 1
    depth_divisor = 1000.0
    depth_f64 = False                  # Bonn: the depth stays float64 through the back-projection
    clamp_depth = None                 # NeuralRGBD: d > clamp -> 0 and d < 1e-3 -> 0 before the back-projection
    color_size = None                  # ScanNetv2: (width, height) the colour image is resized to with Pillow's default filter
    crop_aspect = None                 # Replica: centred crop to this width / height AFTER the back-projection
    raw_size = None                    # 7-Scenes: (height, width) of the raw depth that ``register=`` warps into the colour camera; None: no such step

    def discover(self, base):
        raise NotImplementedError

    @property
    def max_depth(self):               # what the mask sees: the pre-clamp turns d > clamp into 0, which d < 1e-3 masks
        return MAX_DEPTH if self.clamp_depth is None else min(MAX_DEPTH, self.clamp_depth)


class SevenScenesLayout(Layout):
    """sevenScenes.py:48-72: ``*.color.png`` / ``*.depth.proj.png`` / ``*.pose.txt`` (OpenCV camera-to-world) sorted by name.
    ``raw_depth=True``: the depth files are the dataset's own ``*.depth.png`` (a pattern that does not match ``*.depth.proj.png``), which the
    dataset registers to the colour camera itself."""
    base_dataset = "7scenes"
    raw_size = SEVEN_SCENES_SIZE

    def __init__(self, raw_depth=False):
        self.depth_pattern = "*.depth.png" if raw_depth else "*.depth.proj.png"

    def discover(self, base):
        rgb, depth, pose = (_sorted_glob(base, p) for p in ("*.color.png", self.depth_pattern, "*.pose.txt"))
        _same_length(base, colour=rgb, depth=depth, poses=pose)
        if not rgb:
            return np.zeros((0, 4, 4)), np.zeros((0, 3, 3)), rgb, depth
        c2w = np.stack([np.genfromtxt(os.path.join(base, p)) for p in pose], axis=0)
        c2w, rgb, depth = _drop_bad_poses(c2w, rgb, depth)
        K = np.array([[525, 0, 320], [0, 525, 240], [0, 0, 1]], np.float64)
        return _cv_c2w_to_gl_w2c(c2w), np.tile(K, (len(rgb), 1, 1)), rgb, depth


class ScannetV2Layout(Layout):
    """scannetv2.py:48-73,108-114: ``color_270/*.jpg`` (resized to the depth's 640 x 480), ``depth_270/*.png``, ``pose_270.txt`` (4 rows per
    OpenCV camera-to-world matrix), ``intrinsic/intrinsic_depth.txt``."""
    base_dataset = "scannetv2"
    gap = 2
    color_size = (640, 480)

    def discover(self, base):
        rgb, depth = _sorted_glob(base, "color_270/*.jpg"), _sorted_glob(base, "depth_270/*.png")
        c2w = np.genfromtxt(os.path.join(base, "pose_270.txt")).reshape(-1, 4, 4)
        _same_length(base, colour=rgb, depth=depth, poses=c2w)
        c2w, rgb, depth = _drop_bad_poses(c2w, rgb, depth)
        K = np.genfromtxt(os.path.join(base, "intrinsic", "intrinsic_depth.txt")).reshape(4, 4)[:3, :3]
        return _cv_c2w_to_gl_w2c(c2w), np.tile(K, (len(rgb), 1, 1)), rgb, depth


class BonnLayout(Layout):
    """bonn.py:48-79,123-134: ``rgb_110/*.png``, ``depth_110/*.png``, ``groundtruth_110.txt`` (TUM, OpenCV camera-to-world); depth in 1/5000 m,
    float64 through the back-projection, a raw 0 is NaN."""
    base_dataset = "bonn"
    depth_divisor = 5000.0
    depth_f64 = True

    def discover(self, base):
        rgb, depth = _sorted_glob(base, "rgb_110/*.png"), _sorted_glob(base, "depth_110/*.png")
        _, c2w = read_tum_trajectory(os.path.join(base, "groundtruth_110.txt"))
        _same_length(base, colour=rgb, depth=depth, poses=c2w)
        K = np.array([[542.822841, 0, 315.593520], [0, 542.576870, 237.756098], [0, 0, 1]])
        return _cv_c2w_to_gl_w2c(c2w), np.tile(K, (len(rgb), 1, 1)), rgb, depth


class ReplicaLayout(Layout):
    """replica.py:48-85,150-168: ``imap/00/rgb/rgb_<n>.png`` / ``imap/00/depth/depth_<n>.png`` ordered by ``<n>``, ``imap/00/traj_w_cgl.txt``
    (OpenGL camera-to-world, 16 numbers per line); cropped to 4:3 after the back-projection."""
    base_dataset = "replica"
    gap = 3
    crop_aspect = 4 / 3

    def discover(self, base):
        rgb = _sorted_glob(base, "imap/00/rgb/*.png", r"rgb_(\d+)\.png")
        depth = _sorted_glob(base, "imap/00/depth/*.png", r"depth_(\d+)\.png")
        c2w = np.loadtxt(os.path.join(base, "imap", "00", "traj_w_cgl.txt"), delimiter=" ").reshape([-1, 4, 4])
        _same_length(base, colour=rgb, depth=depth, poses=c2w)
        K = np.array([[600.0, 0, 599.5], [0, 600.0, 339.5], [0, 0, 1]], np.float32)
        return np.linalg.inv(c2w), np.tile(K, (len(rgb), 1, 1)), rgb, depth


class NeuralRGBDLayout(Layout):
    """neuralRGBD.py:48-102,145-155: ``images/img<n>.png`` / ``depth/depth<n>.png`` ordered by ``<n>``, ``poses.txt`` (4 lines per OpenGL
    camera-to-world matrix in float32; a block whose first line holds ``nan`` is invalid and its frame is removed BEFORE the gap)."""
    base_dataset = "neuralRGBD"
    gap = 3
    clamp_depth = 10.0

    def discover(self, base):
        rgb = _sorted_glob(base, "images/*.png", r"img(\d+)\.png")
        depth = _sorted_glob(base, "depth/*.png", r"depth(\d+)\.png")
        with open(os.path.join(base, "poses.txt")) as f:
            lines = f.readlines()
        poses, valid = [], []
        for i in range(0, len(lines), 4):
            valid.append("nan" not in lines[i])
            poses.append([[float(x) for x in ln.split()] for ln in lines[i:i + 4]] if valid[-1] else np.eye(4).tolist())
        poses = np.array(poses, np.float32)
        _same_length(base, colour=rgb, depth=depth, poses=poses)
        w2c = [np.linalg.inv(p) for p, m in zip(poses, valid) if m]
        rgb, depth = ([x for x, m in zip(lst, valid) if m] for lst in (rgb, depth))
        K = np.array([[554.2562584220408, 0, 320], [0, 554.2562584220408, 240], [0, 0, 1]], np.float32)
        return np.stack(w2c) if w2c else np.zeros((0, 4, 4), np.float32), np.tile(K, (len(rgb), 1, 1)), rgb, depth


class RGBDSequence:
    """One scene of a layout: poses (world-to-camera, OpenGL), intrinsics, file paths relative to the scene and the clip table."""

    def __init__(self, root, scene_name, layout, clip_length=30, clip_overlap=0):
        base = os.path.join(root, scene_name)
        if not os.path.isdir(base):
            raise FileNotFoundError(f"{layout.base_dataset} scene not found: {base}")
        ext, K, rgb, depth = layout.discover(base)
        if not rgb:
            raise FileNotFoundError(f"{layout.base_dataset} scene holds no frames: {base}")
        g = layout.gap
        self.root, self.scene_name, self.layout = root, scene_name, layout
        self.extrinsics, self.intrinsics = ext[::g], K[::g]
        self.rgb_paths, self.depth_paths = rgb[::g], depth[::g]
        self.clips = split_clips(len(self.rgb_paths), clip_length, clip_overlap)


def _open_rgb(path, layout):
    im = Image.open(path)
    if layout.color_size is not None:
        im = im.resize(layout.color_size)                       # Pillow's default filter (bicubic), scannetv2.py:112
    a = np.array(im)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{path}: the colour image must decode to 8-bit RGB")
    return a


def _open_depth(path):
    d = np.array(Image.open(path))
    if d.ndim != 2:
        raise ValueError(f"{path}: the depth image must have one channel")
    if d.dtype != np.uint16:
        if d.min() < 0 or d.max() > 65535:
            raise ValueError(f"{path}: depth does not fit 16 bits")
        d = d.astype(np.uint16)
    return d


def decode_clip(root, seq, ids):
    """The file decode alone: (frames uint8 [T,H,W,3] - after the layout's colour pre-resize -, depth uint16 [T,H,W])."""
    base = os.path.join(root, seq.scene_name)
    frames = np.stack([_open_rgb(os.path.join(base, seq.rgb_paths[i]), seq.layout) for i in ids])
    depth = np.stack([_open_depth(os.path.join(base, seq.depth_paths[i])) for i in ids])
    if depth.shape != frames.shape[:3]:
        raise ValueError(f"{base}: depth and images differ in size")
    return frames, depth


def decode_depth(root, seq, ids):
    """The depth files of a clip alone: uint16 [T,H,W]."""
    base = os.path.join(root, seq.scene_name)
    return np.stack([_open_depth(os.path.join(base, seq.depth_paths[i])) for i in ids])


def depth_metres(raw, layout):
    """The layout's depth arithmetic on a decoded depth image, before the back-projection."""
    raw = np.asarray(raw).astype(np.float32)
    if layout.depth_f64:                                        # bonn.py:125-130
        d = raw.astype(np.float64) / layout.depth_divisor
        d[raw == 0] = np.nan
        return d
    d = raw / layout.depth_divisor
    if layout.clamp_depth is not None:                          # neuralRGBD.py:149-151
        d[d > layout.clamp_depth] = 0
        d[d < 1e-3] = 0
    return d


def _crop_box(layout, h, w):
    return (0, 0, w, h) if layout.crop_aspect is None else crop_to_aspect(h, w, layout.crop_aspect)


def _assemble(root, seq, ids, keyview_idx, images, ext, K, cam, world, mask, normals=None):
    """The sample dict in the reference's key order (``*Sample.load`` + ``postprocess``).  ``normals = (cam_normal, world_normal,
    normal_mask)``: the first two go where the reference's loaders have them commented out, ``normal_mask`` follows ``mask``."""
    ref_inv = np.linalg.inv(ext[keyview_idx])
    out = {"_base": root, "scene_name": "_".join(seq.scene_name.split("/")), "images": images,
           "image_names": [os.path.basename(seq.rgb_paths[i]) for i in ids], "extrinsics": [e @ ref_inv for e in ext], "intrinsics": K,
           "keyview_idx": keyview_idx}
    if normals is not None:
        out["cam_normal"] = normals[0]
    out.update({"cam_coord": cam, "caption": ""})
    if normals is not None:
        out["world_normal"] = normals[1]
    out.update({"world_coord": world, "mask": mask})
    if normals is not None:
        out["normal_mask"] = normals[2]
    return out


def _clip_cameras(seq, ids, box):
    """float32 poses, per-frame intrinsics (uncropped and shifted by the crop origin)."""
    ext = [np.asarray(seq.extrinsics[i]).astype(np.float32) for i in ids]
    K = [np.asarray(seq.intrinsics[i]).astype(np.float32) for i in ids]
    Kc = []
    for k in K:
        k = k.copy()
        k[0, 2] -= box[0]
        k[1, 2] -= box[1]
        Kc.append(k)
    return ext, K, Kc


def _masked_frame(c):
    """The loaders' validity rule on a whole back-projected frame: (``c`` with the bad pixels zeroed - a copy -, ``bad``)."""
    bad = np.isnan(c).any(axis=0)
    d = -1 * c[2]
    d[np.isnan(d)] = 0
    bad = bad | (d < 1e-3) | (d > MAX_DEPTH)
    c = c.copy()
    c[:, bad] = 0
    return c, bad


def load_clip(root, seq, ids, keyview_idx=0, depth=None, normals=None):
    """One clip at native size on the host: the reference's ``*Sample.load`` + ``postprocess``, step for step.  ``depth`` (uint16 ``[T,H,W]``)
    stands in for the depth files: the registered clip of ``sevenScenesDataset(register=...)``.  ``normals = (radius, edge, min_count)``:
    the sample also carries ``cam_normal`` / ``world_normal`` / ``normal_mask``, fitted to the full native frame before the crop
    (``harness/normals.py``)."""
    layout, base = seq.layout, os.path.join(root, seq.scene_name)
    frames = [_open_rgb(os.path.join(base, seq.rgb_paths[i]), layout) for i in ids]
    h, w = frames[0].shape[:2]
    x1, y1, x2, y2 = box = _crop_box(layout, h, w)
    ext, K, Kc = _clip_cameras(seq, ids, box)
    ref = ext[keyview_idx]
    images, cam, world, masks = [], [], [], []
    fitted = None if normals is None else ([], [], [])
    for j, i in enumerate(ids):
        images.append(frames[j].astype(np.float32).transpose(2, 0, 1)[:, y1:y2, x1:x2])
        raw = _open_depth(os.path.join(base, seq.depth_paths[i])) if depth is None else depth[j]
        c = _backproject_gl(depth_metres(raw, layout), K[0])     # view 0's intrinsics for all views, uncropped, on the full frame
        M = ref @ np.linalg.inv(ext[j])                          # source camera -> key-view camera
        wc = (np.matmul(M[:3, :3], c.reshape(3, -1)) + M[:3, 3][:, None]).reshape(c.shape)
        if fitted is not None:
            full, full_bad = _masked_frame(c)
            n, nm = fit_normals(full, ~full_bad, *normals)
            for lst, a in zip(fitted, (n, world_normals(n, M), nm)):
                lst.append(np.ascontiguousarray(a[..., y1:y2, x1:x2]))
        c, wc = c[:, y1:y2, x1:x2], wc[:, y1:y2, x1:x2]
        c, bad = _masked_frame(c)
        wc[:, bad] = 0
        cam.append(c); world.append(wc); masks.append((~bad).astype(np.float32))
    return _assemble(root, seq, ids, keyview_idx, images, ext, Kc, cam, world, masks, fitted)


class RGBDClipDataset:
    """Clip-level dataset in the unified sample format over one ``Layout``; constructor, keys, dtypes and shapes as ``ScannetPPDataset``,
    without ``cam_normal`` / ``world_normal``.  ``scenes=[...]`` or ``split_file=`` (one scene per line, e.g. a UniGeo checkout's
    ``dataset/<name>/splits/test.txt``) names the scenes; ``"all"`` is not accepted because scene names can be nested (``chess/seq-03``).
    ``prep="device"`` runs the resizes and the ground truth on the GPU; there is no fallback to the host path.
    ``register="host" | "device"`` (7-Scenes only; anywhere else it is a ``ValueError``): the scene holds raw depth, which is warped into the
    colour camera per clip before anything else sees it - on the host (``register_depth``) or on the dataset's engine (no fallback);
    ``register_invalid="drop"`` leaves the raw 65535 marker out of it.
    ``normals="depth"`` (default ``None``: nothing changes) adds ``cam_normal`` / ``world_normal`` (lists of float32 ``[3,H,W]``) and
    ``normal_mask`` (float32 ``[H,W]``): normals fitted to the depth on the full native frame (``harness/normals.py``'s ``fit_normals`` with
    ``normals_radius`` / ``normals_edge`` / ``normals_min_count``; ``ug_prep_gt_normals`` under ``prep="device"``, bit-equal, no fallback),
    cropped and resized like ``cam_coord``.  With ``register=`` the registered depth feeds the fit."""

    layout = None

    def __init__(self, root, scenes=None, split_file=None, split="test", clip_length=17, clip_overlap=0,
                 input_size=None, target_size=None, verbose=False, prep="host", device_id=0, engine=None, register=None,
                 register_invalid="keep", normals=None, normals_radius=2, normals_edge=0.05, normals_min_count=None, **_):
        if prep not in PREP_MODES:
            raise ValueError(f"prep must be one of {list(PREP_MODES)}, not {prep!r}")
        if register not in REGISTER_MODES:
            raise ValueError(f"register must be one of {list(REGISTER_MODES)}, not {register!r}")
        if register_invalid not in REGISTER_INVALID:
            raise ValueError(f"register_invalid must be one of {list(REGISTER_INVALID)}, not {register_invalid!r}")
        if register is not None:
            if self.layout.raw_size is None:
                raise ValueError(f"{self.layout.base_dataset}: register= is for 7-Scenes' raw depth; this dataset's depth needs no registration")
            self.layout = type(self.layout)(raw_depth=True)     # this dataset's own layout: the class attribute keeps the default pattern
        if normals not in NORMALS_MODES:
            raise ValueError(f"normals must be one of {list(NORMALS_MODES)}, not {normals!r}")
        self.normals = normals
        # without normals= the three options are not looked at, as before they existed
        self.normals_opts = None if normals is None else check_fit_options(normals_radius, normals_edge, normals_min_count,
                                                                            "normals_radius / normals_edge / normals_min_count")
        self.register, self.register_invalid = register, register_invalid
        self.prep, self.device_id, self.engine = prep, device_id, engine
        self._lock = threading.Lock()
        self.last_timing = None                             # seconds of the last sample's stages: prep="device" decode / resize / gt (/ normals), register= register
        name = self.layout.base_dataset
        if root is None or not os.path.isdir(root):
            raise FileNotFoundError(f"{name} root not found: {root!r}")
        if isinstance(scenes, str):
            raise ValueError(f"{name}: scenes must be a list of scene names (they can be nested, e.g. 'chess/seq-03'), not {scenes!r}")
        if scenes is None:
            if split_file is None:
                raise FileNotFoundError(f"{name}: no scene list; pass scenes=[...] or split_file=<one scene per line>")
            if not os.path.isfile(split_file):
                raise FileNotFoundError(f"{name} split list not found: {split_file} (pass split_file=... or scenes=[...])")
            with open(split_file) as f:
                scenes = [ln.strip() for ln in f.read().splitlines() if ln.strip()]
        self.root, self.split = root, split
        self.input_size, self.target_size = input_size, target_size
        self.samples = []
        for sc in scenes:
            seq = RGBDSequence(root, sc, self.layout, clip_length, clip_overlap)
            if verbose:
                print(f"sequence name: {sc}, num_seq: {len(seq.rgb_paths)}")
            for key, ids in seq.clips.items():
                self.samples.append((seq, key, ids))

    @property
    def base_dataset(self):
        return self.layout.base_dataset

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, index):
        if index >= len(self.samples):
            raise IndexError(index)
        seq, _, ids = self.samples[index]
        if self.prep == "device":
            out = self._load_clip_device(seq, ids)
        else:
            fit = self.normals_opts if self.normals is not None else None
            if self.register is None:
                out = load_clip(self.root, seq, ids, normals=fit)
            else:
                raw = decode_depth(self.root, seq, ids)
                t0 = time.perf_counter()
                depth = self._register(raw)
                self.last_timing = {"register": time.perf_counter() - t0}
                out = load_clip(self.root, seq, ids, depth=depth, normals=fit)
            if self.input_size is not None:
                ht, wd = self.input_size
                oh, ow = out["images"][0].shape[-2:]
                out["images"] = [_resize(im, ht, wd, 1, True) for im in out["images"]]
                scale = np.array([[wd / ow] * 3, [ht / oh] * 3, [1.0] * 3], np.float32)
                out["intrinsics"] = [k * scale for k in out["intrinsics"]]
            if self.target_size is not None:
                ht, wd = self.target_size
                for attr in ("cam_coord", "world_coord", "mask") + (("cam_normal", "world_normal", "normal_mask") if fit is not None else ()):
                    out[attr] = [_resize(x, ht, wd, 0, False) for x in out[attr]]
        out["_index"] = index
        out["_dataset"] = self.base_dataset
        return out

    def _device_engine(self):
        if self.engine is None:
            from .._lib import Engine                        # raises without the library or a GPU: no host fallback
            self.engine = Engine(self.device_id, workspace_bytes=256 << 20, persist_bytes=1 << 20)
        return self.engine

    def _register(self, raw):
        """The raw depth clip warped into the colour camera, on the host or on the dataset's engine."""
        if raw.shape[1:] != self.layout.raw_size:
            raise ValueError(f"{self.base_dataset}: register= expects raw depth of {self.layout.raw_size[0]} x {self.layout.raw_size[1]}, "
                             f"not {raw.shape[1]} x {raw.shape[2]}")
        if self.register == "host":
            return register_depth(raw, self.register_invalid)
        with self._lock:
            return self._device_engine().prep_register_depth(raw, invalid=self.register_invalid)

    def _load_clip_device(self, seq, ids, keyview_idx=0):
        """``load_clip`` + the two resizes with the pixel arithmetic on the GPU: same keys, shapes and dtypes.  The crop is in the tables:
        taps and picks are built for the cropped length and shifted by the crop origin, so the mirror extension reflects at the crop's edge."""
        layout = seq.layout
        t0 = time.perf_counter()
        frames, depth = decode_clip(self.root, seq, ids)
        t1 = time.perf_counter()
        if self.register is not None:
            depth = self._register(depth)
        tr = time.perf_counter() - t1
        t1 += tr
        T, hi, wi = depth.shape
        x1, y1, x2, y2 = box = _crop_box(layout, hi, wi)
        ch, cw = y2 - y1, x2 - x1
        ext, K, Kc = _clip_cameras(seq, ids, box)
        ref = ext[keyview_idx]
        M = np.stack([ref @ np.linalg.inv(e) for e in ext]).astype(np.float32)
        K0 = np.broadcast_to(K[0], (T, 3, 3))
        ih, iw = self.input_size if self.input_size is not None else (ch, cw)
        th, tw = self.target_size if self.target_size is not None else (ch, cw)
        (ri, rw), (ci, cwt) = resize_taps(ch, ih), resize_taps(cw, iw)
        with self._lock:
            eng = self._device_engine()
            images = eng.prep_resize_frames(frames, ih, iw, row_taps=(ri + y1, rw), col_taps=(ci + x1, cwt))
            t2 = time.perf_counter()
            rows, cols, gt_kw = y1 + resize_pick(ch, th), x1 + resize_pick(cw, tw), dict(
                depth_divisor=layout.depth_divisor, max_depth=layout.max_depth, depth_f64=layout.depth_f64, zoomed=(th, tw) != (ch, cw))
            _, cc, _, wc, mask = eng.prep_gt(depth, None, K0, M, rows, cols, **gt_kw)
            t3 = time.perf_counter()
            fitted = None
            if self.normals is not None:
                r, e, mc = self.normals_opts
                fitted = tuple(list(a) for a in eng.prep_gt_normals(depth, K0, M, rows, cols, radius=r, edge=e, min_count=mc, **gt_kw))
            t4 = time.perf_counter()
        self.last_timing = {"decode": t1 - tr - t0, "resize": t2 - t1, "gt": t3 - t2}
        if self.normals is not None:
            self.last_timing["normals"] = t4 - t3
        if self.register is not None:
            self.last_timing["register"] = tr
        if self.input_size is not None:
            scale = np.array([[iw / cw] * 3, [ih / ch] * 3, [1.0] * 3], np.float32)
            Kc = [k * scale for k in Kc]
        return _assemble(self.root, seq, ids, keyview_idx, list(images), ext, Kc, list(cc), list(wc), list(mask), fitted)


class sevenScenesDataset(RGBDClipDataset):
    layout = SevenScenesLayout()


class bonnDataset(RGBDClipDataset):
    layout = BonnLayout()


class neuralRGBDDataset(RGBDClipDataset):
    layout = NeuralRGBDLayout()


class replicaDataset(RGBDClipDataset):
    layout = ReplicaLayout()


class ScannetV2Dataset(RGBDClipDataset):
    layout = ScannetV2Layout()


LAYOUTS = {"7scenes": sevenScenesDataset, "bonn": bonnDataset, "neuralrgbd": neuralRGBDDataset, "replica": replicaDataset,
           "scannetv2": ScannetV2Dataset}
