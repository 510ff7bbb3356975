"""ScanNet++ clip loader - the sample format either side of the hot path.

Restates, for the processed ScanNet++ layout (``<root>/<scene>/{scene_metadata.npz, images/*.webp, normal/*.webp,
depth/*.png}``):

* sequence metadata + frame sub-sampling + clip split  - ``/root/reference/dataset/scannetpp/scannetpp.py:16-69``
  (OpenCV camera-to-world trajectories -> OpenGL world-to-camera, every 3rd frame, clips every
  ``clip_length - clip_overlap`` frames with the tail padded by its last frame);
* per-clip sample load                                 - ``scannetpp.py:81-135`` (RGB float32 CHW 0..255, normals
  ``x/255*2-1`` with all-zero pixels invalid, depth in mm -> back-projected with the FIRST view's intrinsics,
  flipped to OpenGL);
* post-processing                                      - ``scannetpp.py:140-187`` (world = key-view frame, validity
  mask 1e-3 <= depth <= 80 and finite, extrinsics relative to the key view);
* input / target resizing                              - ``dataset/dataset_core/transforms.py:38-110`` and
  ``dataset/dataset_core/dataset.py:167-170`` (inputs: order-1 with anti-aliasing + intrinsics scaling; targets:
  order-0, no anti-aliasing).

Pinned by ``tests/golden/scannetpp_golden.npz`` (outputs of the reference's own classes on the synthetic scene in
``tests/golden/scannetpp_scene``).  The resize step follows scikit-image's published ``transform.resize`` recipe
(gaussian pre-filter sigma=(s-1)/2 when down-scaling, ``scipy.ndimage.zoom(grid_mode=True, mode='mirror')``) through
scipy; scikit-image itself is not installed here, so that step is UNPINNED (native-size loads are bit-exact vs the reference).

``prep="device"`` keeps the file decode and the small tables here and runs the pixel arithmetic on the GPU:
``resize_taps`` / ``resize_pick`` state the two resizes as per-axis tables, ``resize_restated`` is their float64 evaluation on the host.
"""
import os
import threading
import time

import numpy as np
from PIL import Image

from .dataset import split_clips

_GL_CV = np.float32([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]])
FRAME_GAP = 3                      # scannetpp.py:24-30


class ScannetPPSequence:
    """One scene: poses (world-to-camera, OpenGL), intrinsics, relative file paths and the clip table."""

    def __init__(self, root, scene_name, clip_length=30, clip_overlap=0, gap=FRAME_GAP):
        meta_path = os.path.join(root, scene_name, "scene_metadata.npz")
        if not os.path.isfile(meta_path):
            raise FileNotFoundError(f"ScanNet++ scene metadata missing: {meta_path}")
        with np.load(meta_path) as meta:
            c2w_cv = meta["trajectories"]
            K = meta["intrinsics"]
            names = meta["images"].tolist()
        if not (len(c2w_cv) == len(K) == len(names)):
            raise ValueError(f"{meta_path}: trajectories / intrinsics / images disagree in length")
        w2c_gl = np.linalg.inv(np.einsum("ij,njk,kl->nil", _GL_CV, c2w_cv, _GL_CV))
        self.root, self.scene_name = root, scene_name
        self.extrinsics = w2c_gl[::gap]
        self.intrinsics = K[::gap]
        self.rgb_paths = [os.path.join("images", n + ".webp") for n in names][::gap]
        self.normal_paths = [os.path.join("normal", n + ".webp") for n in names][::gap]
        self.depth_paths = [os.path.join("depth", n + ".png") for n in names][::gap]
        self.clips = split_clips(len(self.rgb_paths), clip_length, clip_overlap)


def _backproject_gl(depth_m, K):
    """utils/geometry_utils.py:246-253 followed by the y/z flip of scannetpp.py:126-127; [3,H,W] float32."""
    h, w = depth_m.shape
    u, v = np.meshgrid(np.arange(w), np.arange(h), indexing="xy")
    x = (u - K[0, 2]) * depth_m / K[0, 0]
    y = (v - K[1, 2]) * depth_m / K[1, 1]
    return np.stack((x, -y, -depth_m), axis=0).astype(np.float32)


def _resize(x, ht, wd, order, anti_alias):
    """scikit-image ``resize`` recipe on the last two axes (mode='reflect' == ndimage 'mirror')."""
    from scipy import ndimage as ndi
    h, w = x.shape[-2:]
    if (h, w) == (ht, wd):
        return x
    lead = x.ndim - 2
    y = x.astype(np.float64) if x.dtype != np.float32 else x
    if anti_alias:
        sig = [0.0] * lead + [max(0.0, (h / ht - 1) / 2), max(0.0, (w / wd - 1) / 2)]
        if any(s > 0 for s in sig):
            y = ndi.gaussian_filter(y, sig, mode="mirror")
    return ndi.zoom(y, [1.0] * lead + [ht / h, wd / w], order=order, mode="mirror", grid_mode=True).astype(x.dtype)


def _mirror(i, n):
    """ndimage's 'mirror' extension (d c b | a b c d | c b a, period 2 (n - 1)) of index i into 0..n-1."""
    if n == 1:
        return 0
    p = 2 * (n - 1)
    i %= p
    return i if i < n else p - i


def resize_taps(n_in, n_out):
    """One axis of ``_resize(order=1, anti_alias=True)`` as a table: output ``o`` is ``sum_k w[o, k] * src[idx[o, k]]``.
    -> (idx int32 [n_out, K], w float64 [n_out, K]).  The gaussian pre-filter (sigma = (s - 1) / 2, radius int(4 sigma + 0.5), mirror) is
    composed with the two taps of the order-1 ``grid_mode`` zoom; taps that mirror onto the same source index are merged, so a row holds
    at most 2 r + 2 of them.  K is the longest row; shorter rows are padded with weight 0 on their first index."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError("resize_taps: sizes must be positive")
    if n_in == n_out:                                     # _resize leaves an unchanged axis alone: zoom factor 1, no filter
        return np.arange(n_in, dtype=np.int32)[:, None], np.ones((n_in, 1), np.float64)
    s = n_in / n_out
    sigma = max(0.0, (s - 1) / 2)
    if sigma > 0:
        r = int(4.0 * sigma + 0.5)
        k = np.arange(-r, r + 1)
        g = np.exp(-0.5 / (sigma * sigma) * k ** 2)
        g = g / g.sum()
    else:
        r, g = 0, np.ones(1)
    rows = []
    for o in range(n_out):
        c = (o + 0.5) * s - 0.5
        f = int(np.floor(c))
        t = c - f
        acc = {}                                          # source index -> weight, in first-appearance order
        for j, wz in ((f, 1.0 - t), (f + 1, t)):
            if wz == 0.0:
                continue
            j = _mirror(j, n_in)
            for d in range(-r, r + 1):
                src = _mirror(j + d, n_in)
                acc[src] = acc.get(src, 0.0) + wz * g[d + r]
        rows.append(list(acc.items()))
    K = max(len(row) for row in rows)
    idx = np.zeros((n_out, K), np.int32)
    w = np.zeros((n_out, K), np.float64)
    for o, row in enumerate(rows):
        idx[o, :] = row[0][0]
        for q, (src, wt) in enumerate(row):
            idx[o, q], w[o, q] = src, wt
    return idx, w


def resize_pick(n_in, n_out):
    """One axis of ``_resize(order=0)``: the source index each output takes, int32 [n_out] (``floor(c + 0.5)`` of the zoom coordinate
    ``c = (o + 0.5) * n_in / n_out - 0.5``); the identity without a resize."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError("resize_pick: sizes must be positive")
    if n_in == n_out:
        return np.arange(n_in, dtype=np.int32)
    c = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
    return np.clip(np.floor(c + 0.5), 0, n_in - 1).astype(np.int32)


def resize_restated(x, ht, wd):
    """``_resize(x, ht, wd, 1, True)`` restated through the tap tables, in float64: the rows first, then the columns, each sum in the
    table's tap order.  The host mirror of ``ug_prep_resize_frames``; [..., H, W] of any dtype -> float64 [..., ht, wd]."""
    x = np.asarray(x, dtype=np.float64)
    ri, rw = resize_taps(x.shape[-2], ht)
    ci, cw = resize_taps(x.shape[-1], wd)
    mid = np.zeros(x.shape[:-2] + (ht, x.shape[-1]))
    for k in range(ri.shape[1]):
        mid += rw[:, k][:, None] * x[..., ri[:, k], :]
    out = np.zeros(x.shape[:-2] + (ht, wd))
    for k in range(ci.shape[1]):
        out += cw[:, k] * mid[..., ci[:, k]]
    return out


PREP_MODES = ("host", "device")


class ScannetPPDataset:
    """Clip-level dataset in the unified sample format (dataset/Readme.md:22-33); ``dataset[i]`` is one clip.

    ``prep="host"`` (default) resizes and prepares the ground truth in numpy.  ``prep="device"`` leaves the host the file decode and the
    small tables; the anti-aliased frame resize and the ground truth at the target pixels run on the GPU (``ug_prep_resize_frames`` /
    ``ug_prep_gt``) on ``engine``, or on a weight-less engine of the dataset's own on ``device_id``, created with the
    first sample.  There is no fallback: without the library or a GPU, ``prep="device"`` raises."""

    base_dataset = "scannetpp"

    def __init__(self, root, scenes=None, split_file=None, split="test", clip_length=17, clip_overlap=0,
                 input_size=None, target_size=None, verbose=False, prep="host", device_id=0, engine=None, **_):
        if prep not in PREP_MODES:
            raise ValueError(f"prep must be one of {list(PREP_MODES)}, not {prep!r}")
        self.prep, self.device_id, self.engine = prep, device_id, engine
        self._lock = threading.Lock()                       # evaluate(models=[...]) indexes the dataset from several threads
        self.last_timing = None                             # prep="device": seconds of the last sample's decode / resize / gt stages
        if root is None or not os.path.isdir(root):
            raise FileNotFoundError(f"ScanNet++ root not found: {root!r}")
        if isinstance(scenes, str):
            if scenes != "all":
                raise ValueError('scenes must be a list of scene names, None (the split list) or "all"')
            # explicit opt-in: every processed scene under root, sorted (NOT what the reference evaluates)
            scenes = sorted(d for d in os.listdir(root) if os.path.isfile(os.path.join(root, d, "scene_metadata.npz")))
        elif scenes is None:
            # scannetpp.py:209-217: the scene set and its ORDER come from splits/<split>.txt next to the loader
            # ('train' or, for every other split value, 'nvs_sem_val' - the ten validation scenes, shipped as data)
            if split_file is None:
                split_file = os.path.join(os.path.dirname(os.path.abspath(__file__)), "splits",
                                          ("train" if split == "train" else "nvs_sem_val") + ".txt")
            if not os.path.isfile(split_file):
                raise FileNotFoundError(f"ScanNet++ split list not found: {split_file} (pass split_file=... or scenes=[...])")
            with open(split_file) as f:
                scenes = [ln for ln in f.read().splitlines() if ln.strip()]
        self.root, self.split = root, split
        self.input_size, self.target_size = input_size, target_size
        self.samples = []
        for sc in scenes:
            seq = ScannetPPSequence(root, sc, clip_length, clip_overlap)
            if verbose:
                print(f"sequence name: {sc}, num_seq: {len(seq.rgb_paths)}")
            for key, ids in seq.clips.items():
                self.samples.append((seq, key, ids))

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, index):
        if index >= len(self.samples):
            raise IndexError(index)
        seq, _, ids = self.samples[index]
        if self.prep == "device":
            out = self._load_clip_device(seq, ids)
            out["_index"] = index
            out["_dataset"] = self.base_dataset
            return out
        out = load_clip(self.root, seq, ids)
        out["_index"] = index
        out["_dataset"] = self.base_dataset
        if self.input_size is not None:
            ht, wd = self.input_size
            oh, ow = out["images"][0].shape[-2:]
            out["images"] = [_resize(im, ht, wd, 1, True) for im in out["images"]]
            scale = np.array([[wd / ow] * 3, [ht / oh] * 3, [1.0] * 3], np.float32)
            out["intrinsics"] = [k * scale for k in out["intrinsics"]]
        if self.target_size is not None:
            ht, wd = self.target_size
            for attr in ("cam_normal", "world_normal", "cam_coord", "world_coord", "mask"):
                out[attr] = [_resize(x, ht, wd, 0, False) for x in out[attr]]
        return out

    def _device_engine(self):
        if self.engine is None:
            from .._lib import Engine                        # raises without the library or a GPU: no host fallback
            self.engine = Engine(self.device_id, workspace_bytes=256 << 20, persist_bytes=1 << 20)
        return self.engine

    def _load_clip_device(self, seq, ids, keyview_idx=0):
        """``load_clip`` + the two resizes with the pixel arithmetic on the GPU: same keys, shapes and dtypes."""
        t0 = time.perf_counter()
        frames, normals, depth = decode_clip(self.root, seq, ids)
        t1 = time.perf_counter()
        T, hi, wi = depth.shape
        out = {"_base": self.root, "scene_name": "_".join(seq.scene_name.split("/")), "keyview_idx": keyview_idx, "caption": ""}
        ext = [seq.extrinsics[i].astype(np.float32) for i in ids]
        K = [seq.intrinsics[i].astype(np.float32) for i in ids]
        ref = ext[keyview_idx]
        ref_inv = np.linalg.inv(ref)
        M = np.stack([ref @ np.linalg.inv(e) for e in ext]).astype(np.float32)      # source camera -> key-view camera, as load_clip
        K0 = np.broadcast_to(K[0], (T, 3, 3))                                      # scannetpp.py:104: view 0's intrinsics for all views
        ih, iw = self.input_size if self.input_size is not None else (hi, wi)
        th, tw = self.target_size if self.target_size is not None else (hi, wi)
        with self._lock:
            eng = self._device_engine()
            images = eng.prep_resize_frames(frames, ih, iw)
            t2 = time.perf_counter()
            cn, cc, wn, wc, mask = eng.prep_gt(depth, normals, K0, M, resize_pick(hi, th), resize_pick(wi, tw), depth_divisor=1000.0,
                                               max_depth=80.0)
            t3 = time.perf_counter()
        self.last_timing = {"decode": t1 - t0, "resize": t2 - t1, "gt": t3 - t2}
        out["images"] = list(images)
        out["image_names"] = [os.path.basename(seq.rgb_paths[i]) for i in ids]
        if self.input_size is not None:
            scale = np.array([[iw / wi] * 3, [ih / hi] * 3, [1.0] * 3], np.float32)
            K = [k * scale for k in K]
        out["intrinsics"] = K
        out.update(cam_normal=list(cn), cam_coord=list(cc), world_normal=list(wn), world_coord=list(wc), mask=list(mask),
                   extrinsics=[e @ ref_inv for e in ext])
        return out


def decode_clip(root, seq, ids):
    """The file decode of ``load_clip`` alone: (frames uint8 [T,H,W,3], normals uint8 [T,H,W,3], depth uint16 [T,H,W])."""
    base = os.path.join(root, seq.scene_name)
    frames = np.stack([np.array(Image.open(os.path.join(base, seq.rgb_paths[i]))) for i in ids])
    normals = np.stack([np.array(Image.open(os.path.join(base, seq.normal_paths[i]))) for i in ids])
    depth = np.stack([np.array(Image.open(os.path.join(base, seq.depth_paths[i]))) for i in ids])
    if frames.dtype != np.uint8 or normals.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or normals.shape != frames.shape:
        raise ValueError(f"{base}: images / normals must decode to 8-bit RGB of one size")
    if depth.dtype != np.uint16:
        if depth.min() < 0 or depth.max() > 65535:
            raise ValueError(f"{base}: depth does not fit 16 bits")
        depth = depth.astype(np.uint16)
    if depth.shape != frames.shape[:3]:
        raise ValueError(f"{base}: depth and images differ in size")
    return frames, normals, depth


def load_clip(root, seq, ids, keyview_idx=0):
    base = os.path.join(root, seq.scene_name)
    out = {"_base": root, "scene_name": "_".join(seq.scene_name.split("/")), "keyview_idx": keyview_idx, "caption": ""}
    out["images"] = [np.array(Image.open(os.path.join(base, seq.rgb_paths[i]))).astype(np.float32).transpose(2, 0, 1)
                     for i in ids]
    out["image_names"] = [os.path.basename(seq.rgb_paths[i]) for i in ids]
    ext = [seq.extrinsics[i].astype(np.float32) for i in ids]
    out["intrinsics"] = [seq.intrinsics[i].astype(np.float32) for i in ids]
    K0 = out["intrinsics"][0]                                 # scannetpp.py:104 uses view 0's intrinsics for all views

    ref = ext[keyview_idx]
    ref_inv = np.linalg.inv(ref)
    cam_n, cam_c, wor_n, wor_c, masks = [], [], [], [], []
    for j, i in enumerate(ids):
        raw = np.array(Image.open(os.path.join(base, seq.normal_paths[i]))).astype(np.float32)
        hole = np.all(raw < 1e-3, axis=2)
        n = raw / 255.0 * 2 - 1
        n[hole] = 0
        n = n.astype(np.float32).transpose(2, 0, 1)
        depth = np.array(Image.open(os.path.join(base, seq.depth_paths[i]))).astype(np.float32) / 1000
        c = _backproject_gl(depth, K0)
        M = ref @ np.linalg.inv(ext[j])                        # source camera -> key-view camera
        wn = (M[:3, :3] @ n.reshape(3, -1)).reshape(n.shape)
        wc = (M[:3, :3] @ c.reshape(3, -1) + M[:3, 3][:, None]).reshape(c.shape)
        d = -1 * c[2]
        bad = np.isnan(n).any(0) | np.isnan(c).any(0)
        d[np.isnan(d)] = 0
        bad |= (d < 1e-3) | (d > 80)
        for a in (n, c, wn, wc):
            a[:, bad] = 0
        cam_n.append(n); cam_c.append(c); wor_n.append(wn); wor_c.append(wc); masks.append((~bad).astype(np.float32))
    out.update(cam_normal=cam_n, cam_coord=cam_c, world_normal=wor_n, world_coord=wor_c, mask=masks,
               extrinsics=[e @ ref_inv for e in ext])
    return out
