"""Inputs shared by tests/test_gt_normals_cpu.py, tests/test_gt_normals_gpu.py and tests/golden/make_gt_normals_golden.py (DESIGN.md section
30): the tiny two-plane scene, its analytic normals, a scalar restatement of the fit for tiny frames, and one temporary scene per RGB-D
layout written in the file layout the loaders read.

The scene (native 24 x 32, focal 40 px unless a layout fixes its own intrinsics): a tilted plane at 2 m left of column 20, a frontal plane at
3.5 m from column 20 on - a depth step -, quantised to the layout's depth unit; a rectangular hole of raw 0 (rows 5..7, columns 5..8) and one
raw 65535 pixel (row 15, column 3).  A clip is T = 2 frames: the scene and a frame of all zeros."""
import os

import numpy as np
from PIL import Image

H, W, T = 24, 32, 2
STEP = 20                                                   # first column of the frontal plane
HOLE = (slice(5, 8), slice(5, 9))
SENTINEL = (15, 3)
K40 = np.array([[40.0, 0, 15.5], [0, 40.0, 11.5], [0, 0, 1]])
N_TILT = np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])      # OpenCV camera frame: n . p = dist
N_FRONT = np.array([0.0, 0.0, 1.0])
D_TILT, D_FRONT = 2.0, 3.5


def plane_depth(n, dist, K, h=H, w=W):
    """z of the plane n . p = dist along every pixel's ray, float64 [h,w]."""
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    return dist / (n[0] * (u - K[0, 2]) / K[0, 0] + n[1] * (v - K[1, 2]) / K[1, 1] + n[2])


def scene_depth(K=K40, h=H, w=W, step=STEP):
    """The two planes in metres, float64 [h,w], unquantised and without holes."""
    d = plane_depth(N_TILT, D_TILT, K, h, w)
    d[:, step:] = plane_depth(N_FRONT, D_FRONT, K, h, w)[:, step:]
    return d


def quantise(d, divisor=1000.0):
    return np.round(d * divisor).astype(np.uint16)


def scene_raw(K=K40, divisor=1000.0, h=H, w=W, step=STEP, holes=True):
    """uint16 [T,h,w]: frame 0 the quantised scene with the hole and the 65535 pixel, frame 1 all zeros."""
    raw = np.zeros((T, h, w), np.uint16)
    raw[0] = quantise(scene_depth(K, h, w, step), divisor)
    if holes:
        raw[0][HOLE] = 0
        raw[0][SENTINEL] = 65535
    return raw


def truth_gl(n_cv):
    """The plane's unit normal in the loader's OpenGL frame, facing the camera (n . p < 0 for points in front of it)."""
    n = np.array([n_cv[0], -n_cv[1], -n_cv[2]], np.float64)
    return n if n[2] > 0 else -n                            # points have z < 0 in OpenGL: a camera-facing normal has n_z > 0 here


def backproject(raw, K, divisor=1000.0, max_depth=20.0):
    """The float32 loaders' arithmetic on one raw frame -> (cam_coord float32 [3,h,w] zeroed where masked, mask bool [h,w])."""
    from unigeo_amd.harness.scannetpp import _backproject_gl
    c = _backproject_gl(raw.astype(np.float32) / np.float32(divisor), np.asarray(K, np.float32))
    d = -c[2]
    bad = np.isnan(c).any(0) | (d < 1e-3) | (d > max_depth)
    c[:, bad] = 0
    return c, ~bad


def angle_deg(a, b):
    """Angle between vectors along the last axis, in degrees, from renormalised vectors with atan2(|a x b|, a . b): exact near 0, where an
    arccos of the dot product of vectors whose norm is 2e-6 short of 1 reads 0.16 degrees."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    a = a / np.maximum(np.linalg.norm(a, axis=-1, keepdims=True), 1e-300)
    b = b / np.maximum(np.linalg.norm(b, axis=-1, keepdims=True), 1e-300)
    return np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1)))


def loop_fit(points, valid, radius=2, edge=0.05, min_count=None):
    """The fit one pixel at a time with numpy.linalg.solve: for tiny frames only, independent of the vectorised mirror and of its closed-form
    solve.  points float [H,W,3] (any float dtype, used as float64), valid bool [H,W] -> (normals float64 [H,W,3], ok bool [H,W],
    count int [H,W])."""
    P = np.asarray(points, np.float64)
    h, w, _ = P.shape
    r = radius
    mc = (2 * r + 1) ** 2 // 2 + 1 if min_count is None else min_count
    N, ok, cnt = np.zeros((h, w, 3)), np.zeros((h, w), bool), np.zeros((h, w), int)
    for i in range(h):
        for j in range(w):
            if not valid[i, j]:
                continue
            dc = -P[i, j, 2]
            q = [P[a, b] for a in range(max(0, i - r), min(h, i + r + 1)) for b in range(max(0, j - r), min(w, j + r + 1))
                 if valid[a, b] and (edge is None or abs(-P[a, b, 2] - dc) <= edge * dc)]
            cnt[i, j] = len(q)
            if len(q) < mc:
                continue
            q = np.array(q)
            n = np.linalg.solve(q.T @ q / len(q) + 1e-6 * np.eye(3), q.mean(0))
            n = n / (np.linalg.norm(n) + 1e-6)
            N[i, j] = -n if n @ P[i, j] > 0 else n
            ok[i, j] = np.isfinite(n).all()
    return N, ok, cnt


# ---------------------------------------------------------------------------------------------------------------- scenes on disk
SCENE = {"7scenes": "chess/seq-07", "bonn": "rgbd_bonn_planes", "neuralrgbd": "planes_room", "replica": "planes_0", "scannetv2": "scene0999_00"}
LAYOUT_K = {"7scenes": np.array([[525.0, 0, 320], [0, 525.0, 240], [0, 0, 1]]),
            "bonn": np.array([[542.822841, 0, 315.593520], [0, 542.576870, 237.756098], [0, 0, 1]]),
            "neuralrgbd": np.array([[554.2562584220408, 0, 320], [0, 554.2562584220408, 240], [0, 0, 1]]),
            "replica": np.array([[600.0, 0, 599.5], [0, 600.0, 339.5], [0, 0, 1]]),
            "scannetv2": np.array([[577.590698, 0, 320.0], [0, 578.729797, 240.0], [0, 0, 1]])}
SIZE = {"7scenes": (H, W), "bonn": (H, W), "neuralrgbd": (H, W), "replica": (H, W + 8), "scannetv2": (480, 640)}      # Replica: the 4:3 crop removes 4 + 4 columns
STEP_COL = {"7scenes": STEP, "bonn": STEP, "neuralrgbd": STEP, "replica": STEP + 4, "scannetv2": 400}
GAP = {"7scenes": 1, "bonn": 1, "neuralrgbd": 3, "replica": 3, "scannetv2": 2}
DIVISOR = {"7scenes": 1000.0, "bonn": 5000.0, "neuralrgbd": 1000.0, "replica": 1000.0, "scannetv2": 1000.0}


def _pose(i, gl=False):
    """A slow pan, camera-to-world."""
    a = 0.05 * i
    P = np.eye(4)
    P[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    P[:3, 3] = [0.1 * i, 0.02 * i, (0.05 if gl else -0.05) * i]
    return P


def layout_raw(L):
    """The clip the loader of layout ``L`` decodes from ``write_scene(L)``: uint16 [T,h,w] with the layout's intrinsics, size and depth unit."""
    h, w = SIZE[L]
    return scene_raw(LAYOUT_K[L], DIVISOR[L], h, w, STEP_COL[L])


def write_scene(root, L, n_clip=T):
    """<root>/<scene> in the file layout of ``L`` (tests/golden/make_rgbd_golden.py has the formats): as many files as the layout's frame gap
    needs for the loader to keep ``n_clip`` frames - the scene, the frame of zeros, then the scene again.  -> the scene's name."""
    raw = layout_raw(L)
    h, w = SIZE[L]
    n = (n_clip - 1) * GAP[L] + 1
    frames = [raw[1] if i == GAP[L] else raw[0] for i in range(n)]
    yy, xx = np.mgrid[0:(30 if L == "scannetv2" else h), 0:(40 if L == "scannetv2" else w)]
    rgbs = [np.stack([(xx * 5 + 3 * i) % 256, (yy * 7 + i) % 256, (xx + yy) % 256], -1).astype(np.uint8) for i in range(n)]
    d = os.path.join(root, SCENE[L])
    save = lambda a, *p: Image.fromarray(np.ascontiguousarray(a)).save(os.path.join(d, *p), compress_level=1)
    if L == "7scenes":
        os.makedirs(d)
        for i in range(n):
            save(rgbs[i], f"frame-{i:06d}.color.png")
            save(frames[i], f"frame-{i:06d}.depth.proj.png")
            np.savetxt(os.path.join(d, f"frame-{i:06d}.pose.txt"), _pose(i), fmt="%.7e", delimiter="\t")
    elif L == "bonn":
        from scipy.spatial.transform import Rotation
        for sub in ("rgb_110", "depth_110"):
            os.makedirs(os.path.join(d, sub))
        lines = ["# timestamp tx ty tz qx qy qz qw"]
        for i in range(n):
            t = 1548266531.51903 + i / 30
            save(rgbs[i], "rgb_110", f"{t:.5f}.png")
            save(frames[i], "depth_110", f"{t + 0.011:.5f}.png")
            P = _pose(i)
            lines.append(" ".join([f"{t:.4f}"] + [f"{v:.6f}" for v in P[:3, 3]] + [f"{v:.6f}" for v in Rotation.from_matrix(P[:3, :3]).as_quat()]))
        with open(os.path.join(d, "groundtruth_110.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    elif L == "neuralrgbd":
        for sub in ("images", "depth"):
            os.makedirs(os.path.join(d, sub))
        lines = []
        for i in range(n):
            save(rgbs[i], "images", f"img{i}.png")
            save(frames[i], "depth", f"depth{i}.png")
            lines += [" ".join(f"{v:.8f}" for v in row) for row in _pose(i, gl=True)]
        with open(os.path.join(d, "poses.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    elif L == "replica":
        d = os.path.join(d, "imap", "00")
        for sub in ("rgb", "depth"):
            os.makedirs(os.path.join(d, sub))
        for i in range(n):
            save(rgbs[i], "rgb", f"rgb_{i}.png")
            save(frames[i], "depth", f"depth_{i}.png")
        with open(os.path.join(d, "traj_w_cgl.txt"), "w") as f:
            f.write("\n".join(" ".join(f"{v:.8f}" for v in _pose(i, gl=True).reshape(-1)) for i in range(n)) + "\n")
    elif L == "scannetv2":
        for sub in ("color_270", "depth_270", "intrinsic"):
            os.makedirs(os.path.join(d, sub))
        for i in range(n):
            Image.fromarray(rgbs[i]).save(os.path.join(d, "color_270", f"{i * 10:06d}.jpg"), quality=90)
            save(frames[i], "depth_270", f"{i * 10:06d}.png")
        np.savetxt(os.path.join(d, "pose_270.txt"), np.concatenate([_pose(i) for i in range(n)], 0), fmt="%.8f")
        K4 = np.eye(4)
        K4[:3, :3] = LAYOUT_K[L]
        np.savetxt(os.path.join(d, "intrinsic", "intrinsic_depth.txt"), K4, fmt="%.6f")
    else:
        raise KeyError(L)
    return SCENE[L]


def write_raw_7scenes(root):
    """A 7-Scenes scene of RAW depth at the raw size (480 x 640) for ``register=``: the two planes seen by the depth camera, two frames."""
    from register_fixtures import write_scene as write_register_scene
    Kd = np.array([[585.0, 0, 320], [0, 585.0, 240], [0, 0, 1]])
    raw = scene_raw(Kd, 1000.0, 480, 640, 400)
    raw[1] = raw[0]                                          # the register fixture's loader keeps both frames: no frame of zeros here
    return write_register_scene(root, raw, raw)
