"""Meshes, cameras and a tiny raw ScanNet++ scene shared by tests/test_render_mesh_cpu.py and tests/test_render_mesh_gpu.py (DESIGN.md
section 29).  Every case is small enough for the numpy mirror to take well under a second; results that several tests need are computed once
(``mirror``) and handed out read-only."""
import functools
import json
import os

import numpy as np
from PIL import Image

from unigeo_amd.harness.ply import write_ply_mesh
from unigeo_amd.harness.render import render_mesh

K_BOX = (40.0, 41.0, 32.3, 24.1)            # fx, fy, cx, cy: no pixel centre on a principal axis
K_DIAG = (32.0, 32.0, 32.0, 24.0)           # rays are multiples of 1/64: the quad's diagonal runs through pixel centres exactly
H, W = 48, 64
BOX_HALF = (1.3, 0.9, 1.7)


def _ro(a):
    a.setflags(write=False)
    return a


def identity_pose():
    return np.eye(4)


def gl_world_pose():
    """A camera whose world frame is the OpenGL camera frame (x right, y up, z backward): cam_to_world = diag(1, -1, -1)."""
    return np.diag([1.0, -1.0, -1.0, 1.0])


def pose(R, centre):
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, centre
    return P


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def plane(z=2.0, half=10.0):
    v = np.float32([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]])
    return v, np.int32([[0, 1, 2], [0, 2, 3]])


def diag_quad():
    """Two triangles at z = 1 whose shared edge y = x passes through the centres of the pixels row = col - 8 under K_DIAG."""
    v = np.float32([[-2, -2, 1], [2, -2, 1], [2, 2, 1], [-2, 2, 1]])
    return v, np.int32([[0, 1, 2], [0, 2, 3]])


def box():
    """The closed box of half-extents BOX_HALF about the origin: 8 corners, 12 triangles."""
    hx, hy, hz = BOX_HALF
    v = np.float32([[sx * hx, sy * hy, sz * hz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.int32([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])
    return v, f


def box_poses(n=20, seed=5):
    """Seeded random rotations, the camera within +-0.5 of the box's centre."""
    rng = np.random.default_rng(seed)
    return np.stack([pose(random_rotation(rng), rng.uniform(-0.5, 0.5, 3)) for _ in range(n)])


def floor(y=1.0, half=50.0):
    """The plane y = 1 (below a camera whose y axis points down), +-50 m: it straddles the camera plane z = 0."""
    v = np.float32([[-half, y, -half], [half, y, -half], [half, y, half], [-half, y, half]])
    return v, np.int32([[0, 1, 2], [0, 2, 3]])


def duplicates(flip=False):
    """One triangle at z = 1.5 twice, the second copy wound the other way (``flip``: the first one)."""
    v = np.float32([[-1, -0.6, 1.5], [1, -0.6, 1.5], [0, 0.8, 1.5]])
    f = np.int32([[0, 1, 2], [0, 2, 1]])
    return v, (f[::-1].copy() if flip else f)


def with_degenerate():
    """The plane at z = 2 behind two degenerate triangles at z = 1 (a repeated corner; three corners on a line): they must be skipped."""
    v, f = plane()
    v = np.concatenate([v, np.float32([[-1, -1, 1], [1, 1, 1], [0, 0, 1]])])
    return v, np.concatenate([np.int32([[4, 4, 5], [4, 6, 5]]), f])


def bumpy_grid(n=32, seed=11):
    """About 2 000 triangles of a bumpy sheet at z ~ 1.5 with cells from a fraction of a pixel to a dozen pixels, in front of ONE quad at
    z = 3 that fills the frame: screen boxes from one pixel to the whole frame.  Rendered at 96 x 128 with GRID_K."""
    rng = np.random.default_rng(seed)
    s = np.linspace(-1.0, 1.0, n)
    g = np.sign(s) * np.abs(s) ** 2.5
    xx, yy = np.meshgrid(g * 1.0, g * 0.7)
    zz = 1.5 + 0.2 * rng.random((n, n))
    v = np.stack([xx, yy, zz], -1).reshape(-1, 3)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel(), idx[1:, :-1].ravel()
    f = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    back = np.float64([[-6, -6, 3], [6, -6, 3], [6, 6, 3], [-6, 6, 3]])
    f = np.concatenate([f, np.int32([[n * n, n * n + 1, n * n + 2], [n * n, n * n + 2, n * n + 3]])])
    return np.concatenate([v, back]).astype(np.float32), f.astype(np.int32)


GRID_K, GRID_HW = (80.0, 80.0, 64.2, 47.9), (96, 128)


@functools.lru_cache(maxsize=None)
def mirror(name):
    """The host mirror's ``(depth_mm, normal, tri_index)`` for a named case, computed once; read-only arrays."""
    cases = {
        "box3": lambda: render_mesh(*box(), box_poses()[:3], K_BOX, H, W),
        "box20": lambda: render_mesh(*box(), box_poses(), K_BOX, H, W),
        "floor": lambda: render_mesh(*floor(), identity_pose(), K_BOX, H, W),
        "diag": lambda: render_mesh(*diag_quad(), identity_pose(), K_DIAG, H, W),
        "dup": lambda: render_mesh(*duplicates(), identity_pose(), K_BOX, H, W),
        "grid": lambda: render_mesh(*bumpy_grid(), identity_pose(), GRID_K, *GRID_HW),
        "box_37x53": lambda: render_mesh(*box(), box_poses()[3:5], (30.0, 29.0, 26.4, 18.7), 37, 53),
        "box_1x1": lambda: render_mesh(*box(), box_poses()[:2], (1.0, 1.0, 0.5, 0.5), 1, 1),
        "empty": lambda: render_mesh(*plane(z=-2.0), identity_pose(), K_BOX, H, W),
        "box_vga": lambda: render_mesh(*box(), box_poses()[:2], (400.0, 410.0, 323.0, 241.0), 480, 640),
    }
    return tuple(_ro(a) for a in cases[name]())


# ---------------------------------------------------------------- a tiny raw ScanNet++ scene for tools/render_scannetpp.py
SCENE = "abc123"
RAW_HW = (48, 64)


def write_raw_scene(root, n=6, seed=3):
    """``<root>/data/<SCENE>/{iphone/{pose_intrinsic_imu.json, rgb/*.jpg, rgb_masks/*.png}, scans/mesh_aligned_0.05.ply}``: the box mesh,
    ``n`` frames of 64 x 48 from inside it, masks that are 255 but for a blanked top-left corner.  Returns the frame names."""
    rng = np.random.default_rng(seed)
    base = os.path.join(root, "data", SCENE)
    for sub in ("iphone/rgb", "iphone/rgb_masks", "scans"):
        os.makedirs(os.path.join(base, sub))
    write_ply_mesh(os.path.join(base, "scans", "mesh_aligned_0.05.ply"), *box())
    h, w = RAW_HW
    poses = box_poses(n, seed=9)
    names, imu = [], {}
    for i in range(n):
        nm = f"frame_{i * 10:06d}"
        names.append(nm)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(base, "iphone", "rgb", nm + ".jpg"), quality=95)
        mask = np.full((h, w), 255, np.uint8)
        mask[:5, :7] = 0
        Image.fromarray(mask).save(os.path.join(base, "iphone", "rgb_masks", nm + ".png"))
        imu[nm] = {"aligned_pose": poses[i].tolist(), "intrinsic": [[40.0 + i, 0.0, 31.6], [0.0, 41.0, 23.7], [0.0, 0.0, 1.0]]}
    with open(os.path.join(base, "iphone", "pose_intrinsic_imu.json"), "w") as f:
        json.dump(imu, f)
    return names
