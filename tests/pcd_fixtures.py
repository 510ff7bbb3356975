"""Seeded synthetic clouds shared by tests/test_pcd_cpu.py and tests/test_pcd_gpu.py: a wavy surface in front of the camera and a copy of it
turned by 0.01 rad, shifted by about 0.01 and perturbed by 0.002 noise - the case ICP has to pull back."""
import numpy as np


def small_rotation(angle=0.01, axis=(1.0, 2.0, 3.0)):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def surface(xy):
    return 0.2 * np.sin(3.0 * xy[..., 0]) * np.cos(2.0 * xy[..., 1]) + 0.1 * xy[..., 0] + 3.0


def wavy_pair(n, seed=0, noise=0.002):
    """-> (pred float32 [n,3], gt float32 [n,3])."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1.0, 1.0, (n, 2))
    gt = np.concatenate([xy, surface(xy)[:, None]], 1)
    pred = gt @ small_rotation().T + np.array([0.01, -0.005, 0.008]) + rng.normal(0.0, noise, gt.shape)
    return pred.astype(np.float32), gt.astype(np.float32)


def wavy_grid(T, H, W, seed=0, keep=0.75, noise=0.002):
    """The same surface sampled on a jittered pixel grid -> (pred [T,H,W,3], gt [T,H,W,3] float32, mask [T,H,W] bool, rgb [T,H,W,3] float32)."""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.linspace(-1, 1, W), np.linspace(-1, 1, H), indexing="xy")
    xy = np.stack([np.broadcast_to(u, (T, H, W)), np.broadcast_to(v, (T, H, W))], -1) + rng.uniform(-0.5, 0.5, (T, H, W, 2)) * (2.0 / max(H, W))
    gt = np.concatenate([xy, surface(xy)[..., None]], -1)
    pred = gt @ small_rotation().T + np.array([0.01, -0.005, 0.008]) + rng.normal(0.0, noise, gt.shape)
    mask = rng.uniform(size=(T, H, W)) < keep
    rgb = rng.uniform(size=(T, H, W, 3)).astype(np.float32)
    return pred.astype(np.float32), gt.astype(np.float32), mask, rgb


def depth_scene(shape, seed):
    """Seeded depth inputs with a different K and a different rotated, translated pose per frame -> (pred, gt [T,H,W] float32 with about 5 %
    invalid pixels, poses [T,4,4], K [T,3,3] float32)."""
    rng = np.random.default_rng(seed)
    T, H, W = shape
    gt = rng.uniform(0.5, 6.0, shape).astype(np.float32)
    gt[rng.uniform(size=shape) < 0.05] = 0.0
    gt[0, 0, 0] = 1.0
    pred = (0.7 * gt + 0.3 + 0.2 * rng.standard_normal(shape)).astype(np.float32) * (1.0 + 0.1 * np.arange(T, dtype=np.float32))[:, None, None]
    f = 0.9 * max(H, W)
    K = np.stack([np.array([[f + 3 * k, 0, W / 2.0 + 0.5 * k], [0, f - 2 * k, H / 2.0 - 0.25 * k], [0, 0, 1]], np.float32) for k in range(T)], 0)
    poses = np.tile(np.eye(4, dtype=np.float32), (T, 1, 1))
    for k in range(T):
        R = small_rotation(0.25 + 0.2 * k, (0.3 + k, 1.0, 0.2 * k))
        poses[k, :3, :3] = R.astype(np.float32)
        poses[k, :3, 3] = (R @ np.array([0.0, 0.0, 3.0]) + np.array([0.8 * k - 0.5, -0.6, 0.7])).astype(np.float32)
    return pred, gt, poses, K
