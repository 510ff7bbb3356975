"""Shared inputs of the camera tests (test_camera_cpu.py, test_pointmap_cpu.py, test_pointmap_gpu.py): seeded trajectories, Sim(3) motions,
point-map scenes with known cameras, and stub models for the harness loop."""
import numpy as np
from scipy.spatial.transform import Rotation


def sim3(rng, scale=1.0, angle=None):
    """A random similarity as (c, R, t)."""
    rv = rng.normal(size=3)
    rv *= (rng.uniform(0.3, 2.5) if angle is None else angle) / np.linalg.norm(rv)
    return scale, Rotation.from_rotvec(rv).as_matrix(), rng.normal(0, 2.0, 3)


def apply_sim3(poses, c, R, t):
    """Camera-to-world poses moved by x -> c R x + t: position c R p + t, rotation R R_i."""
    out = poses.copy()
    out[:, :3, :3] = R @ poses[:, :3, :3]
    out[:, :3, 3] = c * poses[:, :3, 3] @ R.T + t
    return out


def trajectory(n, seed, spread=1.0):
    """n camera-to-world poses on a non-planar curve with turning cameras."""
    rng = np.random.default_rng(seed)
    s = np.linspace(0, 1, n)
    pos = np.stack([spread * np.cos(3 * s), spread * np.sin(2 * s), 0.5 * spread * s * s + 0.1 * np.sin(7 * s)], 1) + rng.normal(0, 0.02, (n, 3))
    T = np.tile(np.eye(4), (n, 1, 1))
    T[:, :3, :3] = Rotation.from_rotvec(np.stack([0.3 * s, -0.5 * s, 0.8 * s], 1) + rng.normal(0, 0.02, (n, 3))).as_matrix()
    T[:, :3, 3] = pos
    return T


def pointmap_scene(T, H, W, f, seed, max_deg=45.0, max_t=0.5, noise=0.0):
    """World points [T,H,W,3] float32 seen by T cameras of focal f and principal point (W/2, H/2); camera 0 is the world frame, camera k is turned by
    up to max_deg and moved by up to max_t.  Depth between 1.5 and 3 m: a smooth surface plus uniform noise.  `noise`: Gaussian sigma added to the
    points.  Returns (points, extrinsics [T,4,4] world to camera, float64)."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    z = 2.25 + 0.6 * np.sin(u / (W / 5.0)) * np.cos(v / (H / 4.0)) + rng.uniform(-0.1, 0.1, (H, W))
    ext = np.tile(np.eye(4), (T, 1, 1))
    pts = np.zeros((T, H, W, 3))
    for k in range(T):
        if k:
            ax = rng.normal(size=3)
            ext[k, :3, :3] = Rotation.from_rotvec(ax / np.linalg.norm(ax) * np.radians(max_deg) * k / (T - 1)).as_matrix()
            tt = rng.normal(size=3)
            ext[k, :3, 3] = tt / np.linalg.norm(tt) * max_t * k / (T - 1)
        zk = z + 0.05 * k
        cam = np.stack([(u - W / 2) * zk / f, (v - H / 2) * zk / f, zk], -1)
        pts[k] = (cam - ext[k, :3, 3]) @ ext[k, :3, :3]          # R^T (c - t)
    if noise:
        pts += rng.normal(0, noise, pts.shape)
    return pts.astype(np.float32), ext


def pose_errors(E, ext):
    """Largest rotation distance in degrees and largest translation distance of extrinsics E from ext."""
    dr = np.degrees(Rotation.from_matrix(E[:, :3, :3] @ ext[:, :3, :3].transpose(0, 2, 1)).magnitude())
    return float(dr.max()), float(np.linalg.norm(E[:, :3, 3] - ext[:, :3, 3], axis=1).max())


def gt_opencv_poses(data):
    """The camera-to-world poses that prepare_gt_label gives for a sample, as float64 numpy."""
    from unigeo_amd.harness import prepare_gt_label
    return prepare_gt_label(data)["gt_poses"].numpy().astype(np.float64)


def moving_camera_dataset(**kw):
    """SyntheticGeometryDataset with a camera that turns and leaves the x axis: the stock one slides along x only, and positions on one line do
    not determine the alignment that ATE / RPE need."""
    from unigeo_amd.harness import SyntheticGeometryDataset

    class MovingCameraDataset(SyntheticGeometryDataset):
        def _frame(self, t):
            fr = super()._frame(t)
            c2w = np.eye(4)
            c2w[:3, :3] = Rotation.from_rotvec([0.02 * t, -0.03 * t, 0.01 * t]).as_matrix()
            c2w[:3, 3] = [0.05 * t, 0.04 * np.sin(0.7 * t), 0.002 * t * t]
            cam = fr["cam"].astype(np.float64)
            fr["world"] = (np.einsum("ij,jhw->ihw", c2w[:3, :3], cam) + c2w[:3, 3, None, None]).astype(np.float32)
            fr["ext"] = np.linalg.inv(c2w).astype(np.float32)
            return fr
    return MovingCameraDataset(**kw)


class PoseModel:
    """Stub plugin: returns the ground-truth poses moved by a fixed Sim(3) plus a perturbation seeded by the clip index as ``pred_poses``."""

    def __init__(self, noise=0.0, seed=0):
        self.noise, self.seed = noise, seed
        self.c, self.R, self.t = sim3(np.random.default_rng(seed), scale=1.7)

    def forward(self, data):
        gt = gt_opencv_poses(data)
        pred = apply_sim3(gt, self.c, self.R, self.t)
        pred[:, :3, 3] += np.random.default_rng(self.seed * 1000 + data["_index"]).normal(0, self.noise, (len(pred), 3))
        return dict(_depth_outputs(data), pred_poses=pred)


def _depth_outputs(data):
    z = np.stack([np.abs(np.asarray(c)[2]) for c in data["cam_coord"]], 0).astype(np.float32)
    return {"pred_depths": z * np.float32(1.1) + np.float32(0.05), "pred_normals": np.zeros(z.shape + (3,), np.float32)}


class NoPoseModel:
    """Stub plugin of a depth model: a scaled and shifted ground-truth depth, no poses, no world points."""

    def forward(self, data):
        return _depth_outputs(data)


class PointMapModel:
    """Stub plugin of a point-map model: ``pred_world_pts`` = the ground-truth world points expressed in the frame of the clip's first camera (so
    that frame 0 is its own camera frame, as Spann3R / CUT3R predict), float32; no poses."""
    predicts_world_points = True

    def forward(self, data):
        from unigeo_amd.harness import prepare_gt_label
        gt = prepare_gt_label(data)
        w2c0 = np.linalg.inv(gt["gt_poses"].numpy().astype(np.float64)[0])
        pts = gt["gt_world_pts"].numpy().astype(np.float64)
        return {"pred_world_pts": (pts @ w2c0[:3, :3].T + w2c0[:3, 3]).astype(np.float32)}
