"""Camera-pose metrics of the reference's ``eval_camera`` branch (eval.py:85-95, ``metrics/eval_camera.py``): ATE, RPE trans, RPE rot.
numpy + scipy in float64; a clip is about 25 poses, so there is nothing here for the GPU.

* ``tum_poses`` restates ``get_tum_poses`` / ``c2w_to_tumpose`` (``metrics/utils.py:169-192``) and is PINNED by
  ``tests/golden/camera_golden.npz``, which holds that function's own output.
* ``camera_pose_evaluation`` restates ``evo_utils.eval_metrics`` (``metrics/evo_utils.py:163-249``).  UNPINNED: ``evo`` is not installed, so
  what it computes (Sim(3) Umeyama alignment, APE on the translation part, RPE over consecutive frames on the translation part and on the
  rotation angle in degrees, each as RMSE) is restated from its definition and tested by its properties (tests/test_camera_cpu.py).
"""
import math
import os
import warnings

import numpy as np
from scipy.spatial.transform import Rotation

CAMERA_KEYS = ("ATE", "RPE trans", "RPE rot")


def _np64(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def tum_poses(c2w):
    """Camera-to-world matrices ``[N,4,4]`` -> ``(rows [N,7] = x y z qw qx qy qz, stamps = arange(N) as float)``.  The rotation goes through
    scipy's ``Rotation.from_matrix``, which replaces a matrix that is slightly off orthonormal by the closest rotation, as the reference's
    does."""
    c2w = _np64(c2w).reshape(-1, 4, 4)
    if len(c2w) == 0:
        return np.zeros((0, 7)), np.zeros(0)
    q = Rotation.from_matrix(c2w[:, :3, :3]).as_quat()          # x y z w
    return np.concatenate([c2w[:, :3, 3], q[:, 3:4], q[:, :3]], 1), np.arange(len(c2w)).astype(float)


def poses_from_tum(rows):
    """``[N,7]`` rows ``x y z qw qx qy qz`` -> ``[N,4,4]``; the quaternion is normalised first."""
    rows = np.asarray(rows, np.float64).reshape(-1, 7)
    T = np.tile(np.eye(4), (len(rows), 1, 1))
    if len(rows):
        T[:, :3, :3] = Rotation.from_quat(rows[:, [4, 5, 6, 3]]).as_matrix()
        T[:, :3, 3] = rows[:, :3]
    return T


def umeyama_sim3(x, y):
    """Least-squares ``y ~ c R x + t`` over positions ``[N,3]`` (Umeyama 1991) -> ``(R, t, c)``, or ``None`` when fewer than two singular
    values of the covariance exceed machine epsilon (all ``x`` equal or on one line: the rotation is not determined)."""
    mx, my = x.mean(0), y.mean(0)
    sx2 = float(((x - mx) ** 2).sum(1).mean())
    cov = (y - my).T @ (x - mx) / len(x)
    U, D, Vt = np.linalg.svd(cov)
    if int((D > np.finfo(np.float64).eps).sum()) < 2:
        return None
    S = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0])
    R = U @ S @ Vt
    c = float(np.trace(np.diag(D) @ S)) / sx2
    return R, my - c * (R @ mx), c


def align_sim3(pred, gt):
    """Predicted poses ``[N,4,4]`` moved onto the ground truth by the Sim(3) that fits the positions: position ``R (c p) + t``, rotation
    ``R R_i``.  ``None`` when the alignment is not determined."""
    fit = umeyama_sim3(pred[:, :3, 3], gt[:, :3, 3])
    if fit is None:
        return None
    R, t, c = fit
    out = pred.copy()
    out[:, :3, 3] = (c * pred[:, :3, 3]) @ R.T + t
    out[:, :3, :3] = R @ pred[:, :3, :3]
    return out


def _inv_se3(T):
    out = np.tile(np.eye(4), (len(T), 1, 1))
    Rt = T[:, :3, :3].transpose(0, 2, 1)
    out[:, :3, :3] = Rt
    out[:, :3, 3] = -np.einsum("nij,nj->ni", Rt, T[:, :3, 3])
    return out


def camera_pose_evaluation(pred_pose, gt_pose):
    """``(ate, rpe_trans, rpe_rot)`` of camera-to-world poses ``[N,4,4]``, the reference's signature.  UNPINNED (module docstring).

    Both trajectories go through ``tum_poses`` and back (unit quaternion -> matrix), as ``make_traj`` does.  The prediction is aligned with
    the Sim(3) of Umeyama on the positions.  ``ATE = sqrt(mean |p'_i - q_i|^2)``.  RPE over the pairs ``(i, i + 1)`` of the aligned
    trajectory: ``E = (Q_i^-1 Q_i+1)^-1 (P'_i^-1 P'_i+1)``, translation error ``|E[:3, 3]|``, rotation error the angle of ``E[:3, :3]`` in degrees
    from the quaternion (``2 atan2(|xyz|, |w|)``), each as the RMSE over the pairs.

    Deliberate differences: a different number of poses is a ``ValueError`` (the reference prints the two counts and lets ``evo`` associate
    by timestamp); fewer than 2 poses, or predicted positions that do not determine the alignment (standing still or on one line, where
    ``evo`` raises ``GeometryException``), give three NaN and one warning, so that one clip does not end a whole evaluation -
    ``MetricsManager`` leaves NaN out of the average."""
    pred, gt = _np64(pred_pose).reshape(-1, 4, 4), _np64(gt_pose).reshape(-1, 4, 4)
    if len(pred) != len(gt):
        raise ValueError(f"camera_pose_evaluation: {len(pred)} predicted poses and {len(gt)} ground-truth poses")
    nan3 = (math.nan, math.nan, math.nan)
    if len(pred) < 2:
        warnings.warn(f"camera_pose_evaluation: {len(pred)} pose(s); ATE / RPE need at least 2", RuntimeWarning, stacklevel=2)
        return nan3
    P, Q = poses_from_tum(tum_poses(pred)[0]), poses_from_tum(tum_poses(gt)[0])
    Pa = align_sim3(P, Q)
    if Pa is None:
        warnings.warn("camera_pose_evaluation: the predicted positions coincide or lie on one line; the Sim(3) alignment is not determined",
                      RuntimeWarning, stacklevel=2)
        return nan3
    ate = math.sqrt(float(((Pa[:, :3, 3] - Q[:, :3, 3]) ** 2).sum(1).mean()))
    dQ = _inv_se3(Q[:-1]) @ Q[1:]
    dP = _inv_se3(Pa[:-1]) @ Pa[1:]
    E = _inv_se3(dQ) @ dP
    et = np.linalg.norm(E[:, :3, 3], axis=1)
    er = np.degrees(Rotation.from_matrix(E[:, :3, :3]).magnitude())
    return ate, math.sqrt(float((et * et).mean())), math.sqrt(float((er * er).mean()))


# ------------------------------------------------------------------------------------------------------------------ vis_camera
def write_tum_trajectory(path, c2w):
    """``stamp x y z qx qy qz qw`` per pose, the TUM order that ``read_tum_trajectory`` (harness/rgbd.py) reads back.  The reference's
    ``save_trajectory_tum_format`` writes the quaternion scalar first; files written here follow the format's own definition instead."""
    rows, stamps = tum_poses(c2w)
    with open(path, "w") as f:
        for s, r in zip(stamps, rows):
            f.write(" ".join(repr(float(v)) for v in (s, r[0], r[1], r[2], r[4], r[5], r[6], r[3])) + "\n")


def best_plot_axes(positions):
    """The two axes of largest variance, largest first (``best_plotmode`` of ``metrics/evo_utils.py:328-331``)."""
    _, i1, i2 = np.argsort(np.var(np.asarray(positions, np.float64), axis=0))
    return int(i2), int(i1)


def save_camera_trajectories(pred_pose, gt_pose, out_dir):
    """``vis_camera``: ``pred_traj.txt`` / ``gt_traj.txt`` (TUM) and, with matplotlib, ``traj.png`` - the aligned prediction in blue over
    the ground truth in gray dashes on the two axes of largest ground-truth variance (``plot_trajectory``).  Returns the files written."""
    os.makedirs(out_dir, exist_ok=True)
    pred, gt = _np64(pred_pose).reshape(-1, 4, 4), _np64(gt_pose).reshape(-1, 4, 4)
    files = [os.path.join(out_dir, "pred_traj.txt"), os.path.join(out_dir, "gt_traj.txt")]
    write_tum_trajectory(files[0], pred)
    write_tum_trajectory(files[1], gt)
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return files
    aligned = align_sim3(pred, gt) if len(pred) == len(gt) and len(pred) >= 2 else None
    shown = pred if aligned is None else aligned
    a, b = best_plot_axes(gt[:, :3, 3])
    fig = plt.figure(figsize=(8, 8))
    ax = fig.add_subplot(111)
    ax.plot(gt[:, a, 3], gt[:, b, 3], "--", color="gray", label="Ground Truth")
    ax.plot(shown[:, a, 3], shown[:, b, 3], "-", color="blue", label="Predicted")
    ax.set_xlabel("xyz"[a] + " (m)"); ax.set_ylabel("xyz"[b] + " (m)")
    ax.set_aspect("equal", adjustable="datalim")
    ax.legend()
    files.append(os.path.join(out_dir, "traj.png"))
    fig.savefig(files[-1])
    plt.close(fig)
    return files
