"""CPU: the camera branch of the harness - ``tum_poses`` against the reference's own rows (tests/golden/camera_golden.npz,
made by tests/golden/make_camera_golden.py), ``camera_pose_evaluation`` by its properties (``evo`` is not installed: UNPINNED), and the loop."""
import math
import os
import warnings

import numpy as np
import pytest
from scipy.optimize import minimize
from scipy.spatial.transform import Rotation

from camera_fixtures import NoPoseModel, PoseModel, apply_sim3, moving_camera_dataset, sim3, trajectory

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera_golden.npz")


def _C():
    from unigeo_amd.harness import camera
    return camera


# ------------------------------------------------------------------------------------------------------------------ TUM rows (pinned)
def test_tum_rows_equal_the_reference():
    """x y z qw qx qy qz of the reference's get_tum_poses, the rotation up to the sign of the quaternion, within 1e-12; one of the matrices is
    slightly off orthonormal and one is close to a half turn."""
    g = np.load(GOLD)
    rows, stamps = _C().tum_poses(g["tum_c2w"])
    assert rows.shape == (9, 7) and np.array_equal(stamps, g["tum_stamps"]) and stamps.dtype == np.float64
    assert np.abs(np.linalg.det(g["tum_c2w"][:, :3, :3]) - 1).max() > 1e-6          # the off-orthonormal one is really in there
    assert np.abs(rows[:, :3] - g["tum_rows"][:, :3]).max() <= 1e-12
    sign = np.sign((rows[:, 3:] * g["tum_rows"][:, 3:]).sum(1))[:, None]
    d = np.abs(rows[:, 3:] * sign - g["tum_rows"][:, 3:]).max()
    print("tum rows: quaternion distance", d)
    assert d <= 1e-12
    assert np.abs(np.linalg.norm(rows[:, 3:], axis=1) - 1).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------------------ properties (unpinned)
def test_a_perfect_prediction_scores_zero():
    """pred = a random Sim(3) with scale 2.5 of a non-planar trajectory of 12 poses: positions are O(1) in float64, rounding about 1e-13."""
    gt = trajectory(12, seed=1)
    pred = apply_sim3(gt, *sim3(np.random.default_rng(2), scale=2.5))
    ate, rt, rr = _C().camera_pose_evaluation(pred, gt)
    print("perfect prediction:", ate, rt, rr)
    assert 0 <= ate < 1e-9 and 0 <= rt < 1e-9 and 0 <= rr < 1e-9


def test_known_rpe():
    """Ground truth: steps of length s in the xy-plane, identity rotations; prediction: the same positions, rotations Rz(i * 2 deg).  The
    alignment is the identity, RPE rot is 2 deg, and the relative translation P_i^-1 (p_i+1 - p_i) is the step turned by -theta_i, so its error
    against the step itself is 2 s sin(theta_i / 2)."""
    n, s = 10, 0.3
    rng = np.random.default_rng(5)
    steps = np.zeros((n - 1, 3))
    ang = rng.uniform(0, 2 * np.pi, n - 1)
    steps[:, 0], steps[:, 1] = s * np.cos(ang), s * np.sin(ang)
    gt = np.tile(np.eye(4), (n, 1, 1))
    gt[1:, :3, 3] = np.cumsum(steps, 0)
    pred = gt.copy()
    theta = np.radians(2.0) * np.arange(n)
    pred[:, :3, :3] = Rotation.from_rotvec(np.stack([0 * theta, 0 * theta, theta], 1)).as_matrix()
    ate, rt, rr = _C().camera_pose_evaluation(pred, gt)
    want = math.sqrt(np.mean((2 * s * np.sin(theta[:-1] / 2)) ** 2))
    print("known RPE:", ate, rt, want, rr)
    assert ate < 1e-9 and abs(rr - 2.0) <= 1e-9 and abs(rt - want) <= 1e-9


def _noisy_pair(seed=3, n=15, noise=0.05):
    rng = np.random.default_rng(seed)
    gt = trajectory(n, seed=seed)
    pred = apply_sim3(gt, *sim3(rng, scale=0.6))
    pred[:, :3, 3] += rng.normal(0, noise, (n, 3))
    pred[:, :3, :3] = pred[:, :3, :3] @ Rotation.from_rotvec(rng.normal(0, 0.05, (n, 3))).as_matrix()
    return pred, gt


def test_no_similarity_beats_the_reported_ate():
    """scipy.optimize.minimize over the seven Sim(3) parameters (rotation vector, translation, log scale), started at the answer and at three
    perturbed starts, never finds an RMSE below the reported ATE minus 1e-10."""
    C = _C()
    pred, gt = _noisy_pair()
    ate = C.camera_pose_evaluation(pred, gt)[0]
    P, Q = C.poses_from_tum(C.tum_poses(pred)[0])[:, :3, 3], C.poses_from_tum(C.tum_poses(gt)[0])[:, :3, 3]
    R, t, c = C.umeyama_sim3(P, Q)

    def rmse(x):
        Rm = Rotation.from_rotvec(x[:3]).as_matrix()
        return math.sqrt(np.mean(((math.exp(x[6]) * P @ Rm.T + x[3:6] - Q) ** 2).sum(1)))
    x0 = np.concatenate([Rotation.from_matrix(R).as_rotvec(), t, [math.log(c)]])
    assert abs(rmse(x0) - ate) <= 1e-12
    rng = np.random.default_rng(11)
    best = min(minimize(rmse, x0 + d, method="Nelder-Mead", options={"xatol": 1e-12, "fatol": 1e-14, "maxiter": 4000}).fun
               for d in [np.zeros(7)] + [rng.normal(0, 0.05, 7) for _ in range(3)])
    print("ATE", ate, "best found", best)
    assert best >= ate - 1e-10


def test_mirrored_positions_are_aligned_by_a_proper_rotation():
    C = _C()
    gt = trajectory(12, seed=4)
    pred = gt.copy()
    pred[:, 0, 3] *= -1                                  # a reflection fits best; the alignment must stay a rotation
    R, t, c = C.umeyama_sim3(pred[:, :3, 3], gt[:, :3, 3])
    assert abs(np.linalg.det(R) - 1) <= 1e-12 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and c > 0
    assert C.camera_pose_evaluation(pred, gt)[0] > 1e-3


def test_the_numbers_are_invariant():
    """Under a Sim(3) applied to the prediction, and under one rigid motion applied to both trajectories (1e-9)."""
    C = _C()
    pred, gt = _noisy_pair(seed=6)
    base = C.camera_pose_evaluation(pred, gt)
    rng = np.random.default_rng(8)
    a = C.camera_pose_evaluation(apply_sim3(pred, *sim3(rng, scale=3.2)), gt)
    _, R, t = sim3(rng)
    b = C.camera_pose_evaluation(apply_sim3(pred, 1.0, R, t), apply_sim3(gt, 1.0, R, t))
    print("invariance:", base, a, b)
    assert np.abs(np.subtract(a, base)).max() <= 1e-9 and np.abs(np.subtract(b, base)).max() <= 1e-9
    assert min(base) > 1e-3


def test_edge_cases():
    C = _C()
    gt = trajectory(6, seed=9)
    with pytest.warns(RuntimeWarning) as rec:
        out = C.camera_pose_evaluation(gt[:1], gt[:1])
    assert len(rec) == 1 and all(math.isnan(v) for v in out)
    line = gt.copy()
    line[:, :3, 3] = np.outer(np.arange(6), [0.3, -0.1, 0.2]) + [1, 2, 3]
    with pytest.warns(RuntimeWarning) as rec:
        out = C.camera_pose_evaluation(line, gt)
    assert len(rec) == 1 and all(math.isnan(v) for v in out)
    still = gt.copy()
    still[:, :3, 3] = [1, 2, 3]
    with pytest.warns(RuntimeWarning):
        assert all(math.isnan(v) for v in C.camera_pose_evaluation(still, gt))
    with pytest.raises(ValueError, match="5 predicted poses and 6"):
        C.camera_pose_evaluation(gt[:5], gt)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert all(math.isfinite(v) for v in C.camera_pose_evaluation(gt[:3] + 0, gt[:3]))      # three poses off one line are enough
    with pytest.warns(RuntimeWarning):
        assert all(math.isnan(v) for v in C.camera_pose_evaluation(gt[:2] + 0, gt[:2]))          # two positions are always on one line


# ------------------------------------------------------------------------------------------------------------------ the loop
CFG = {"root": "x", "h": 32, "w": 32, "clip_length": 4, "clip_overlap": 1,
       "eval_depth": {"metric_names": ["Abs Rel", "RMSE"]}}
CAM = {"eval_camera": {"metric_names": ["ATE", "RPE trans", "RPE rot"]}}


def _ds():
    return moving_camera_dataset(clip_length=4, clip_overlap=1, input_size=(32, 32), num_frames=9)


def test_loop_fills_rows_and_csv(tmp_path):
    from unigeo_amd.harness import camera_pose_evaluation, evaluate, prepare_gt_label
    ds = _ds()
    rows, mm = evaluate({**CFG, **CAM}, dataset=ds, model=PoseModel(noise=0.01, seed=1), save_dir=str(tmp_path), verbose=False)
    assert len(rows) == len(ds) == 3
    replay = PoseModel(noise=0.01, seed=1)
    for i, r in enumerate(rows):
        want = camera_pose_evaluation(replay.forward(ds[i])["pred_poses"], prepare_gt_label(ds[i])["gt_poses"])
        assert (r["ATE"], r["RPE trans"], r["RPE rot"]) == want and all(math.isfinite(v) and v > 0 for v in want)
    lines = open(tmp_path / "metrics.csv").read().splitlines()
    assert lines[0] == ",Abs Rel,RMSE,ATE,RPE trans,RPE rot" and len(lines) == 5
    for ln, r in zip(lines[1:4], rows):
        assert ln.split(",")[3:] == ["%.5f" % r[k] for k in ("ATE", "RPE trans", "RPE rot")]
    avg = mm.calculate_averages()
    for k in ("ATE", "RPE trans", "RPE rot"):
        assert avg[k] == pytest.approx(sum(r[k] for r in rows) / 3, abs=1e-15)
    assert lines[4].split(",")[0] == "Average" and lines[4].split(",")[3:] == ["%.5f" % avg[k] for k in ("ATE", "RPE trans", "RPE rot")]


def test_loop_with_several_models_carries_the_camera_keys(tmp_path):
    from unigeo_amd.harness import evaluate, evaluate_sharded
    ds = _ds()
    serial, _ = evaluate({**CFG, **CAM}, dataset=ds, model=PoseModel(0.01), save_dir=str(tmp_path / "a"), verbose=False)
    threaded, _ = evaluate({**CFG, **CAM}, dataset=ds, models=[PoseModel(0.01), PoseModel(0.01)], save_dir=str(tmp_path / "b"), verbose=False)
    sharded, _ = evaluate_sharded({**CFG, **CAM}, ds, PoseModel(0.01), save_dir=str(tmp_path / "c"))
    for other in (threaded, sharded):
        assert [r["seq_name"] for r in other] == [r["seq_name"] for r in serial]
        for a, b in zip(serial, other):
            assert a["ATE"] > 1e-4 and all(abs(a[k] - b[k]) <= 1e-12 for k in ("ATE", "RPE trans", "RPE rot"))


def test_loop_errors(tmp_path):
    from unigeo_amd.harness import evaluate
    with pytest.raises(ValueError, match=r"000_synthetic.*NoPoseModel"):
        evaluate({**CFG, **CAM}, dataset=_ds(), model=NoPoseModel(), save_dir=str(tmp_path), verbose=False)
    with pytest.raises(ValueError, match="vis_camera needs eval_camera"):
        evaluate({**CFG, "vis_camera": True}, dataset=_ds(), model=NoPoseModel(), save_dir=str(tmp_path), verbose=False)

    class Never:
        def forward(self, data):
            raise AssertionError("the model ran before the configuration was checked")
    with pytest.raises(ValueError, match="unknown key.*ransac"):
        evaluate({**CFG, "eval_camera": {"metric_names": ["ATE"], "ransac": 1}}, dataset=_ds(), model=Never(), save_dir=str(tmp_path), verbose=False)
    with pytest.raises(ValueError, match="positive"):
        evaluate({**CFG, "eval_camera": {"metric_names": ["ATE"], "reproj_px": 0}}, dataset=_ds(), model=Never(), save_dir=str(tmp_path), verbose=False)


def test_without_eval_camera_the_csv_keeps_its_bytes(tmp_path):
    """The CSV of a configuration without eval_camera, written here from the rows' existing keys with the sink's own rule ('%.5f', empty for NaN,
    the Average row over the finite values)."""
    from unigeo_amd.harness import evaluate
    rows, _ = evaluate(CFG, dataset=_ds(), model=PoseModel(), save_dir=str(tmp_path), verbose=False)
    names = ["Abs Rel", "RMSE"]
    assert not any(k in r for r in rows for k in ("ATE", "RPE trans", "RPE rot"))
    text = "," + ",".join(names) + "\n"
    for r in rows:
        text += r["seq_name"] + "," + ",".join("%.5f" % r[k] for k in names) + "\n"
    text += "Average," + ",".join("%.5f" % (sum(r[k] for r in rows) / len(rows)) for k in names) + "\n"
    assert open(tmp_path / "metrics.csv", "rb").read() == text.encode()
    assert not [d for d in os.listdir(tmp_path) if d.startswith("camera_")]


def test_vis_camera_writes_trajectories_that_read_back(tmp_path):
    from unigeo_amd.harness import evaluate, prepare_gt_label, read_tum_trajectory
    ds = _ds()
    rows, _ = evaluate({**CFG, **CAM, "vis_camera": True}, dataset=ds, model=PoseModel(noise=0.01, seed=1), save_dir=str(tmp_path), verbose=False)
    replay = PoseModel(noise=0.01, seed=1)
    for i, r in enumerate(rows):
        d = tmp_path / f"camera_{r['seq_name']}"
        want = {"pred_traj.txt": replay.forward(ds[i])["pred_poses"], "gt_traj.txt": prepare_gt_label(ds[i])["gt_poses"].numpy().astype(np.float64)}
        for name, poses in want.items():
            stamps, T = read_tum_trajectory(str(d / name))
            assert np.array_equal(stamps, np.arange(4.0)) and T.shape == (4, 4, 4)
            assert np.abs(T[:, :3, 3] - poses[:, :3, 3]).max() <= 1e-12
            assert np.abs(T[:, :3, :3] - Rotation.from_matrix(poses[:, :3, :3]).as_matrix()).max() <= 1e-12
        try:
            import matplotlib  # noqa: F401
        except ImportError:
            continue
        assert (d / "traj.png").stat().st_size > 1000
