"""CPU: the numpy mirror of the point-map step (harness/pointmap.py) - the focal against the reference's float32 values
(tests/golden/camera_golden.npz), the pose solver against known cameras, an independent optimiser, outliers, invalid pixels, and the loop.

Measured here (printed by the tests): poses of the exact scene within 4.3e-7 degrees and 1.8e-8 m of the truth."""
import os

import numpy as np
import pytest
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation

from camera_fixtures import PointMapModel, moving_camera_dataset, pointmap_scene, pose_errors

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera_golden.npz")


def _P():
    from unigeo_amd.harness import pointmap
    return pointmap


def test_focal_against_the_reference():
    """Relative distance from the reference's float32 value at most twice the distance the generator recorded: the reference is the yardstick,
    the stored number is the record."""
    g = np.load(GOLD)
    for k in range(2):
        f = _P().pointmap_focal(g[f"focal_pts_{k}"])
        d = abs(f - g["focal_ref"][k]) / g["focal_ref"][k]
        print(f"focal {k}: {f!r} reference {g['focal_ref'][k]!r} relative distance {d:.3g} recorded {g['focal_distance'][k]:.3g}")
        assert g["focal_distance"][k] < 1e-6 and d <= 2 * g["focal_distance"][k]
    assert not np.isfinite(g["focal_pts_1"]).all() and (g["focal_pts_1"][..., 2] == 0).any()


def test_ordered_sum_is_the_plain_sum_in_another_order():
    P = _P()
    rng = np.random.default_rng(0)
    for n in (1, 255, 256, 257, 391, 768, 262144 + 5):          # the last one crosses the 1024-block cap: a second pixel per thread
        v = rng.normal(size=(n, 3))
        s = P._ordered_sum(v)
        assert np.abs(s - v.sum(0)).max() <= 1e-9 and np.abs(P._ordered_sum(v, reverse=True) - s).max() <= 1e-9
        assert P._ordered_sum(v[:, 0]) == s[0]
    ints = np.arange(1000, dtype=np.float64)
    assert P._ordered_sum(ints) == 499500.0


@pytest.fixture(scope="module")
def exact():
    """3 frames of 24 x 32, focal 30, depth 1.5 .. 3 m, poses up to 45 degrees and 0.5 m from frame 0, points rounded to float32."""
    pts, ext = pointmap_scene(3, 24, 32, 30.0, seed=1)
    assert 1.4 < np.linalg.norm(pts[0], axis=-1).min() and pts[0][..., 2].max() < 3.1
    return pts, ext, _P().pointmap_poses(pts, focal=30.0)


def test_pose_recovery_on_exact_data(exact):
    """From the identity start, within 2e-5 degrees and 6e-7 m of the truth: 100 x what a prototype of this solver reached, because the error
    scales with the float32 rounding of the inputs."""
    pts, ext, res = exact
    dr, dt = pose_errors(res["extrinsics"], ext)
    print(f"exact data: rotation {dr:.3g} deg, translation {dt:.3g} m, iterations {res['iterations'].tolist()}, rms {res['reproj_rms'].tolist()}")
    assert dr <= 2e-5 and dt <= 6e-7
    assert np.array_equal(res["n_inliers"], [768] * 3) and res["inliers"].all() and (res["iterations"] < 300).all()
    assert (res["reproj_rms"] < 1e-4).all()
    z = (pts.astype(np.float64) @ ext[:, :3, :3].transpose(0, 2, 1)[:, None] + ext[:, None, None, :3, 3])[..., 2]
    assert res["depth"].dtype == np.float32 and np.abs(res["depth"] - z).max() <= 1e-6
    assert np.array_equal(res["extrinsics"][:, 3], np.tile([0, 0, 0, 1.0], (3, 1)))
    assert np.abs(res["extrinsics"][:, :3, :3] @ res["extrinsics"][:, :3, :3].transpose(0, 2, 1) - np.eye(3)).max() <= 1e-14


def test_focal_then_poses(exact):
    """Without a focal the first frame gives it; the scene's focal comes back and the poses with it."""
    pts, ext, _ = exact
    res = _P().pointmap_poses(pts)
    dr, dt = pose_errors(res["extrinsics"], ext)
    print(f"recovered focal {res['focal']!r}: rotation {dr:.3g} deg, translation {dt:.3g} m")
    assert abs(res["focal"] - 30.0) <= 1e-6 and dr <= 1e-4 and dt <= 1e-5


def _objective(P, pts_k, f, x):
    fr = P._Frame(pts_k, f, pts_k.shape[1] / 2.0, pts_k.shape[0] / 2.0, False)
    c = fr.X @ Rotation.from_rotvec(x[:3]).as_matrix().T + x[3:]
    return (c - fr.b * (fr.b * c).sum(1, keepdims=True)).ravel()


@pytest.mark.parametrize("noise", [0.0, 0.01])
def test_an_independent_optimiser_finds_nothing_better(noise):
    """scipy.optimize.least_squares on the same object-space residuals (rotation vector + t), started at the truth, does not reach an objective
    below the solver's by more than a relative 1e-9 - on points with 1 cm of noise, where the optimum is not the truth.  On the exact scene the
    objective is the float32 rounding of the input and is only known to a relative 1e-10 (c - V c cancels), and the solver stops when it moves
    by less than 1e-6 of the rounding sum (pointmap_poses); there the same check is made with the bound that this stop rule gives: the
    objective settles near 0.07 of the rounding sum, so 1e-6 / 0.07, rounded up to 1e-4."""
    P = _P()
    pts, ext = pointmap_scene(3, 24, 32, 30.0, seed=2, noise=noise)
    res = P.pointmap_poses(pts, focal=30.0, reproj_px=1e6)
    for k in (1, 2):
        E = res["extrinsics"][k]
        mine = float((_objective(P, pts[k], 30.0, np.concatenate([Rotation.from_matrix(E[:3, :3]).as_rotvec(), E[:3, 3]])) ** 2).sum())
        x0 = np.concatenate([Rotation.from_matrix(ext[k, :3, :3]).as_rotvec(), ext[k, :3, 3]])
        opt = least_squares(lambda x: _objective(P, pts[k], 30.0, x), x0, xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale=1.0)
        theirs = float((opt.fun ** 2).sum())
        print(f"noise {noise} frame {k}: solver {mine:.17g} least_squares {theirs:.17g} relative {(mine - theirs) / mine:.3g}")
        assert theirs >= mine * (1 - (1e-9 if noise else 1e-4))


def test_outliers_are_trimmed():
    """5 % of the points displaced by about 1 m at 48 x 64, focal 60: the trim removes at least 90 % of them and at most 2 % of the others, and
    the pose is closer to the truth than the untrimmed fit."""
    P = _P()
    pts, ext = pointmap_scene(2, 48, 64, 60.0, seed=3, noise=0.002)
    rng = np.random.default_rng(4)
    bad = rng.uniform(size=pts.shape[:3]) < 0.05
    d = rng.normal(size=(int(bad.sum()), 3))
    pts[bad] += (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.7, 1.3, (len(d), 1))).astype(np.float32)
    res = P.pointmap_poses(pts, focal=60.0)
    raw = P.pointmap_poses(pts, focal=60.0, max_rounds=0)
    removed_bad = 1 - res["inliers"][bad].mean()
    removed_good = 1 - res["inliers"][~bad].mean()
    e_trim, e_raw = pose_errors(res["extrinsics"], ext), pose_errors(raw["extrinsics"], ext)
    print(f"outliers: {removed_bad:.3f} of the displaced and {removed_good:.4f} of the others removed; trimmed {e_trim}, untrimmed {e_raw}")
    assert removed_bad >= 0.9 and removed_good <= 0.02
    assert e_trim[0] < e_raw[0] and e_trim[1] < e_raw[1]
    assert np.array_equal(res["n_inliers"], res["inliers"].reshape(2, -1).sum(1))


def test_invalid_pixels_and_mask():
    P = _P()
    pts, ext = pointmap_scene(2, 17, 23, 25.0, seed=5)
    rng = np.random.default_rng(6)
    holes = rng.uniform(size=pts.shape[:3]) < 0.1
    pts[holes, rng.integers(0, 3, int(holes.sum()))] = np.nan
    pts[0, 0, 0] = np.inf
    mask = rng.uniform(size=pts.shape[:3]) < 0.8
    res = P.pointmap_poses(pts, focal=25.0, mask=mask)
    valid = np.isfinite(pts).all(-1) & mask
    assert np.array_equal(res["depth"] == 0, ~valid) and not res["inliers"][~valid].any()
    assert np.array_equal(res["n_inliers"], valid.reshape(2, -1).sum(1))
    dr, dt = pose_errors(res["extrinsics"], ext)
    print(f"holes and mask: rotation {dr:.3g} deg, translation {dt:.3g} m")
    assert dr <= 2e-5 and dt <= 6e-7
    masked_out = pts.copy()
    masked_out[~mask] = 1e3                          # what the mask hides does not matter
    again = P.pointmap_poses(masked_out, focal=25.0, mask=mask)
    assert again["extrinsics"].tobytes() == res["extrinsics"].tobytes() and again["depth"].tobytes() == res["depth"].tobytes()
    few = np.zeros(pts.shape[:3], bool)
    few[1].ravel()[np.flatnonzero(valid[1])[:3]] = True
    few[0] = True
    with pytest.raises(ValueError, match="frame 1 has 3 valid pixels"):
        P.pointmap_poses(pts, focal=25.0, mask=few)
    with pytest.raises(ValueError, match="focal"):
        P.pointmap_poses(pts, focal=0.0)
    with pytest.raises(ValueError, match=r"\[T,H,W,3\]"):
        P.pointmap_poses(pts[0], focal=25.0)


def test_end_to_end_through_the_loop(tmp_path):
    """pred_world_pts of a stub point-map model through evaluate with eval_camera and eval_pcd: ATE below 1e-5 m on exact data."""
    from unigeo_amd.harness import evaluate
    cfg = {"root": "x", "h": 32, "w": 48, "clip_length": 4, "clip_overlap": 1,
           "eval_pcd": {"metric_names": ["acc", "comp"], "pcd_downsample_num": 400},
           "eval_camera": {"metric_names": ["ATE", "RPE trans", "RPE rot"]}}
    ds = moving_camera_dataset(clip_length=4, clip_overlap=1, input_size=(32, 48), num_frames=6)
    rows, mm = evaluate(cfg, dataset=ds, model=PointMapModel(), save_dir=str(tmp_path), verbose=False)
    assert len(rows) == 2
    for r in rows:
        print(r["seq_name"], "ATE", r["ATE"], "RPE trans", r["RPE trans"], "RPE rot", r["RPE rot"], "acc", r["acc"])
        assert 0 <= r["ATE"] < 1e-5 and r["RPE trans"] < 1e-5 and r["RPE rot"] < 1e-3 and np.isfinite(r["acc"])
    assert rows[0]["acc"] < 1e-6          # the first camera of clip 0 is the world frame: the predicted points are the ground truth
    given, _ = evaluate({**cfg, "eval_camera": {"metric_names": ["ATE"], "focal": 500.0 * 48 / 640, "reproj_px": 4.0}}, dataset=ds, model=PointMapModel(),
                        save_dir=str(tmp_path / "f"), verbose=False)
    assert all(0 <= r["ATE"] < 1e-5 for r in given)
    lines = open(tmp_path / "metrics.csv").read().splitlines()
    assert lines[0] == ",acc,comp,ATE,RPE trans,RPE rot" and all(c != "" for ln in lines[1:] for c in ln.split(","))
