"""CPU: the numpy mirror of the point-cloud evaluation (harness.metrics.pcd_evaluation and its parts) against
tests/golden/pcd_golden.npz - the reference's own alignment and scores, written by tests/golden/make_pcd_golden.py -, its neighbour
search against scipy's k-d tree, ICP and normals on synthetic clouds, csrc/pcd_host.h in a stand-alone sanitizer build against numpy, and
the harness loop with ``eval_pcd`` / ``vis_pcd``."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from pcd_fixtures import small_rotation, wavy_grid, wavy_pair
from unigeo_amd.harness import SyntheticGeometryDataset, evaluate, pcd_evaluation, read_ply, world_points_from_depth, write_ply
from unigeo_amd.harness import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "pcd_golden.npz"), allow_pickle=False)
KEYS = list(M.PCD_KEYS)


# ------------------------------------------------------------------------------------------------------------------ alignment, scores
def test_alignment_matches_the_reference():
    """Shifts and gt_scale bit-equal; pred_scale (the reference takes its norm in float32: 1 ulp) and the points within
    max(1e-6, 2 x the distance the golden script measured and stored: 1.2e-7 and 2.4e-7)."""
    m = G["align_mask"].reshape(-1)
    p, g, (ps, gs, pz, gz) = M.pcd_align(G["align_pred"].reshape(-1, 3)[m], G["align_gt"].reshape(-1, 3)[m])
    ref_ps, ref_gs, ref_pz, ref_gz = G["align_scalars"]
    assert p.dtype == g.dtype == np.float32
    assert np.float32(gs) == ref_gs and np.float32(pz) == ref_pz and np.float32(gz) == ref_gz
    assert abs(float(ps) - float(ref_ps)) <= max(1e-6, 2 * float(G["scale_distance"]))
    bound = max(1e-6, 2 * float(G["point_distance"]))
    assert np.abs(p - G["align_pts"]).max() <= bound and np.abs(g - G["align_pts_gt"]).max() <= bound
    res = pcd_evaluation(G["align_pred"], G["align_gt"], G["align_mask"], G["align_rgb"])      # the same through the public function
    assert res["pred_pcd"][0].tobytes() == p.tobytes() and res["gt_pcd"][0].tobytes() == g.tobytes()
    assert np.array_equal(res["pred_pcd"][1], G["align_rgb_masked"]) and res["n_points"] == int(m.sum())
    assert (np.float32(res["pred_scale"]), np.float32(res["gt_shift_z"])) == (np.float32(ps), ref_gz)


def test_scores_match_the_reference():
    got = M.pcd_scores(G["score_gt"], G["score_pred"], G["score_gt_normals"], G["score_pred_normals"])
    for k, ref in zip(KEYS, G["score_vals"]):
        assert got[k] == pytest.approx(float(ref), rel=1e-12), k
    brute = M.pcd_scores(G["score_gt"], G["score_pred"], G["score_gt_normals"], G["score_pred_normals"], nn=M.nn_brute)
    for k, ref in zip(KEYS, G["score_vals"]):
        assert brute[k] == pytest.approx(float(ref), rel=1e-12), k


# ------------------------------------------------------------------------------------------------------------------ neighbour search
def test_brute_force_neighbours_equal_the_kd_tree():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(0)
    q, t = rng.normal(size=(700, 3)), rng.normal(size=(1300, 3))
    d, i = M.nn_brute(q, t, chunk=50000)                    # several chunks
    rd, ri = cKDTree(t).query(q)
    np.testing.assert_allclose(d, rd, rtol=0, atol=1e-12)
    assert np.array_equal(i, ri)                            # no ties in a random cloud
    d1, i1 = M.nn_brute(q, t)
    assert d1.tobytes() == d.tobytes() and np.array_equal(i1, i)


def test_ties_go_to_the_lowest_index():
    rng = np.random.default_rng(1)
    base = rng.normal(size=(50, 3))
    t = np.concatenate([base, base[::-1], base])
    d, i = M.nn_brute(base, t)
    assert np.array_equal(i, np.arange(50)) and not d.any()
    nbr = M.knn_brute(t, 5)
    ref = np.argsort(M._d2(t, t), axis=1, kind="stable")[:, :5]
    assert np.array_equal(nbr, ref)
    assert (nbr[:50, 0] == np.arange(50)).all() and (nbr[50:100, 0] == np.arange(49, -1, -1)).all()      # the first copy wins
    assert np.array_equal(M.knn_brute(base, 5), np.argsort(M._d2(base, base), axis=1, kind="stable")[:, :5])   # the fast path, no ties
    assert M.knn_brute(base[:3], 5).shape == (3, 3)


# ------------------------------------------------------------------------------------------------------------------ ICP
@pytest.fixture(scope="module")
def wavy():
    p, g = wavy_pair(4000)
    return p, g, M.pcd_metrics_from_clouds(p, g)


def test_icp_converges_on_the_wavy_surface(wavy):
    """Measured here: 7 updates, acc 1.86e-2 -> 3.14e-3, every |d rmse| before the last >= 3.6e-4, the last 7.4e-7; a 1e-7 perturbation of
    the input moves acc by less than 1e-5 relative."""
    p, g, res = wavy
    before = M._nn(p.astype(np.float64), g.astype(np.float64))[0].mean()
    assert 2 <= res["icp_iterations"] < 30 and res["icp_fitness"] == 1.0
    assert res["acc"] < 0.25 * before and res["acc"] < 2.5 * 0.002            # down to the noise: |N(0, 0.002^2 I_3)| has mean 3.2e-3
    assert res["nc1"] > 0.999 and res["nc2"] > 0.999
    R = res["transformation"][:3, :3]
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
    np.testing.assert_allclose(R, small_rotation().T, atol=2e-3)            # the inverse of the rotation that was applied
    steps = np.abs(np.diff(np.asarray(res["icp_history"]), axis=0))
    assert len(steps) == res["icp_iterations"]
    for s in steps[:-1].reshape(-1):                                          # nothing before the last update sits near the stopping bound
        assert s <= 1e-7 or s >= 1e-5, steps
    assert (steps[-1] < 1e-6).all()
    rng = np.random.default_rng(2)
    moved = M.pcd_metrics_from_clouds(p + rng.uniform(-1e-7, 1e-7, p.shape).astype(np.float32), g)
    assert moved["icp_iterations"] == res["icp_iterations"] and abs(moved["acc"] - res["acc"]) <= 1e-5 * res["acc"]


def test_icp_without_a_correspondence_returns_the_identity_after_one_update():
    p, g = wavy_pair(200)
    res = M.pcd_metrics_from_clouds(p + np.float32(50.0), g)
    assert res["icp_iterations"] == 1 and res["icp_fitness"] == 0.0 and res["icp_rmse"] == 0.0
    assert np.array_equal(res["transformation"], np.eye(4))
    assert res["acc"] > 40 and np.array_equal(M.umeyama_rigid(np.zeros((0, 3)), np.zeros((0, 3))), np.eye(4))


def test_max_iteration_caps_the_updates(wavy):
    p, g, res = wavy
    two = M.pcd_metrics_from_clouds(p, g, max_iteration=2)
    assert two["icp_iterations"] == 2 and two["acc"] > res["acc"]
    assert M.pcd_metrics_from_clouds(p, g, max_iteration=0)["icp_iterations"] == 0


# ------------------------------------------------------------------------------------------------------------------ normals
def test_normals_of_a_noisy_plane():
    rng = np.random.default_rng(3)
    n0 = np.array([1.0, -2.0, 2.0]) / 3.0
    a, b = np.linalg.svd(n0[None])[2][1:]
    pts = rng.uniform(-1, 1, (600, 1)) * a + rng.uniform(-1, 1, (600, 1)) * b + rng.normal(0, 1e-5, (600, 1)) * n0
    nrm = M.knn_normals(pts)
    np.testing.assert_allclose(np.linalg.norm(nrm, axis=-1), 1.0, atol=1e-12)
    assert np.abs(nrm @ n0).min() >= 1 - 1e-6
    for n in (1, 2):
        assert np.array_equal(M.knn_normals(pts[:n]), np.tile([0.0, 0.0, 1.0], (n, 1)))


# ------------------------------------------------------------------------------------------------------------------ pcd_host.h
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler for the stand-alone pcd_host.h program")
    exe = str(tmp_path_factory.mktemp("pcd_host") / "pcd_host_main")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "pcd_host_main.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    return np.array([[float(x) for x in l.split()] for l in out.strip().split("\n")])


def _numpy_rotation(H):
    U, _, Vt = np.linalg.svd(H)
    return U @ np.diag([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0]) @ Vt


def test_host_svd_rotation_equals_numpy_under_sanitizers(host_program):
    rng = np.random.default_rng(4)
    mats = [rng.normal(size=(3, 3)) for _ in range(40)]
    mats += [m * [1.0, 1.0, -1.0] for m in mats[:10]]                                         # reflections: the sign correction acts
    rank2 = []
    for _ in range(20):
        a, b = rng.normal(size=(3, 2)), rng.normal(size=(2, 3))
        rank2.append(a @ b)
    mats += rank2 + [np.eye(3), np.diag([3.0, 2.0, 0.0])]
    out = _run(host_program, ["h " + " ".join(repr(float(x)) for x in m.reshape(-1)) for m in mats])
    assert out.shape == (len(mats), 12)
    for m, o in zip(mats, out):
        R, w = o[:9].reshape(3, 3), o[9:]
        np.testing.assert_allclose(w, np.linalg.svd(m, compute_uv=False), atol=1e-12 * max(1.0, np.abs(m).max()))
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
        assert np.linalg.det(R) == pytest.approx(1.0, abs=1e-12)
        np.testing.assert_allclose(R, _numpy_rotation(m), atol=1e-9)
    zero = _run(host_program, ["h " + " ".join(["0"] * 9)])[0]
    assert np.array_equal(zero[:9].reshape(3, 3), np.eye(3))


def test_host_umeyama_from_sums_equals_the_mirror(host_program):
    rng = np.random.default_rng(5)
    s = rng.normal(size=(500, 3)) + [0.0, 0.0, 3.0]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = small_rotation(0.3, (2.0, -1.0, 0.5)), [0.2, -0.1, 0.05]
    d = M._move(T, s) + rng.normal(0, 1e-3, s.shape)
    sums = np.concatenate([[len(s)], s.sum(0), d.sum(0), (d.T @ s).reshape(-1), [0.0]])
    got = _run(host_program, ["sums " + " ".join(repr(float(x)) for x in sums), "sums " + " ".join(["0"] * 17)])
    np.testing.assert_allclose(got[0].reshape(4, 4), M.umeyama_rigid(s, d), atol=1e-10)
    assert np.array_equal(got[1].reshape(4, 4), np.eye(4))


# ------------------------------------------------------------------------------------------------------------------ world points
def test_world_points_share_the_arithmetic_of_the_global_depth_evaluation():
    ds = SyntheticGeometryDataset(clip_length=3, clip_overlap=1, input_size=(64, 64), num_frames=3)
    from unigeo_amd.harness import prepare_gt_label
    data = ds[0]
    gt = prepare_gt_label(data)
    K = np.stack(data["intrinsics"], 0)
    depth = gt["gt_depths"].numpy()
    pred = (0.5 * depth + 0.25).astype(np.float32)
    pts, (s_d, t_d) = world_points_from_depth(pred, depth, gt["gt_poses"], K)
    assert pts.shape == (3, 64, 64, 3) and pts.dtype == np.float32
    assert (s_d, t_d) == pytest.approx((2.0, -0.5), abs=1e-5)
    np.testing.assert_allclose(pts, gt["gt_world_pts"].numpy(), atol=2e-5)                     # the aligned depth is the ground truth again
    radius = np.linalg.norm(gt["gt_world_pts"].numpy().astype(np.float64), axis=-1).astype(np.float32)
    _, rmap, _, fit_d = M.depth_evaluation_in_global_coord(pred, depth, radius, gt["gt_poses"], K, align_with_lstsq=True, return_fits=True)
    assert fit_d == (s_d, t_d)
    clipped, _ = world_points_from_depth(pred, depth, gt["gt_poses"], K, post_clip_max=float(np.median(depth)))
    assert not np.array_equal(clipped, pts)


# ------------------------------------------------------------------------------------------------------------------ harness
class _NoisyGTModel:
    """pred = an affine image of the ground-truth depth plus seeded noise: least squares brings it back up to the noise"""

    def forward(self, data):
        d = np.stack([-np.asarray(c)[2] for c in data["cam_coord"]], 0)             # OpenGL z -> OpenCV depth
        noise = np.random.default_rng(11).normal(0.0, 2e-3, d.shape)
        return {"pred_depths": torch.from_numpy(0.5 * d + 0.2 + noise).float()}


class _WorldPointModel:
    predicts_world_points = True

    def forward(self, data):
        from unigeo_amd.harness import prepare_gt_label
        return {"pred_world_pts": prepare_gt_label(data)["gt_world_pts"] * 2.0}


class _NeverCalled:
    def forward(self, data):
        raise AssertionError("the model must not run")


class _NoIntrinsics:
    def __init__(self, ds):
        self.ds = ds

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        d = dict(self.ds[i])
        d.pop("intrinsics")
        return d


def _cfg(**pcd):
    return {"dataset": "SyntheticGeometryDataset", "root": "unused", "h": 64, "w": 64, "clip_length": 3, "clip_overlap": 1,
            "eval_depth": {"metric_names": ["Abs Rel"]},
            "eval_pcd": {"metric_names": ["acc", "comp", "nc1", "nc2"], "pcd_downsample_num": 800, **pcd}}


def test_harness_rows_carry_the_point_cloud_metrics(tmp_path):
    ds = SyntheticGeometryDataset(clip_length=3, clip_overlap=1, input_size=(64, 64), num_frames=5)
    cfg = {**_cfg(seed=5), "vis_pcd": True}
    rows, mm = evaluate(cfg, dataset=ds, model=_NoisyGTModel(), save_dir=str(tmp_path / "a"), verbose=False)
    again, _ = evaluate(cfg, dataset=ds, model=_NoisyGTModel(), save_dir=str(tmp_path / "b"), verbose=False)
    other, _ = evaluate(_cfg(seed=6), dataset=ds, model=_NoisyGTModel(), save_dir=str(tmp_path / "c"), verbose=False)
    assert len(rows) == len(ds) == 3
    for r, r2, r3 in zip(rows, again, other):
        assert all(k in r and np.isfinite(r[k]) for k in KEYS)
        assert all(r[k] == r2[k] for k in KEYS)                                    # the same seed: the same sample, the same row
        assert any(r[k] != r3[k] for k in KEYS)                                    # another seed: another sample
        assert r["acc"] < 0.05 and r["nc1"] > 0.9 and r["Abs Rel"] < 0.01
        for name in ("pred.ply", "gt.ply"):
            pts, col = read_ply(str(tmp_path / "a" / f"pcd_{r['seq_name']}" / name))
            assert pts.shape == col.shape == (800, 3) and pts.dtype == np.float32 and col.dtype == np.uint8 and np.isfinite(pts).all()
    assert not (tmp_path / "c" / f"pcd_{rows[0]['seq_name']}").exists()            # vis_pcd is off there
    text = (tmp_path / "a" / "metrics.csv").read_text().splitlines()
    assert text[0] == ",Abs Rel,acc,comp,nc1,nc2" and all(cell for cell in text[1].split(","))
    assert set(mm.calculate_averages()) == {"Abs Rel", "acc", "comp", "nc1", "nc2"}


def test_harness_uses_the_models_world_points_when_it_returns_them(tmp_path):
    ds = SyntheticGeometryDataset(clip_length=3, clip_overlap=1, input_size=(64, 64), num_frames=3)
    cfg = _cfg()
    del cfg["eval_depth"]
    rows, _ = evaluate(cfg, dataset=_NoIntrinsics(ds), model=_WorldPointModel(), save_dir=str(tmp_path), verbose=False)
    assert len(rows) == len(ds) and all(r["acc"] < 1e-3 for r in rows)                                 # the scale is aligned away


def test_harness_configuration_errors_come_before_the_first_clip(tmp_path):
    ds = SyntheticGeometryDataset(clip_length=3, clip_overlap=1, input_size=(64, 64), num_frames=5)
    cfg = _cfg()
    del cfg["eval_pcd"]
    with pytest.raises(ValueError, match="vis_pcd"):
        evaluate({**cfg, "vis_pcd": True}, dataset=ds, model=_NeverCalled(), save_dir=str(tmp_path / "x"), verbose=False)
    assert not (tmp_path / "x").exists()
    with pytest.raises(ValueError, match="intrinsics"):
        evaluate(_cfg(), dataset=_NoIntrinsics(ds), model=_NeverCalled(), save_dir=str(tmp_path / "y"), verbose=False)
    rows, _ = evaluate(cfg, dataset=ds, model=_NoisyGTModel(), save_dir=str(tmp_path / "z"), verbose=False)      # nothing changes without eval_pcd
    assert "acc" not in rows[0] and "Abs Rel" in rows[0]


def test_ply_round_trip(tmp_path):
    rng = np.random.default_rng(6)
    pts, col = rng.normal(size=(37, 3)).astype(np.float32), rng.uniform(size=(37, 3)).astype(np.float32)
    write_ply(str(tmp_path / "c.ply"), pts, col)
    raw = (tmp_path / "c.ply").read_bytes()
    assert raw.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 37\n") and len(raw) == raw.index(b"end_header\n") + 11 + 37 * 15
    back, bcol = read_ply(str(tmp_path / "c.ply"))
    assert back.tobytes() == pts.tobytes() and np.array_equal(bcol, (col * np.float32(255)).astype(np.uint8))
    write_ply(str(tmp_path / "e.ply"), np.zeros((0, 3), np.float32))
    assert read_ply(str(tmp_path / "e.ply"))[0].shape == (0, 3)


def test_downsampling_and_the_empty_mask():
    pred, gt, mask, rgb = wavy_grid(2, 24, 32, seed=1)
    n = int(mask.sum())
    full = pcd_evaluation(pred, gt, mask, rgb)
    assert full["n_points"] == n and pcd_evaluation(pred, gt, mask, rgb, downsample_num=n + 5)["acc"] == full["acc"]      # no error beyond n
    a, b = pcd_evaluation(pred, gt, mask, rgb, downsample_num=300, seed=1), pcd_evaluation(pred, gt, mask, rgb, downsample_num=300, seed=1)
    c = pcd_evaluation(pred, gt, mask, rgb, downsample_num=300, seed=2)
    assert a["n_points"] == 300 and a["acc"] == b["acc"] and a["acc"] != c["acc"]
    assert a["pred_pcd"][0].tobytes() == full["pred_pcd"][0][M.pcd_sample_indices(n, 300, 1)].tobytes()     # aligned on all points, then sampled
    assert a["gt_shift_z"] == full["gt_shift_z"] and a["pred_scale"] == full["pred_scale"]
    empty = pcd_evaluation(pred, gt, np.zeros_like(mask), rgb)
    assert empty["n_points"] == 0 and all(np.isnan(empty[k]) for k in KEYS) and np.array_equal(empty["transformation"], np.eye(4))
