"""CPU: farthest-point sampling for eval_pcd - the host mirror pcd_fps_indices of harness/metrics.py against known
answers and a scalar loop written on its own, pcd_evaluation(sampling="fps"), the configuration key and the harness loop."""
import math

import numpy as np
import pytest
import torch

from pcd_fixtures import wavy_grid, wavy_pair
from unigeo_amd.harness import SyntheticGeometryDataset, evaluate, parse_pcd_eval_config, pcd_evaluation, read_ply
from unigeo_amd.harness import metrics as M

KEYS = ("acc", "comp", "nc1", "nc2", "acc_med", "comp_med", "nc1_med", "nc2_med")
f32 = np.float32


def _line(n=9):
    return np.stack([np.arange(n, dtype=f32), np.zeros(n, f32), np.zeros(n, f32)], 1)


def test_nine_points_on_a_line():
    """0, then the far end, then the middle; 2 and 6 are both 2 away from what is picked and the lower index goes first."""
    idx, sel = M.pcd_fps_indices(_line(), 9)
    assert idx.dtype == np.int64 and sel.dtype == f32
    assert idx.tolist() == [0, 8, 4, 2, 6, 1, 3, 5, 7]
    assert sel.tolist() == [math.inf, 64.0, 16.0, 4.0, 4.0, 1.0, 1.0, 1.0, 1.0]


def test_selected_distances_do_not_increase_and_shorter_runs_are_prefixes():
    pts = wavy_pair(500, seed=2)[0]
    idx, sel = M.pcd_fps_indices(pts, 120)
    assert sel[0] == np.inf and (np.diff(sel[1:]) <= 0).all() and sel[-1] > 0
    assert len(set(idx.tolist())) == 120
    for k in (1, 2, 37):
        i2, s2 = M.pcd_fps_indices(pts, k)
        assert np.array_equal(i2, idx[:k]) and s2.tobytes() == sel[:k].tobytes()
    for bad in (0, 501):
        with pytest.raises(ValueError):
            M.pcd_fps_indices(pts, bad)


def test_non_finite_points_are_skipped():
    pts = wavy_pair(60, seed=3)[0]
    pts[0, 0], pts[1, 1], pts[2, 2], pts[3] = np.nan, np.inf, -np.inf, np.nan        # a leading run
    pts[17, 1], pts[40, 0] = np.nan, np.inf                                           # and two further on
    bad = {0, 1, 2, 3, 17, 40}
    idx, sel = M.pcd_fps_indices(pts, 54)                                             # every finite point
    assert idx[0] == 4 and not bad & set(idx.tolist()) and len(set(idx.tolist())) == 54
    assert np.isfinite(sel[1:]).all() and (sel[1:] > 0).all()
    idx, sel = M.pcd_fps_indices(pts, 56)                                             # then the distance-0 repeats; never a marked point
    assert sel[54] == 0 and sel[55] == 0 and not bad & set(idx.tolist())
    only_bad = np.full((3, 3), np.nan, f32)
    idx, sel = M.pcd_fps_indices(only_bad, 2)                                         # nothing finite: index 0 with the mark -1
    assert idx.tolist() == [0, 0] and sel.tolist() == [-1.0, -1.0]


def _fps_scalar(pts, k):
    """The statement again, one float32 operation at a time in plain Python loops."""
    n = len(pts)
    m = [f32(np.inf) if all(math.isfinite(float(c)) for c in pts[j]) else f32(-1) for j in range(n)]
    idx, sel = [], []
    for _ in range(k):
        s = 0
        for j in range(1, n):
            if m[j] > m[s]:
                s = j
        idx.append(s)
        sel.append(m[s])
        for j in range(n):
            dx, dy, dz = f32(pts[j, 0] - pts[s, 0]), f32(pts[j, 1] - pts[s, 1]), f32(pts[j, 2] - pts[s, 2])
            d = f32(f32(f32(dx * dx) + f32(dy * dy)) + f32(dz * dz))
            if d < m[j]:
                m[j] = d
    return np.array(idx, np.int64), np.array(sel, f32)


def test_the_vectorised_mirror_equals_a_scalar_loop():
    pts = wavy_pair(200, seed=4)[0]
    pts[5, 1] = np.nan
    pts[150:160] = pts[20:30]                                                          # exact repeats: ties at distance 0
    with np.errstate(invalid="ignore"):
        ref_idx, ref_sel = _fps_scalar(pts, 200)
    idx, sel = M.pcd_fps_indices(pts, 200)
    assert np.array_equal(idx, ref_idx) and sel.tobytes() == ref_sel.tobytes()


def test_sample_indices_fps_samples_each_cloud_on_its_own():
    p, g = wavy_pair(100, seed=5)
    assert M.pcd_sample_indices_fps(p, g, -1) is None and M.pcd_sample_indices_fps(p, g, 100) is None
    assert M.pcd_sample_indices_fps(p, g, 0) is None and M.pcd_sample_indices_fps(p, g, 101) is None
    ip, ig = M.pcd_sample_indices_fps(p, g, 30)
    assert np.array_equal(ip, M.pcd_fps_indices(p, 30)[0]) and np.array_equal(ig, M.pcd_fps_indices(g, 30)[0])
    assert not np.array_equal(ip, ig)


@pytest.fixture(scope="module")
def grid_case():
    pred, gt, mask, rgb = wavy_grid(2, 24, 32)
    return (pred, gt, mask, rgb), pcd_evaluation(pred, gt, mask, rgb, downsample_num=300, seed=1, sampling="fps")


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        if k in ("pred_pcd", "gt_pcd"):
            assert a[k][0].tobytes() == b[k][0].tobytes() and a[k][1].tobytes() == b[k][1].tobytes(), k
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def test_pcd_evaluation_with_fps(grid_case):
    (pred, gt, mask, rgb), res = grid_case
    n = int(mask.sum())
    assert res["n_points"] == 300
    for k in ("pred_idx", "gt_idx"):
        assert res[k].dtype == np.int64 and len(np.unique(res[k])) == 300 and res[k].min() >= 0 and res[k].max() < n
    m = mask.reshape(-1)
    p, g, scal = M.pcd_align(pred.reshape(-1, 3)[m], gt.reshape(-1, 3)[m])
    col = rgb.reshape(-1, 3)[m]
    assert np.array_equal(res["pred_idx"], M.pcd_fps_indices(p, 300)[0]) and np.array_equal(res["gt_idx"], M.pcd_fps_indices(g, 300)[0])
    assert res["pred_pcd"][0].tobytes() == p[res["pred_idx"]].tobytes() and res["gt_pcd"][0].tobytes() == g[res["gt_idx"]].tobytes()
    assert res["pred_pcd"][1].tobytes() == col[res["pred_idx"]].tobytes() and res["gt_pcd"][1].tobytes() == col[res["gt_idx"]].tobytes()
    by_hand = M.pcd_metrics_from_clouds(p[res["pred_idx"]], g[res["gt_idx"]])
    for k in KEYS + ("icp_iterations", "icp_fitness", "icp_rmse"):
        assert res[k] == by_hand[k] and np.isfinite(res[k]), k
    assert np.array_equal(res["transformation"], by_hand["transformation"])
    assert res["pred_scale"] == float(scal[0]) and res["gt_shift_z"] == float(scal[3])


def test_fps_ignores_the_seed_and_random_is_unchanged(grid_case):
    (pred, gt, mask, rgb), res = grid_case
    _same(res, pcd_evaluation(pred, gt, mask, rgb, downsample_num=300, seed=99, sampling="fps"))
    a = pcd_evaluation(pred, gt, mask, rgb, downsample_num=300, seed=4)
    b = pcd_evaluation(pred, gt, mask, rgb, downsample_num=300, seed=4, sampling="random")
    _same(a, b)
    assert "pred_idx" not in a and any(a[k] != res[k] for k in KEYS)
    with pytest.raises(ValueError, match="sampling"):
        pcd_evaluation(pred, gt, mask, rgb, downsample_num=300, sampling="grid")


def test_fps_with_every_point_is_the_unsampled_evaluation(grid_case):
    (pred, gt, mask, rgb), _ = grid_case
    n = int(mask.sum())
    plain = pcd_evaluation(pred, gt, mask, rgb)
    for down in (-1, n, n + 5):
        res = pcd_evaluation(pred, gt, mask, rgb, downsample_num=down, sampling="fps")
        assert np.array_equal(res.pop("pred_idx"), np.arange(n)) and np.array_equal(res.pop("gt_idx"), np.arange(n))
        _same(res, plain)
    empty = pcd_evaluation(pred, gt, np.zeros_like(mask), rgb, downsample_num=300, sampling="fps")
    assert empty["n_points"] == 0 and len(empty["pred_idx"]) == 0 and all(np.isnan(empty[k]) for k in KEYS)


# ------------------------------------------------------------------------------------------------------------------ configuration, harness
class _NoisyGTModel:
    """pred = an affine image of the ground-truth depth plus seeded noise"""

    def forward(self, data):
        d = np.stack([-np.asarray(c)[2] for c in data["cam_coord"]], 0)             # OpenGL z -> OpenCV depth
        noise = np.random.default_rng(11).normal(0.0, 2e-3, d.shape)
        return {"pred_depths": torch.from_numpy(0.5 * d + 0.2 + noise).float()}


class _NeverTouched:
    def __len__(self):
        raise AssertionError("the dataset must not be touched")

    def __getitem__(self, i):
        raise AssertionError("the dataset must not be touched")


def _cfg(**pcd):
    return {"dataset": "SyntheticGeometryDataset", "root": "unused", "h": 64, "w": 64, "clip_length": 3, "clip_overlap": 1,
            "eval_depth": {"metric_names": ["Abs Rel"]},
            "eval_pcd": {"metric_names": ["acc", "comp", "nc1", "nc2"], "pcd_downsample_num": 400, **pcd}}


def test_the_sampling_key_is_parsed_and_checked(tmp_path):
    assert parse_pcd_eval_config(_cfg())["sampling"] == "random"
    assert parse_pcd_eval_config(_cfg(sampling="random"))["sampling"] == "random"
    assert parse_pcd_eval_config(_cfg(sampling="fps"))["sampling"] == "fps"
    with pytest.raises(ValueError, match="sampling"):
        parse_pcd_eval_config(_cfg(sampling="grid"))
    with pytest.raises(ValueError, match="sampling"):
        evaluate(_cfg(sampling="grid"), dataset=_NeverTouched(), model=_NoisyGTModel(), save_dir=str(tmp_path / "x"), verbose=False)
    assert not (tmp_path / "x").exists()


def test_harness_rows_under_fps_equal_the_direct_call(tmp_path):
    from unigeo_amd.harness import prepare_gt_label, world_points_from_depth
    ds = SyntheticGeometryDataset(clip_length=3, clip_overlap=1, input_size=(64, 64), num_frames=3)
    cfg = {**_cfg(sampling="fps", seed=5), "vis_pcd": True}
    rows, _ = evaluate(cfg, dataset=ds, model=_NoisyGTModel(), save_dir=str(tmp_path / "a"), verbose=False)
    other, _ = evaluate(_cfg(sampling="fps", seed=6), dataset=ds, model=_NoisyGTModel(), save_dir=str(tmp_path / "b"), verbose=False)
    assert len(rows) == len(ds) == 2
    for i, (row, row2) in enumerate(zip(rows, other)):
        data = ds[i]
        gt = prepare_gt_label(data)
        pts = world_points_from_depth(_NoisyGTModel().forward(data)["pred_depths"], gt["gt_depths"], gt["gt_poses"],
                                      np.stack(data["intrinsics"], 0))[0]
        ref = pcd_evaluation(pts, gt["gt_world_pts"], gt["gt_masks"], gt["gt_rgbs"], downsample_num=400, sampling="fps")
        for k in KEYS:
            assert row[k] == ref[k] == row2[k] and np.isfinite(row[k]), k                 # the direct call; and no seed enters
        assert not np.array_equal(ref["pred_idx"], ref["gt_idx"])
        for name, key in (("pred.ply", "pred_pcd"), ("gt.ply", "gt_pcd")):                # each cloud with the colours of its own points
            p, col = read_ply(str(tmp_path / "a" / f"pcd_{row['seq_name']}" / name))
            assert p.tobytes() == ref[key][0].tobytes()
            assert np.array_equal(col, (np.clip(ref[key][1], 0.0, 1.0) * np.float32(255)).astype(np.uint8))
    text = (tmp_path / "a" / "metrics.csv").read_text().splitlines()
    assert text[0] == ",Abs Rel,acc,comp,nc1,nc2"
