"""CPU: the host restatement of the reference's depth evaluation in global coordinates (harness.metrics.depth_evaluation_in_global_coord,
DESIGN.md section 14) against tests/golden/depth_global_golden.npz - the reference's own outputs, written by
tests/golden/make_depth_global_golden.py - and the harness loop honouring ``eval_depth.coord``.

Bounds: metrics rel max(3e-5, 2 x metric_distance), abs 1e-6 - the project's bound for device least squares against the reference, and
twice the distance the fixture's generator measured between the reference and a CPU emulation of the device's arithmetic (two chained
fits); radius map rtol max(1e-5, 2 x map_distance), atol 1e-6 - the error-map bound under lstsq.  Both distances are stored in the fixture;
neither comes from the code under test."""
import os

import numpy as np
import pytest
import torch

from unigeo_amd.harness import (SyntheticGeometryDataset, depth_evaluation, depth_evaluation_in_global_coord, evaluate, parse_depth_coord,
                                prepare_gt_label)

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "depth_global_golden.npz"), allow_pickle=False)
KEYS = [str(k) for k in G["keys"]]
CLIPS = dict(zip(("pre_clip_min", "pre_clip_max", "post_clip_min", "post_clip_max"), (float(c) for c in G["clips"])))
METRIC_REL = max(3e-5, 2.0 * float(G["metric_distance"]))
MAP_RTOL = max(1e-5, 2.0 * float(G["map_distance"]))


def test_fixture_holds_what_the_tests_assume():
    gt, pred, gr = G["gt"], G["pred"], G["gt_radius"]
    assert tuple(G["clips"]) == (1.0, 4.0, 0.8, 5.0) and pred.shape == (3, 20, 28) and pred.dtype == np.float32
    m1 = (gt > 0) & (gt < 80)
    assert (gt == 0).any() and (gt == 90).sum() == 1 and (pred < 0).any() and not G["mask"].all()
    assert gr[m1].min() >= 0.3
    K, P = G["K"], G["poses"]
    assert K.shape == (3, 3, 3) and P.shape == (3, 4, 4) and K.dtype == P.dtype == np.float32
    for a in range(3):
        assert not np.allclose(P[a, :3, :3], P[a, :3, :3].T, atol=1e-2)            # rotated: a transposed R is another matrix
        for b in range(a + 1, 3):
            assert not np.allclose(K[a], K[b]) and not np.allclose(P[a], P[b], atol=1e-2)
    assert 0 <= float(G["metric_distance"]) < 1e-3 and 0 <= float(G["map_distance"]) < 1e-3


@pytest.mark.parametrize("clip", ["noclip", "clip"])
def test_host_matches_the_reference(clip):
    res, rmap = depth_evaluation_in_global_coord(G["pred"], G["gt"], G["gt_radius"], G["poses"], G["K"], custom_mask=G["mask"],
                                                 align_with_lstsq=True, **(CLIPS if clip == "clip" else {}))
    want = G[f"{clip}_vals"]
    for k, w_ in zip(KEYS[:8], want):
        assert res[k] == pytest.approx(w_, rel=METRIC_REL, abs=1e-6), k
    assert res["valid_pixels"] == int(want[8])
    ref, eq = G[f"{clip}_map"], G[f"{clip}_map_equal"]
    assert rmap.shape == ref.shape and rmap.dtype == np.float32
    assert np.array_equal(rmap.view(np.uint32)[eq], ref.view(np.uint32)[eq])       # bit-equal where the generator's emulation was
    np.testing.assert_allclose(rmap, ref, rtol=MAP_RTOL, atol=1e-6)


def test_host_accepts_torch_tensors_and_returns_the_fits():
    t = torch.from_numpy
    a = depth_evaluation_in_global_coord(G["pred"], G["gt"], G["gt_radius"], G["poses"], G["K"], custom_mask=G["mask"], align_with_lstsq=True,
                                         return_fits=True)
    b = depth_evaluation_in_global_coord(t(G["pred"]), t(G["gt"]), t(G["gt_radius"]), t(G["poses"]), t(G["K"]), custom_mask=t(G["mask"]),
                                         align_with_lstsq=True, return_fits=True)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2:] == b[2:]
    s_r, t_r, s_d, t_d = (float(v) for v in G["noclip_emu_fits"])
    assert a[2] == pytest.approx((s_r, t_r), rel=1e-5) and a[3] == pytest.approx((s_d, t_d), rel=1e-5)


def _synthetic_clip(h=20, w=28, nf=3):
    ds = SyntheticGeometryDataset(clip_length=nf, clip_overlap=1, input_size=(h, w), num_frames=nf)
    data = ds[0]
    gt = prepare_gt_label(data)
    K = np.stack(data["intrinsics"], 0)
    return gt["gt_depths"].numpy(), K


def _radius(depth, K, poses):
    """|R p + t| of the back-projected depth in float64, rounded once"""
    T, H, W = depth.shape
    col, row = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
    z = depth.astype(np.float64)
    K, poses = K.astype(np.float64), poses.astype(np.float64)
    x = (col - K[:, None, None, 0, 2]) * z / K[:, None, None, 0, 0]
    y = (row - K[:, None, None, 1, 2]) * z / K[:, None, None, 1, 1]
    world = np.einsum("tij,thwj->thwi", poses[:, :3, :3], np.stack([x, y, z], -1)) + poses[:, None, None, :3, 3]
    return np.linalg.norm(world, axis=-1).astype(np.float32)


def test_identity_pose_and_the_true_depth_give_zero_error():
    depth, K = _synthetic_clip()
    eye = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    gr = _radius(depth, K, eye)
    res, rmap = depth_evaluation_in_global_coord(depth, depth, gr, eye, K, align_with_lstsq=True)
    assert res["valid_pixels"] == depth.size and res["Abs Rel"] < 1e-5 and res["delta < 1.25"] == 1.0
    np.testing.assert_allclose(rmap, gr, rtol=1e-5)


def test_a_depth_bent_per_frame_scores_worse_in_global_coordinates():
    """Frame k scaled by 1 + 0.1 k: one (s, t) cannot undo it.  The world origin lies INSIDE the scene, 1 in front of every camera
    (t = R (0, 0, -1), a different R per frame), as it does when a sequence's first camera is the origin and later ones look back at it:
    near the optical axis r = z - 1, both fits are affine in the prediction, so the residual the first fit leaves in depth is the
    residual the second leaves in radius - over a target smaller by 1 (depth 2.5 .. 2.9).  The bend costs more in the world."""
    depth, K = _synthetic_clip()
    poses = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    for k in range(3):
        c, s_ = np.cos(0.3 * k), np.sin(0.3 * k)
        R = np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]])
        poses[k, :3, :3] = R
        poses[k, :3, 3] = R @ np.array([0.0, 0.0, -1.0])
    gr = _radius(depth, K, poses)
    assert gr.min() >= 0.3
    bent = depth * (1.0 + 0.1 * np.arange(3, dtype=np.float32))[:, None, None]
    res_g, _ = depth_evaluation_in_global_coord(bent, depth, gr, poses, K, align_with_lstsq=True)
    res_c, _ = depth_evaluation(bent, depth, align_with_lstsq=True)
    exact, _ = depth_evaluation_in_global_coord(depth, depth, gr, poses, K, align_with_lstsq=True)
    assert exact["Abs Rel"] < 1e-5
    assert res_g["valid_pixels"] == res_c["valid_pixels"] == depth.size and res_c["Abs Rel"] > 1e-2
    assert res_g["Abs Rel"] > res_c["Abs Rel"]


def test_mask1_comes_from_the_depth_not_from_the_radius():
    gr = G["gt_radius"].copy()
    gr[0, 10] = 100.0                                                              # a radius beyond max_depth stays a valid target
    res, _ = depth_evaluation_in_global_coord(G["pred"], G["gt"], gr, G["poses"], G["K"], align_with_lstsq=True)
    assert res["valid_pixels"] == int(((G["gt"] > 0) & (G["gt"] < 80)).sum())
    res, _ = depth_evaluation_in_global_coord(G["pred"], G["gt"], gr, G["poses"], G["K"], align_with_lstsq=True, max_depth=None)
    assert res["valid_pixels"] == int((G["gt"] > 0).sum())


def test_no_valid_pixel_returns_the_zeros_convention():
    pred, gt = np.ones((2, 4, 5), np.float32), np.zeros((2, 4, 5), np.float32)
    res, rmap, fit_r, fit_d = depth_evaluation_in_global_coord(pred, gt, np.ones_like(gt), G["poses"][:2], G["K"][:2], custom_mask=np.ones(gt.shape, bool),
                                                               align_with_lstsq=True, return_fits=True, **CLIPS)
    assert all(res[k] == 0 for k in KEYS[:8]) and res["valid_pixels"] == 0
    assert fit_r == (0.0, 0.0) and fit_d == (0.0, 0.0)
    assert rmap.shape == gt.shape and rmap.dtype == np.float32 and not rmap.any()


def test_only_least_squares_is_accepted():
    args = (G["pred"], G["gt"], G["gt_radius"], G["poses"], G["K"])
    with pytest.raises(ValueError, match="align_with_lstsq"):
        depth_evaluation_in_global_coord(*args)
    with pytest.raises(ValueError, match="align_with_lstsq"):
        depth_evaluation_in_global_coord(*args, align_with_lstsq=False, metric_scale=True)
    for flag in ("disp_input", "align_with_lad", "align_with_lad2"):
        with pytest.raises(NotImplementedError):
            depth_evaluation_in_global_coord(*args, align_with_lstsq=True, **{flag: True})


class _GTModel:
    """pred = the ground-truth depth"""

    def forward(self, data):
        d = np.stack([-np.asarray(c)[2] for c in data["cam_coord"]], 0)             # OpenGL z -> OpenCV depth
        return {"pred_depths": torch.from_numpy(d).float()}


class _NeverCalled:
    def forward(self, data):
        raise AssertionError("the model must not run")


def _cfg(**eval_depth):
    return {"dataset": "SyntheticGeometryDataset", "root": "unused", "h": 64, "w": 64, "clip_length": 3, "clip_overlap": 1,
            "eval_depth": {"metric_names": ["Abs Rel", "delta < 1.25"], **eval_depth}}


def test_parse_depth_coord():
    assert parse_depth_coord({}) == "camera" and parse_depth_coord(_cfg()) == "camera" and parse_depth_coord(_cfg(coord="camera")) == "camera"
    assert parse_depth_coord(_cfg(coord="global")) == "global" and parse_depth_coord(_cfg(coord="global", depth_alignment="lstsq")) == "global"
    with pytest.raises(ValueError, match="coord"):
        parse_depth_coord(_cfg(coord="world"))
    with pytest.raises(ValueError, match="lstsq"):
        parse_depth_coord(_cfg(coord="global", depth_alignment="median"))
    assert parse_depth_coord(_cfg(coord="camera", depth_alignment="median")) == "camera"


@pytest.mark.parametrize("bad", [{"coord": "world"}, {"coord": "global", "depth_alignment": "median"}])
def test_evaluate_rejects_a_bad_coord_before_the_first_clip(tmp_path, bad):
    ds = SyntheticGeometryDataset(clip_length=3, clip_overlap=1, input_size=(64, 64), num_frames=5)
    with pytest.raises(ValueError):
        evaluate(_cfg(**bad), dataset=ds, model=_NeverCalled(), save_dir=str(tmp_path / "x"), verbose=False)
    assert not (tmp_path / "x").exists()


def test_evaluate_in_global_coordinates_on_the_host(tmp_path):
    ds = SyntheticGeometryDataset(clip_length=3, clip_overlap=1, input_size=(64, 64), num_frames=5)
    rows, mm = evaluate(_cfg(coord="global"), dataset=ds, model=_GTModel(), save_dir=str(tmp_path), verbose=False)
    assert len(rows) == len(ds) == 3
    for r in rows:
        assert r["Abs Rel"] < 1e-4 and r["delta < 1.25"] == 1.0 and r["valid_pixels"] == 3 * 64 * 64
    assert set(mm.calculate_averages()) == {"Abs Rel", "delta < 1.25"} and (tmp_path / "metrics.csv").exists()
