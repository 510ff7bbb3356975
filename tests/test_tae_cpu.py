"""CPU: the temporal alignment error's numpy mirror (unigeo_amd/harness/temporal.py) against closed forms, against the
independent per-pixel oracle of tests/tae_fixtures.py, at its edge cases, and through the harness key ``eval_temporal``."""
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from tae_fixtures import (SMALL_CASES, assert_scene_conditions, bad_pixel_scene, check_flicker, check_plane_shift, contest_case, disparity_scene,      # noqa: E402
                          eye_poses, facing_apart_scene, flicker_case, make_scene, pinhole, plane_shift_case, same_bytes, tae_oracle)

from unigeo_amd.harness import (SyntheticGeometryDataset, aligned_depth, evaluate, parse_metric_config, parse_temporal_eval_config,      # noqa: E402
                                prepare_gt_label, relative_poses, temporal_alignment_error, warp_depth)

F32 = np.float32


def test_flicker_closed_form():
    sc, want = flicker_case()
    res = temporal_alignment_error(sc["pred"], sc["gt"], sc["poses"], sc["K"], sc["fit"], return_maps=True)
    check_flicker(res, want)
    for p, (a, _) in enumerate([(0, 1), (1, 0), (1, 2), (2, 1)]):
        assert same_bytes(res["warp"][p], sc["pred"][a])


def test_plane_shift_closed_form():
    sc = plane_shift_case()
    check_plane_shift(temporal_alignment_error(sc["pred"], sc["gt"], sc["poses"], sc["K"], sc["fit"], return_maps=True))


def _against_oracle(sc, **kw):
    got = temporal_alignment_error(sc["pred"], sc["gt"], sc["poses"], sc["K"], sc["fit"], custom_mask=sc["mask"], return_maps=True, **kw)
    ref = tae_oracle(sc["pred"], sc["gt"], sc["poses"], sc["K"], sc["fit"], sc["mask"], **kw)
    assert same_bytes(got["warp"], ref["warp"]) and same_bytes(got["err"], ref["err"])
    assert (got["pair_values"][:, 1] == ref["pair_values"][:, 1]).all()
    np.testing.assert_allclose(got["pair_values"][:, 0], ref["pair_values"][:, 0], rtol=1e-12, atol=0, equal_nan=True)
    for k in ("TAE pairs", "TAE pairs total", "TAE pixels"):
        assert got[k] == ref[k], k
    assert got["TAE"] == pytest.approx(ref["TAE"], rel=1e-12, nan_ok=True)
    return got, ref


@pytest.mark.parametrize("T,H,W,stride,seed", SMALL_CASES)
def test_mirror_equals_the_oracle(T, H, W, stride, seed):
    got, ref = _against_oracle(make_scene(T, H, W, seed), stride=stride)
    assert_scene_conditions(ref["pair_values"], ref["hits"], H, W)
    assert got["TAE pairs"] == got["TAE pairs total"] == 2 * (T - stride) and 0 < got["TAE"] < 1


def test_pieces_are_public():
    T, H, W, stride, seed = SMALL_CASES[2]
    sc = make_scene(T, H, W, seed)
    rel = relative_poses(sc["poses"], stride)
    assert rel.shape == (2 * (T - stride), 3, 4) and rel.dtype == np.float64
    C = sc["poses"].astype(np.float64)
    assert same_bytes(rel[1], (np.linalg.inv(C[0]) @ C[stride])[:3])
    d = aligned_depth(sc["pred"], sc["fit"])
    assert d.dtype == F32 and same_bytes(d, sc["pred"] * sc["fit"][0] + sc["fit"][1])
    ref = tae_oracle(sc["pred"], sc["gt"], sc["poses"], sc["K"], sc["fit"], stride=stride)
    assert same_bytes(warp_depth(d, sc["K"], rel, stride), ref["warp"])


def test_t_equal_to_stride_gives_nan_and_no_pairs():
    sc = make_scene(*SMALL_CASES[0][:3], SMALL_CASES[0][4])
    for stride in (3, 5):
        res = temporal_alignment_error(sc["pred"], sc["gt"], sc["poses"], sc["K"], sc["fit"], stride=stride, return_maps=True)
        assert math.isnan(res["TAE"]) and res["TAE pairs"] == res["TAE pairs total"] == res["TAE pixels"] == 0
        assert res["warp"].shape == (0, 5, 7) and res["pair_values"].shape == (0, 2)
    with pytest.raises(ValueError):
        temporal_alignment_error(sc["pred"], sc["gt"], sc["poses"], sc["K"], sc["fit"], stride=0)


def test_a_pair_facing_apart_is_left_out_not_scored_as_zero():
    sc = facing_apart_scene()
    got, _ = _against_oracle(sc)
    v = got["pair_values"]
    assert got["TAE pairs"] == 2 and got["TAE pairs total"] == 4
    assert (v[2:, 1] == 0).all() and np.isnan(v[2:, 0]).all() and not got["warp"][2:].any()
    assert got["TAE"] == float(v[:2, 0].mean()) and got["TAE"] > 0.5 * v[:2, 0].max()      # the mean of two pairs, not of four with two zeros


def test_bad_pixels_and_a_nan_pose_are_dropped_quietly():
    sc = bad_pixel_scene()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = temporal_alignment_error(sc["pred"], sc["gt"], sc["poses"], sc["K"], sc["fit"], custom_mask=sc["mask"], return_maps=True)
    _against_oracle(sc)
    assert got["TAE pairs"] == 4 and got["TAE pairs total"] == 6 and math.isfinite(got["TAE"])      # the pairs of frame 3 reach nothing
    assert np.isfinite(got["warp"]).all() and np.isfinite(got["err"]).all()


def test_points_behind_the_target_camera_are_dropped():
    T, H, W = 2, 6, 8
    d = np.full((T, H, W), 2.0, F32)
    poses = eye_poses(T)
    poses[1, 2, 3] = 3.0      # camera 1 stands behind the surface camera 0 sees
    res = temporal_alignment_error(d, d, poses, pinhole(T, 8, 8, W / 2, H / 2), (1.0, 0.0), return_maps=True)
    assert not res["warp"][0].any() and res["pair_values"][0, 1] == 0
    assert set(np.unique(res["warp"][1])) == {0.0, 5.0} and res["pair_values"][1, 1] > 0
    assert res["TAE pairs"] == 1 and res["TAE"] == 1.5      # |5 - 2| / 2


def test_the_nearest_of_contesting_sources_wins():
    d, K = contest_case()
    res = temporal_alignment_error(d, d, eye_poses(2), K, (1.0, 0.0), return_maps=True)
    ref = tae_oracle(d, d, eye_poses(2), K, (1.0, 0.0))
    assert ref["hits"][0, 0, 0] == 4 and same_bytes(res["warp"], ref["warp"])
    assert res["warp"][0, 0, 0] == d[0, :2, :2].min()                # rint(0.5) = 0: rows and columns 0 and 1 fold onto 0
    assert res["warp"][0, 1, 2] == d[0, 2, 3:6].min()                # rint(1.5) = rint(2.5) = 2


@pytest.mark.parametrize("kw", [{"space": "disparity"}, {"space": "disparity", "disp_clip_min": 0.3},
                                {"space": "disparity", "disp_clip_min": 0.3, "post_clip_min": 2.0, "post_clip_max": 3.0},
                                {"post_clip_min": 2.0, "post_clip_max": 3.2}, {"post_clip_max": 3.0, "max_depth": 3.1}, {"max_depth": None}])
def test_disparity_space_and_clips(kw):
    sc = disparity_scene() if kw.get("space") == "disparity" else make_scene(*SMALL_CASES[1][:3], SMALL_CASES[1][4])
    got, _ = _against_oracle(sc, **kw)
    assert got["TAE pairs"] == 6 and math.isfinite(got["TAE"])
    if "disp_clip_min" in kw and "post_clip_max" not in kw:
        assert np.isclose(got["warp"].max(), 1 / 0.3, rtol=0.2) and got["warp"].max() > 3.0      # the floor bounds the depth
    with pytest.raises(ValueError):
        temporal_alignment_error(sc["pred"], sc["gt"], sc["poses"], sc["K"], sc["fit"], space="depth", disp_clip_min=0.1)


# ---------------------------------------------------------------------------------------------------------------- configuration and harness
class _GTModel:
    """pred = the ground-truth depth"""

    def forward(self, data):
        d = np.stack([-np.asarray(c)[2] for c in data["cam_coord"]], 0)
        return {"pred_depths": torch.from_numpy(d).float()}


class _NeverCalled:
    def forward(self, data):
        raise AssertionError("the model must not run")


class _NoIntrinsics:
    def __init__(self, ds):
        self.ds = ds

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        return {k: v for k, v in self.ds[i].items() if k != "intrinsics"}


def _cfg(temporal=None, **eval_depth):
    cfg = {"dataset": "SyntheticGeometryDataset", "root": "unused", "h": 48, "w": 64, "clip_length": 3, "clip_overlap": 1,
           "eval_depth": {"metric_names": ["Abs Rel", "delta < 1.25"], **eval_depth}}
    if temporal is not None:
        cfg["eval_temporal"] = temporal
    return cfg


def _ds():
    return SyntheticGeometryDataset(clip_length=3, clip_overlap=1, input_size=(48, 64), num_frames=5)


def test_parse_temporal_eval_config():
    assert parse_temporal_eval_config(_cfg()) is None
    assert parse_temporal_eval_config(_cfg({"metric_names": ["TAE"]})) == {"stride": 1, "gt": False}
    assert parse_temporal_eval_config(_cfg({"metric_names": ["TAE", "TAE gt"], "stride": 2})) == {"stride": 2, "gt": True}
    assert parse_metric_config(_cfg({"metric_names": ["TAE", "TAE gt"]})) == ["Abs Rel", "delta < 1.25", "TAE", "TAE gt"]
    with pytest.raises(ValueError, match="unknown key"):
        parse_temporal_eval_config(_cfg({"metric_names": ["TAE"], "strides": 2}))
    for bad in (0, -1, 1.5, True, "2", None):
        with pytest.raises(ValueError, match="stride"):
            parse_temporal_eval_config(_cfg({"metric_names": ["TAE"], "stride": bad}))
    with pytest.raises(ValueError, match="eval_depth"):
        parse_temporal_eval_config({"eval_temporal": {"metric_names": ["TAE"]}})
    with pytest.raises(ValueError, match="global"):
        parse_temporal_eval_config(_cfg({"metric_names": ["TAE"]}, coord="global"))


@pytest.mark.parametrize("bad", ["unknown_key", "stride", "no_eval_depth", "global", "no_intrinsics"])
def test_evaluate_rejects_a_bad_configuration_before_the_first_clip_runs(tmp_path, bad):
    ds, cfg = _ds(), _cfg({"metric_names": ["TAE"]})
    if bad == "unknown_key":
        cfg["eval_temporal"]["window"] = 3
    elif bad == "stride":
        cfg["eval_temporal"]["stride"] = 0
    elif bad == "no_eval_depth":
        del cfg["eval_depth"]
    elif bad == "global":
        cfg["eval_depth"]["coord"] = "global"
    else:
        ds = _NoIntrinsics(ds)
    with pytest.raises(ValueError, match="eval_temporal"):
        evaluate(cfg, dataset=ds, model=_NeverCalled(), save_dir=str(tmp_path / "x"), verbose=False)


def test_evaluate_fills_tae_and_tae_gt(tmp_path):
    ds = _ds()
    rows, mm = evaluate(_cfg({"metric_names": ["TAE", "TAE gt"]}), dataset=ds, model=_GTModel(), save_dir=str(tmp_path / "t"), verbose=False)
    plain, _ = evaluate(_cfg(), dataset=ds, model=_GTModel(), save_dir=str(tmp_path / "p"), verbose=False)
    assert len(rows) == len(plain) == len(ds) == 3
    for i, (r, q) in enumerate(zip(rows, plain)):
        assert set(q) == {"seq_name", "Abs Rel", "Sq Rel", "RMSE", "Log RMSE", "delta < 1.", "delta < 1.25", "delta < 1.25^2", "delta < 1.25^3",
                          "valid_pixels"}                                        # without the key: the rows as they were
        assert {k: r[k] for k in q} == q and set(r) - set(q) == {"TAE", "TAE gt", "TAE pairs", "TAE pairs total", "TAE pixels"}
        gt = prepare_gt_label(ds[i])
        K = np.stack([np.asarray(k, F32) for k in ds[i]["intrinsics"]], 0)
        want = temporal_alignment_error(gt["gt_depths"], gt["gt_depths"], gt["gt_poses"], K, (1.0, 0.0), custom_mask=gt["gt_masks"])
        assert r["TAE gt"] == want["TAE"] and r["TAE pairs"] == r["TAE pairs total"] == 4 and r["TAE pixels"] > 0.25 * 4 * 48 * 64
        assert 0 <= r["TAE"] < 0.05 and r["TAE"] == pytest.approx(r["TAE gt"], abs=1e-4)      # the model returns the ground truth
    head = (tmp_path / "t" / "metrics.csv").read_text().splitlines()[0]
    assert head == ",Abs Rel,delta < 1.25,TAE,TAE gt"
    assert (tmp_path / "p" / "metrics.csv").read_text().splitlines()[0] == ",Abs Rel,delta < 1.25"
    assert not math.isnan(mm.calculate_averages()["TAE"])
