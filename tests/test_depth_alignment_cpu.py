"""CPU: the host restatement of the reference's depth alignment modes (harness.metrics.depth_evaluation: metric / median / scale / lstsq,
pre- and post-alignment clamps, error map) against tests/golden/depth_alignment_golden.npz - the reference's own outputs, written by
tests/golden/make_depth_alignment_golden.py - and the harness loop honouring ``eval_depth.depth_alignment``."""
import os

import numpy as np
import pytest
import torch

from unigeo_amd.harness import SyntheticGeometryDataset, depth_evaluation, evaluate

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "depth_alignment_golden.npz"), allow_pickle=False)
KEYS = [str(k) for k in G["keys"]]
MODES = {"metric": {"metric_scale": True}, "median": {}, "scale": {"align_with_scale": True}, "lstsq": {"align_with_lstsq": True}}
CLIPS = dict(zip(("pre_clip_min", "pre_clip_max", "post_clip_min", "post_clip_max"), (float(c) for c in G["clips"])))
CASES = [(tag, mode, clip) for tag in ("a", "q", "e") for mode in MODES for clip in ("noclip", "clip")]


def _run(tag, mode, clip, **kw):
    return depth_evaluation(G[f"{tag}_pred"], G[f"{tag}_gt"], custom_mask=G[f"{tag}_mask"], **MODES[mode],
                            **(CLIPS if clip == "clip" else {}), **kw)


def test_fixture_holds_what_the_tests_assume():
    assert tuple(G["clips"]) == (1.0, 4.0, 0.8, 5.0) and G["a_pred"].shape == (3, 20, 28)
    valid = lambda t: int(((G[f"{t}_gt"] > 0) & (G[f"{t}_gt"] < 80)).sum())
    assert valid("a") % 2 == 1 and valid("e") % 2 == 0 and valid("a") < 1680       # odd / even counts, invalid pixels present
    assert (G["a_gt"] == 90).sum() == 1 and (G["a_pred"] < 0).any() and not G["a_mask"].all()
    assert len(np.unique(G["q_pred"])) == 8
    assert 0 < float(G["scale_distance"]) < 0.1


@pytest.mark.parametrize("tag,mode,clip", [c for c in CASES if c[1] != "scale"])
def test_host_modes_match_the_reference(tag, mode, clip):
    """metric / median / lstsq: every metric within the project's G5 bound (rel 2e-5, abs 1e-6) of the reference's own result.
    Error map: rtol 1e-5.  With s equal as float32 (metric, median) the map repeats the reference's float32 operations and needs
    no absolute term.  Under lstsq s and t come out of a float32 LAPACK solve whose last bits are not pinned across builds; a
    relative change d of s moves a map entry |s p + t - g| / g by d * s p / g whatever the entry's own size, so entries near zero
    get the absolute term 1e-6 (the abs of the metric bound: 8 float32 roundings at s p / g of order 1)."""
    res, (s, t), emap = _run(tag, mode, clip, return_error_map=True)
    want = G[f"{tag}_{mode}_{clip}_vals"]
    for k, w in zip(KEYS[:8], want):
        assert res[k] == pytest.approx(w, rel=2e-5, abs=1e-6), k
    assert res["valid_pixels"] == int(want[8])
    assert emap.shape == G[f"{tag}_gt"].shape and emap.dtype == np.float32
    np.testing.assert_allclose(emap, G[f"{tag}_{mode}_{clip}_emap"], rtol=1e-5, atol=1e-6 if mode == "lstsq" else 0)
    if mode != "lstsq":
        assert np.float32(s) == G[f"{tag}_{mode}_{clip}_s"] and t == 0.0       # equal as float32
    if mode == "metric":
        assert (s, t) == (1.0, 0.0)


@pytest.mark.parametrize("tag,clip", [(t, c) for t in ("a", "q", "e") for c in ("noclip", "clip")])
def test_host_scale_mode_within_twice_the_measured_distance(tag, clip):
    """``scale`` is ill-conditioned: the reference's float32 result and the float64 restatement differ by the
    distance the fixture's generator measured and stored; the bound is twice that stored number, never one taken from this code."""
    bound = 2.0 * float(G["scale_distance"])
    res, (s, t), emap = _run(tag, "scale", clip, return_error_map=True)
    want = G[f"{tag}_scale_{clip}_vals"]
    for k, w in zip(KEYS[:8], want):
        assert res[k] == pytest.approx(w, rel=bound, abs=1e-6), k
    assert res["valid_pixels"] == int(want[8]) and t == 0.0
    assert s == pytest.approx(float(G[f"{tag}_scale_{clip}_s"]), rel=bound)
    # the map is the stated formula at the returned s, in the reference's float32 operations
    p, g = G[f"{tag}_pred"], G[f"{tag}_gt"]
    m1 = (g > 0) & (g < 80)
    ref = np.zeros_like(g)
    ref[m1] = np.abs(p[m1] * np.float32(s) - g[m1]) / g[m1]
    np.testing.assert_array_equal(emap, ref)


def test_lower_median_on_an_even_count_and_on_ties():
    gt = np.array([[1.0, 2.0, 3.0, 4.0, 0.0, 100.0]], np.float32)               # 4 valid pixels
    pred = np.array([[8.0, 2.0, 6.0, 4.0, 1.0, 1.0]], np.float32)
    _, (s, t) = depth_evaluation(pred, gt)
    assert s == float(np.float32(2.0) / np.float32(4.0)) and t == 0.0           # lower medians: gt 2 of (1,2,3,4), pred 4 of (2,4,6,8); not 2.5 / 5
    _, (s, _) = depth_evaluation(pred, gt, max_depth=None)                      # gt = 100 now valid: 5 pixels, medians 3 and 4
    assert s == float(np.float32(3.0) / np.float32(4.0))
    # ties: the quantised fixture's median is one of its 8 levels
    p, g = G["q_pred"], G["q_gt"]
    m1 = (g > 0) & (g < 80)
    _, (s, _) = depth_evaluation(p, g)
    med_p = np.sort(p[m1])[(m1.sum() - 1) // 2]
    assert med_p in np.unique(p) and s == float(np.sort(g[m1])[(m1.sum() - 1) // 2] / med_p)


def test_pre_clip_feeds_the_alignment_and_the_error_map_uses_the_original_prediction():
    gt = np.array([[2.0, 2.0, 2.0]], np.float32)
    pred = np.array([[0.5, 1.0, 9.0]], np.float32)
    res, (s, _), emap = depth_evaluation(pred, gt, pre_clip_min=1.0, pre_clip_max=1.0, return_error_map=True)
    assert s == 2.0 and res["Abs Rel"] == 0.0                                   # every pixel clamps to 1 -> median 1 -> s = 2 -> exact
    np.testing.assert_array_equal(emap, np.abs(pred * np.float32(2.0) - gt) / gt)
    res, _ = depth_evaluation(pred, gt, metric_scale=True, post_clip_min=2.0, post_clip_max=2.0)
    assert res["Abs Rel"] == 0.0


def test_flag_precedence_follows_the_reference():
    p, g, m = G["a_pred"], G["a_gt"], G["a_mask"]
    only = {k: depth_evaluation(p, g, custom_mask=m, **kw) for k, kw in MODES.items()}
    assert len({only[k][1] for k in only}) == 4                                  # the four modes give four different (s, t)
    every = dict(metric_scale=True, align_with_lstsq=True, align_with_scale=True)
    assert depth_evaluation(p, g, custom_mask=m, **every) == only["metric"]
    assert depth_evaluation(p, g, custom_mask=m, align_with_lstsq=True, align_with_scale=True) == only["lstsq"]
    assert depth_evaluation(p, g, custom_mask=m, align_with_scale=True) == only["scale"]
    assert depth_evaluation(p, g, custom_mask=m) == only["median"]


@pytest.mark.parametrize("flag", ["align_with_lad", "align_with_lad2", "disp_input"])
def test_unreproducible_modes_still_raise(flag):
    with pytest.raises(NotImplementedError):
        depth_evaluation(G["a_pred"], G["a_gt"], **{flag: True})
    with pytest.raises(NotImplementedError):
        depth_evaluation(G["a_pred"], G["a_gt"], align_with_lstsq=True, **{flag: True})


@pytest.mark.parametrize("mode", list(MODES))
def test_no_valid_pixel_returns_the_zeros_convention(mode):
    pred, gt = np.ones((1, 4, 4), np.float32), np.zeros((1, 4, 4), np.float32)
    res, st, emap = depth_evaluation(pred, gt, custom_mask=np.ones((1, 4, 4), bool), return_error_map=True, **MODES[mode], **CLIPS)
    assert all(res[k] == 0 for k in KEYS[:8]) and res["valid_pixels"] == 0
    assert st == ((1.0, 0.0) if mode == "metric" else (0.0, 0.0))
    assert not emap.any()


class _HalfGTModel:
    """pred = 0.5 * gt: a pure scale ambiguity."""
    calls = 0

    def forward(self, data):
        type(self).calls += 1
        d = np.stack([-np.asarray(c)[2] for c in data["cam_coord"]], 0)          # OpenGL z -> OpenCV depth
        return {"pred_depths": torch.from_numpy(0.5 * d).float()}


def _cfg(**eval_depth):
    return {"dataset": "SyntheticGeometryDataset", "root": "unused", "h": 32, "w": 48, "clip_length": 5, "clip_overlap": 1,
            "eval_depth": {"metric_names": ["Abs Rel", "delta < 1.25"], **eval_depth}}


@pytest.mark.parametrize("alignment,abs_rel", [("median", 0.0), ("scale", 0.0), ("lstsq", 0.0), ("metric", 0.5), (None, 0.0)])
def test_evaluate_honours_depth_alignment(tmp_path, alignment, abs_rel):
    ds = SyntheticGeometryDataset(clip_length=5, clip_overlap=1, input_size=(32, 48), target_size=(32, 48), root="unused", num_frames=9)
    cfg = _cfg() if alignment is None else _cfg(depth_alignment=alignment)
    rows, _ = evaluate(cfg, dataset=ds, model=_HalfGTModel(), save_dir=str(tmp_path), verbose=False)
    assert len(rows) == len(ds) == 3
    for r in rows:
        assert r["Abs Rel"] == pytest.approx(abs_rel, abs=2e-6) and r["delta < 1.25"] == (1.0 if abs_rel == 0 else 0.0)


def test_evaluate_applies_the_clip_keys_and_max_depth(tmp_path):
    ds = SyntheticGeometryDataset(clip_length=5, clip_overlap=1, input_size=(32, 48), target_size=(32, 48), root="unused", num_frames=5)
    plain, _ = evaluate(_cfg(depth_alignment="metric"), dataset=ds, model=_HalfGTModel(), save_dir=str(tmp_path), verbose=False)
    floor, _ = evaluate(_cfg(depth_alignment="metric", post_clip_min=1e3, post_clip_max=1e3), dataset=ds, model=_HalfGTModel(),
                        save_dir=str(tmp_path), verbose=False)
    assert plain[0]["Abs Rel"] == pytest.approx(0.5, abs=1e-6) and floor[0]["Abs Rel"] > 10       # every prediction clamped to 1000
    none, _ = evaluate(_cfg(depth_alignment="metric", max_depth=1e-3), dataset=ds, model=_HalfGTModel(), save_dir=str(tmp_path), verbose=False)
    assert none[0]["Abs Rel"] == 0 and none[0]["valid_pixels"] == 0                                  # max_depth below every gt: no valid pixel


def test_evaluate_rejects_an_unknown_alignment_before_the_first_clip(tmp_path):
    ds = SyntheticGeometryDataset(clip_length=5, clip_overlap=1, input_size=(32, 48), target_size=(32, 48), root="unused", num_frames=5)
    before = _HalfGTModel.calls
    with pytest.raises(ValueError, match="depth_alignment"):
        evaluate(_cfg(depth_alignment="lad"), dataset=ds, model=_HalfGTModel(), save_dir=str(tmp_path / "x"), verbose=False)
    assert _HalfGTModel.calls == before and not (tmp_path / "x").exists()
