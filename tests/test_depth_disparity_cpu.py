"""CPU: depth evaluation in disparity space on the host (harness.metrics.depth_evaluation(align_space="disparity"))
against tests/golden/depth_disparity_golden.npz - the reference's own ``disp_input=True`` outputs with the function it never defines
supplied, written by tests/golden/make_depth_disparity_golden.py - on hand-sized cases with the answers written out, and through the
harness loop (``eval_depth.space: disparity``)."""
import math
import os
import re

import numpy as np
import pytest
import torch

from unigeo_amd.harness import SyntheticGeometryDataset, depth_evaluation, depth_evaluation_in_global_coord, evaluate
from unigeo_amd.harness.eval import parse_depth_space_config
from unigeo_amd.harness.metrics import _lstsq_f32, disparity_to_depth, l1_fit, l1_objective

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "depth_disparity_golden.npz"), allow_pickle=False)
KEYS = [str(k) for k in G["keys"]]
MODES = {"metric": {"metric_scale": True}, "median": {}, "scale": {"align_with_scale": True}, "lstsq": {"align_with_lstsq": True}}
CLIPS = dict(zip(("pre_clip_min", "pre_clip_max", "post_clip_min", "post_clip_max"), (float(c) for c in G["clips"])))
CASES = [(tag, mode, clip) for tag in ("a", "q", "e") for mode in MODES for clip in ("noclip", "clip")]
f32 = np.float32


def _run(tag, mode, clip, **kw):
    return depth_evaluation(G[f"{tag}_pred"], G[f"{tag}_gt"], custom_mask=G[f"{tag}_mask"], align_space="disparity", **MODES[mode],
                            **(CLIPS if clip == "clip" else {}), **kw)


def test_fixture_holds_what_the_tests_assume():
    assert tuple(G["clips"]) == (f32(0.3), 1.0, f32(0.8), 5.0) and G["a_pred"].shape == (3, 20, 28)
    valid = lambda t: int(((G[f"{t}_gt"] > 0) & (G[f"{t}_gt"] < 80)).sum())
    assert valid("a") % 2 == 1 and valid("e") % 2 == 0 and valid("a") < 1680       # odd / even counts, invalid pixels present
    assert (G["a_gt"] == 90).sum() == 1 and (G["a_pred"] < 0).sum() > 30 and not G["a_mask"].all()
    assert np.isfinite(G["a_pred"]).all() and set(np.unique(G["q_pred"]).tolist()) <= {k / 8 for k in range(2, 9)}
    assert 0 < float(G["scale_distance"]) < 0.1
    # the generator's guard: no stored case inverts an aligned disparity nearer to 0 than 0.1
    assert float(G["min_abs_aligned_disparity"]) >= 0.1 and float(G["min_abs_aligned_disparity_map"]) >= 0.1


@pytest.mark.parametrize("tag,mode,clip", [c for c in CASES if c[1] != "scale"])
def test_host_modes_match_the_reference(tag, mode, clip):
    """metric / median / lstsq: every metric within the project's G5 bound (rel 2e-5, abs 1e-6) of the reference's own result.  Error map:
    rtol 1e-5, with the absolute term 1e-6 under lstsq only (as tests/test_depth_alignment_cpu.py).  s equal as float32 where the mode has
    no shift."""
    res, (s, t), emap = _run(tag, mode, clip, return_error_map=True)
    want = G[f"{tag}_{mode}_{clip}_vals"]
    worst = max(abs(res[k] - w) / max(abs(w), 1e-12) for k, w in zip(KEYS[:8], want))
    print(f"{tag}_{mode}_{clip}: largest relative distance of a metric to the reference {worst:.3e}")
    for k, w in zip(KEYS[:8], want):
        assert res[k] == pytest.approx(w, rel=2e-5, abs=1e-6), k
    assert res["valid_pixels"] == int(want[8])
    assert emap.shape == G[f"{tag}_gt"].shape and emap.dtype == np.float32
    np.testing.assert_allclose(emap, G[f"{tag}_{mode}_{clip}_emap"], rtol=1e-5, atol=1e-6 if mode == "lstsq" else 0)
    if mode != "lstsq":
        assert f32(s) == G[f"{tag}_{mode}_{clip}_s"] and t == 0.0       # equal as float32
    if mode == "metric":
        assert (s, t) == (1.0, 0.0)


@pytest.mark.parametrize("tag,clip", [(t, c) for t in ("a", "q", "e") for c in ("noclip", "clip")])
def test_host_scale_mode_within_twice_the_measured_distance(tag, clip):
    """``scale`` is ill-conditioned: the bound is twice the distance the generator measured and stored."""
    bound = 2.0 * float(G["scale_distance"])
    res, (s, t), emap = _run(tag, "scale", clip, return_error_map=True)
    want = G[f"{tag}_scale_{clip}_vals"]
    for k, w in zip(KEYS[:8], want):
        assert res[k] == pytest.approx(w, rel=bound, abs=1e-6), k
    assert res["valid_pixels"] == int(want[8]) and t == 0.0
    assert s == pytest.approx(float(G[f"{tag}_scale_{clip}_s"]), rel=bound)
    # the map is the stated formula at the returned s, in the stated float32 operations
    p, g = G[f"{tag}_pred"], G[f"{tag}_gt"]
    m1 = (g > 0) & (g < 80)
    ref = np.zeros_like(g)
    ref[m1] = np.abs(disparity_to_depth(p[m1] * f32(s)) - g[m1]) / g[m1]
    np.testing.assert_array_equal(emap, ref)


def _masked(tag, clip):
    p, g = G[f"{tag}_pred"], G[f"{tag}_gt"]
    m1 = (g > 0) & (g < 80)
    p = p[m1]
    if clip:
        p = np.minimum(np.maximum(p, f32(CLIPS["pre_clip_min"])), f32(CLIPS["pre_clip_max"]))
    return p, f32(1) / (g[m1] + f32(1e-8))


@pytest.mark.parametrize("tag,clip", [(t, c) for t in ("a", "q", "e") for c in (False, True)])
def test_l1_in_disparity_space_is_the_exact_fit_against_the_inverse_depth(tag, clip):
    """No reference: the returned (s, t) are ``l1_fit(p, gd)`` rounded once, and its objective is not above that of the lstsq and median
    fits on the same input."""
    kw = CLIPS if clip else {}
    res, (s, t) = depth_evaluation(G[f"{tag}_pred"], G[f"{tag}_gt"], custom_mask=G[f"{tag}_mask"], align_space="disparity", align_with_l1=True, **kw)
    p, gd = _masked(tag, clip)
    s64, t64, info = l1_fit(p, gd)
    assert info["certified"] == 1 and (s, t) == (float(f32(s64)), float(f32(t64)))
    F = l1_objective(p, gd, s64, t64)
    for other in ({"align_with_lstsq": True}, {}):
        so, to = depth_evaluation(G[f"{tag}_pred"], G[f"{tag}_gt"], align_space="disparity", **other, **kw)[1]
        assert F <= l1_objective(p, gd, so, to)
    assert res["valid_pixels"] == int(G[f"{tag}_median_noclip_vals"][8])


# ------------------------------------------------------------------------------------------------- hand-sized cases, answers written out
def test_a_non_positive_aligned_disparity_is_depth_zero_and_the_floor_turns_it_far():
    gt = np.array([2.0, 4.0, 1.0, 0.0], f32)                  # the last pixel is invalid
    pred = np.array([0.5, -0.25, 0.0, 9.0], f32)              # metric: a = pred
    res, (s, t), emap = depth_evaluation(pred, gt, metric_scale=True, align_space="disparity", return_error_map=True)
    assert (s, t) == (1.0, 0.0) and res["valid_pixels"] == 3
    # d = (2, 0, 0): |d - gt| / gt = (0, 1, 1)
    np.testing.assert_array_equal(emap, np.array([0.0, 1.0, 1.0, 0.0], f32))
    assert res["Abs Rel"] == pytest.approx(2 / 3, rel=1e-6) and res["RMSE"] == pytest.approx(math.sqrt((0 + 16 + 1) / 3), rel=1e-6)
    # floor 0.125: a = (0.5, 0.125, 0.125) -> d = (2, 8, 8); post-clip max 5 -> (2, 5, 5) for the metrics, the map keeps (2, 8, 8)
    res, _, emap = depth_evaluation(pred, gt, metric_scale=True, align_space="disparity", disp_clip_min=0.125, post_clip_max=5.0,
                                    return_error_map=True)
    np.testing.assert_array_equal(emap, np.array([0.0, 1.0, 7.0, 0.0], f32))
    assert res["Abs Rel"] == pytest.approx((0 + 1 / 4 + 4) / 3, rel=1e-6) and res["RMSE"] == pytest.approx(math.sqrt((0 + 1 + 16) / 3), rel=1e-6)
    # a NaN aligned disparity gives depth 0, with and without the floor
    nan = np.array([np.nan, 0.5], f32)
    np.testing.assert_array_equal(disparity_to_depth(nan), np.array([0.0, 2.0], f32))
    np.testing.assert_array_equal(disparity_to_depth(nan, 1.0), np.array([0.0, 1.0], f32))


def test_the_pre_clip_feeds_the_fit_and_the_map_uses_the_original_prediction():
    gt = np.array([1.0, 2.0, 4.0], f32)                       # gd = (1, 0.5, 0.25) up to the 1e-8
    pred = np.array([4.0, 1.0, 0.5], f32)
    # median without clips: s = 0.5 / 1.0
    _, (s, t) = depth_evaluation(pred, gt, align_space="disparity")
    assert (s, t) == (0.5, 0.0)
    # pre-clip max 2: p = (2, 1, 0.5), same medians, s = 0.5: a = (1, 0.5, 0.25), d = gt exactly up to the 1e-8 -> metrics ~ 0 ...
    res, (s, t), emap = depth_evaluation(pred, gt, align_space="disparity", pre_clip_max=2.0, return_error_map=True)
    assert (s, t) == (0.5, 0.0) and res["Abs Rel"] == pytest.approx(0.0, abs=1e-7)
    # ... while the map sees the original 4.0: a0 = 2, d0 = 0.5, |0.5 - 1| / 1
    np.testing.assert_allclose(emap, np.array([0.5, 0.0, 0.0], f32), atol=1e-7)
    # pre-clip min 2: every p = 2 for the fit (s = 0.5 / 2), the metrics see a = 0.5 -> d = 2 everywhere, the map the original prediction
    res, (s, t), emap = depth_evaluation(pred, gt, align_space="disparity", pre_clip_min=2.0, pre_clip_max=2.0, return_error_map=True)
    assert (s, t) == (0.25, 0.0) and res["Abs Rel"] == pytest.approx((1 + 0 + 0.5) / 3, rel=1e-6)
    np.testing.assert_allclose(emap, np.array([0.0, 1.0, 1.0], f32), atol=1e-7)       # d0 = (1, 4, 8)


def test_max_depth_none_keeps_every_positive_ground_truth():
    gt = np.array([1.0, 2.0, 100.0, 0.0], f32)
    pred = np.array([1.0, 0.5, 0.01, 1.0], f32)
    res, (s, t) = depth_evaluation(pred, gt, metric_scale=True, align_space="disparity")
    assert res["valid_pixels"] == 2 and res["Abs Rel"] == pytest.approx(0.0, abs=1e-7)
    res, (s, t), emap = depth_evaluation(pred, gt, metric_scale=True, align_space="disparity", max_depth=None, return_error_map=True)
    assert res["valid_pixels"] == 3 and res["Abs Rel"] == pytest.approx(0.0, abs=1e-6) and emap[3] == 0.0
    # the median over three valid pixels: gd = (1, 0.5, 0.01) -> 0.5, p -> 0.5
    assert depth_evaluation(pred, gt, align_space="disparity", max_depth=None)[1] == (1.0, 0.0)


@pytest.mark.parametrize("mode", ["metric", "median", "scale", "lstsq", "l1"])
def test_no_valid_pixel_returns_the_zeros_convention(mode):
    kw = {"l1": {"align_with_l1": True}, **MODES}[mode]
    gt = np.zeros((2, 3), f32)
    pred = np.full((2, 3), 0.5, f32)
    res, (s, t), emap = depth_evaluation(pred, gt, align_space="disparity", return_error_map=True, **kw)
    assert all(res[k] == 0 for k in KEYS[:8]) and res["valid_pixels"] == 0
    assert (s, t) == ((1.0, 0.0) if mode == "metric" else (0.0, 0.0))
    assert emap.shape == gt.shape and not emap.any()


def test_flags():
    p, g, m = G["a_pred"], G["a_gt"], G["a_mask"]
    with pytest.raises(NotImplementedError):
        depth_evaluation(p, g, disp_input=True)
    with pytest.raises(NotImplementedError):
        depth_evaluation(p, g, disp_input=True, align_space="disparity")
    with pytest.raises(NotImplementedError):
        depth_evaluation_in_global_coord(p, g, g, np.tile(np.eye(4, dtype=f32), (3, 1, 1)), np.tile(np.eye(3, dtype=f32), (3, 1, 1)),
                                         align_with_lstsq=True, disp_input=True)
    with pytest.raises(TypeError):        # the world-frame evaluation does not take the option
        depth_evaluation_in_global_coord(p, g, g, np.tile(np.eye(4, dtype=f32), (3, 1, 1)), np.tile(np.eye(3, dtype=f32), (3, 1, 1)),
                                         align_with_lstsq=True, align_space="disparity")
    for bad in ("disp", "Depth", None, 1):
        with pytest.raises(ValueError, match="alignment space"):
            depth_evaluation(p, g, align_space=bad)
    for bad in (0, 0.0, -1e-3, float("inf"), float("nan"), "x", True):
        with pytest.raises(ValueError, match="disp_clip_min"):
            depth_evaluation(p, g, align_space="disparity", disp_clip_min=bad)
    with pytest.raises(ValueError, match="disp_clip_min"):
        depth_evaluation(p, g, disp_clip_min=1e-3)                       # a floor in depth space
    with pytest.raises(ValueError, match="disp_clip_min"):
        depth_evaluation(p, g, align_space="depth", disp_clip_min=1e-3)
    # the default is today's call: same values, same map bytes
    for kw in ({"align_with_lstsq": True}, {}, {"align_with_l1": True, **CLIPS}):
        a = depth_evaluation(p, g, custom_mask=m, return_error_map=True, **kw)
        b = depth_evaluation(p, g, custom_mask=m, return_error_map=True, align_space="depth", disp_clip_min=None, **kw)
        assert a[:2] == b[:2] and a[2].tobytes() == b[2].tobytes()
    # the precedence of the flags is unchanged in disparity space
    ls = depth_evaluation(p, g, align_space="disparity", align_with_lstsq=True)
    assert depth_evaluation(p, g, align_space="disparity", align_with_lstsq=True, align_with_l1=True, align_with_scale=True) == ls
    assert depth_evaluation(p, g, align_space="disparity", metric_scale=True, align_with_lstsq=True)[1] == (1.0, 0.0)
    # and the space matters
    assert depth_evaluation(p, g, align_space="disparity", align_with_lstsq=True)[0] != depth_evaluation(p, g, align_with_lstsq=True)[0]


def test_lstsq_in_double_rounds_to_the_float32_solve_or_its_neighbour():
    """What the device solves: the same system in float64, rounded once (tests/test_depth_disparity_gpu.py bounds the two at 2 ulps)."""
    for tag in ("a", "q", "e"):
        p, gd = _masked(tag, False)
        s32, t32 = _lstsq_f32(p, gd)
        s64, t64 = _lstsq_f32(p, gd, np.float64)
        assert abs(float(s32) - float(s64)) <= 4 * np.spacing(abs(s64)) and abs(float(t32) - float(t64)) <= 4 * np.spacing(abs(t64))


# ------------------------------------------------------------------------------------------------- harness
def test_parse_accepts_the_two_keys_and_rejects_bad_values():
    assert parse_depth_space_config({}) == ("depth", None)
    assert parse_depth_space_config({"eval_depth": {"metric_names": []}}) == ("depth", None)
    assert parse_depth_space_config({"eval_depth": {"space": "disparity"}}) == ("disparity", None)
    assert parse_depth_space_config({"eval_depth": {"space": "disparity", "disp_clip_min": 1e-3}}) == ("disparity", 1e-3)
    assert parse_depth_space_config({"eval_depth": {"space": "disparity", "coord": "camera", "depth_alignment": "l1"}}) == ("disparity", None)
    with pytest.raises(ValueError, match="space"):
        parse_depth_space_config({"eval_depth": {"space": "disp"}})
    for bad in (0, -1.0, float("inf"), float("nan"), "small"):
        with pytest.raises(ValueError, match="disp_clip_min"):
            parse_depth_space_config({"eval_depth": {"space": "disparity", "disp_clip_min": bad}})
    with pytest.raises(ValueError, match="disp_clip_min"):
        parse_depth_space_config({"eval_depth": {"disp_clip_min": 1e-3}})
    with pytest.raises(ValueError, match="global"):
        parse_depth_space_config({"eval_depth": {"space": "disparity", "coord": "global"}})


class _Stub:
    """depth = gt * 1.1 + 0.2 and, when asked, the normalised disparity of a model that sees 1 / gt up to an affine map."""

    def __init__(self, disparity):
        self.disparity, self.calls = disparity, 0

    def forward(self, data):
        self.calls += 1
        d = np.stack([-np.asarray(c)[2] for c in data["cam_coord"]], 0).astype(np.float32)          # OpenGL z -> OpenCV depth
        out = {"pred_depths": torch.from_numpy(d * f32(1.1) + f32(0.2))}
        if self.disparity:
            x = 1.0 / np.maximum(d, f32(0.05))
            out["pred_disps"] = torch.from_numpy(((x - x.min()) / (x.max() - x.min())).astype(np.float32))
        return out


def _cfg(**eval_depth):
    return {"dataset": "SyntheticGeometryDataset", "root": "unused", "h": 32, "w": 48, "clip_length": 3,
            "eval_depth": {"metric_names": ["Abs Rel", "RMSE", "delta < 1.25"], **eval_depth}}


def _ds():
    return SyntheticGeometryDataset(clip_length=3, clip_overlap=0, input_size=(32, 48), target_size=(32, 48), root="unused", num_frames=6)


def test_evaluate_scores_pred_disps_in_disparity_space(tmp_path):
    from unigeo_amd.harness.io_utils import prepare_gt_label
    ds = _ds()
    rows_d, _ = evaluate(_cfg(space="disparity"), dataset=ds, model=_Stub(True), save_dir=str(tmp_path / "disp"), verbose=False)
    rows_z, _ = evaluate(_cfg(space="depth"), dataset=ds, model=_Stub(True), save_dir=str(tmp_path / "depth"), verbose=False)
    assert len(rows_d) == len(rows_z) == len(ds) == 2
    stub = _Stub(True)
    for i, (rd, rz) in enumerate(zip(rows_d, rows_z)):
        assert rd["seq_name"] == rz["seq_name"] and rd["Abs Rel"] != rz["Abs Rel"]
        data = ds[i]
        gt = prepare_gt_label(data)
        want = depth_evaluation(stub.forward(data)["pred_disps"], gt["gt_depths"], custom_mask=gt["gt_masks"], align_space="disparity",
                                align_with_lstsq=True)[0]
        assert rd["Abs Rel"] == want["Abs Rel"] and rd["RMSE"] == want["RMSE"]          # the row is the host function's
        assert rd["Abs Rel"] < 1e-3                                                     # the stub's disparity is affine in 1 / gt
    # the floor reaches the host function
    rows_f, _ = evaluate(_cfg(space="disparity", disp_clip_min=0.5, post_clip_max=80.0), dataset=ds, model=_Stub(True),
                         save_dir=str(tmp_path / "floor"), verbose=False)
    assert rows_f[0]["Abs Rel"] != rows_d[0]["Abs Rel"]


def test_a_model_without_pred_disps_is_a_named_error(tmp_path):
    model = _Stub(False)
    with pytest.raises(ValueError) as e:
        evaluate(_cfg(space="disparity"), dataset=_ds(), model=model, save_dir=str(tmp_path), verbose=False)
    msg = str(e.value)
    assert "000_" in msg and "_Stub" in msg and "return_disparity" in msg and "pred_disps" in msg
    assert model.calls == 1                                                             # at its first clip


def test_bad_keys_raise_before_the_first_clip(tmp_path):
    for bad in ({"space": "inverse"}, {"space": "disparity", "disp_clip_min": -1}, {"disp_clip_min": 1e-3},
                {"space": "disparity", "coord": "global"}):
        model = _Stub(True)
        with pytest.raises(ValueError):
            evaluate(_cfg(**bad), dataset=_ds(), model=model, save_dir=str(tmp_path), verbose=False)
        assert model.calls == 0


def test_a_configuration_without_the_keys_writes_the_same_csv(tmp_path, monkeypatch):
    """Two runs of one configuration without the new keys, the second with the disparity path made unreachable: same rows, same CSV bytes,
    and the rows are those of the plain depth call."""
    from unigeo_amd.harness import eval as ev
    from unigeo_amd.harness import metrics
    ds = _ds()
    rows_a, _ = evaluate(_cfg(depth_alignment="median"), dataset=ds, model=_Stub(True), save_dir=str(tmp_path / "a"), verbose=False)

    def never(*a, **k):
        raise AssertionError("the disparity path was entered")
    monkeypatch.setattr(metrics, "disparity_to_depth", never)
    seen = []
    real = ev.depth_evaluation

    def spy(*a, **k):
        seen.append(k)
        return real(*a, **k)
    monkeypatch.setattr(ev, "depth_evaluation", spy)
    rows_b, _ = evaluate(_cfg(depth_alignment="median"), dataset=ds, model=_Stub(True), save_dir=str(tmp_path / "b"), verbose=False)
    assert rows_a == rows_b and len(seen) == 2
    assert all("align_space" not in k and "disp_clip_min" not in k for k in seen)       # the call the loop made before this option existed
    a, b = (tmp_path / "a" / "metrics.csv").read_bytes(), (tmp_path / "b" / "metrics.csv").read_bytes()
    assert a == b and a.count(b"\n") == 4


def test_the_plugin_option_is_off_by_default_and_adds_one_key():
    """``return_disparity`` with a recording pipeline: the default makes the pipeline call it always made and returns no ``pred_disps``."""
    from types import SimpleNamespace
    from unigeo_amd.model.depthcrafter import DepthCrafter

    class Rec:
        def __init__(self):
            self.calls = []

        def __call__(self, frames, **kw):
            self.calls.append(kw)
            T, H, W = frames.shape[0], frames.shape[2], frames.shape[3]
            return SimpleNamespace(frames=[None], depth=np.ones((T, H, W), f32), normals=np.zeros((T, H, W, 3), f32),
                                   disparity=np.full((T, H, W), 0.25, f32) if kw.get("return_disparity") else None)
    data = {"images": [np.zeros((3, 64, 64), f32)] * 2, "intrinsics": [np.eye(3, dtype=f32)] * 2, "_index": 0}
    p = DepthCrafter.__new__(DepthCrafter)
    p.pipeline, p.num_inference_steps, p.seed, p._calls, p.device, p.noise = Rec(), 2, 0, 0, "cpu", "device"
    out = p.forward(data)
    assert set(out) == {"pred_depths", "pred_normals"} and "return_disparity" not in p.pipeline.calls[-1]
    p.return_disparity = True
    out = p.forward(data)
    first, last = p.pipeline.calls
    assert last["return_disparity"] is True and set(last) == set(first) | {"return_disparity"}
    assert all(np.array_equal(last[k], first[k]) for k in first)
    assert out["pred_disps"].dtype == torch.float32 and tuple(out["pred_disps"].shape) == (2, 64, 64) and float(out["pred_disps"][0, 0, 0]) == 0.25


# ------------------------------------------------------------------------------------------------- exports
def test_the_new_symbols_are_declared_and_bound():
    from unigeo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "unigeo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym in ("ug_depth_eval_opts2_default", "ug_eval_depth_ex2", "ug_dc_get_disparity"):
        assert re.search(rf"\b{sym}\s*\(", code), sym
        assert sym in _lib.EXPORTS
    assert re.search(r"#define\s+UG_DEPTH_ALIGN_DISPARITY\s+1\b", code) and _lib.DEPTH_ALIGN_DISPARITY == 1
    assert "disp_input (calls a" not in hdr and "ug_eval_depth_ex2 below" in hdr          # the sentence that said it has no counterpart is gone
    # the ctypes mirror: the old struct first and unchanged, then flags and the floor
    import ctypes as C
    assert [f[0] for f in _lib.DepthEvalOpts2C._fields_] == ["base", "flags", "disp_clip_min"]
    assert C.sizeof(_lib.DepthEvalOptsC) == 24 and C.sizeof(_lib.DepthEvalOpts2C) == 32 and _lib.DepthEvalOpts2C.flags.offset == 24
