"""GPU: the temporal alignment error on the device (ug_eval_tae, kernels/temporal.hip) against the numpy mirror
(unigeo_amd/harness/temporal.py) with the same (s, t): warped maps and error maps byte for byte, counts equal, values to rel 1e-10.

The value bound is derived, not measured: a pair's value is a float64 sum of at most 2^19 non-negative float32 terms taken in two different
orders, which differ by at most (n - 1) * 2^-53 < 6e-11 relative; the division by the same count adds one rounding on each side."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from tae_fixtures import (LARGE_CASE, SMALL_CASES, assert_scene_conditions, bad_pixel_scene, check_flicker, check_plane_shift, contest_case,      # noqa: E402
                          disparity_scene, facing_apart_scene, flicker_case, make_scene, plane_shift_case, same_bytes, source_hits)

pytestmark = pytest.mark.gpu

F32 = np.float32
REL = 1e-10


def _mirror(sc, pred=None, **kw):
    from unigeo_amd.harness import temporal_alignment_error
    return temporal_alignment_error(sc["pred"] if pred is None else pred, sc["gt"], sc["poses"], sc["K"], sc["fit"], custom_mask=sc.get("mask"),
                                    return_maps=True, **kw)


def _device(engine, sc, pred=False, **kw):
    return engine.eval_tae(sc["gt"], sc["poses"], sc["K"], sc["fit"], sc.get("mask"), pred=sc["pred"] if pred is False else pred,
                           return_maps=True, **kw)


def _same(dev, ref):
    assert same_bytes(dev["warp"], ref["warp"]) and same_bytes(dev["err"], ref["err"])
    assert (dev["pair_values"][:, 1] == ref["pair_values"][:, 1]).all()
    print("pair values: device", dev["pair_values"][:, 0].tolist(), "mirror", ref["pair_values"][:, 0].tolist())
    np.testing.assert_allclose(dev["pair_values"][:, 0], ref["pair_values"][:, 0], rtol=REL, atol=0, equal_nan=True)
    for k in ("TAE pairs", "TAE pairs total", "TAE pixels"):
        assert dev[k] == ref[k], k
    assert dev["TAE"] == pytest.approx(ref["TAE"], rel=REL, nan_ok=True)


def _conditions(sc, ref, stride=1, **kw):
    from unigeo_amd.harness import aligned_depth
    H, W = sc["gt"].shape[1:]
    d = aligned_depth(sc["pred"], sc["fit"], kw.get("space", "depth"), kw.get("disp_clip_min"), kw.get("post_clip_min"), kw.get("post_clip_max"))
    assert_scene_conditions(ref["pair_values"], source_hits(d, sc["poses"], sc["K"], stride), H, W)


@pytest.mark.parametrize("T,H,W,stride,seed", SMALL_CASES + [LARGE_CASE])
def test_device_equals_the_mirror(engine, T, H, W, stride, seed):
    sc = make_scene(T, H, W, seed)
    ref = _mirror(sc, stride=stride)
    _conditions(sc, ref, stride)
    dev = _device(engine, sc, stride=stride)
    _same(dev, ref)
    assert dev["TAE pairs"] == 2 * (T - stride)
    plain = engine.eval_tae(sc["gt"], sc["poses"], sc["K"], sc["fit"], sc["mask"], pred=sc["pred"], stride=stride)      # no maps asked for
    assert plain == {k: dev[k] for k in plain}


def test_two_calls_give_the_same_bytes(engine):
    T, H, W, stride, seed = LARGE_CASE
    sc = make_scene(T, H, W, seed)
    a, b = _device(engine, sc), _device(engine, sc)
    assert a["TAE"] == b["TAE"] and same_bytes(a["pair_values"], b["pair_values"])
    assert same_bytes(a["warp"], b["warp"]) and same_bytes(a["err"], b["err"])


def test_closed_forms_on_the_device(engine):
    sc, want = flicker_case()
    check_flicker(_device(engine, sc), want)
    check_plane_shift(_device(engine, plane_shift_case()))


def test_edge_cases_on_the_device(engine):
    sc = make_scene(*SMALL_CASES[0][:3], SMALL_CASES[0][4])
    res = _device(engine, sc, stride=3)      # T == stride: a result, not an error
    assert math.isnan(res["TAE"]) and res["TAE pairs"] == res["TAE pairs total"] == res["TAE pixels"] == 0
    apart = facing_apart_scene()
    dev = _device(engine, apart)
    _same(dev, _mirror(apart))
    assert dev["TAE pairs"] == 2 and dev["TAE pairs total"] == 4
    bad = bad_pixel_scene()
    dev = _device(engine, bad)
    _same(dev, _mirror(bad))
    assert dev["TAE pairs"] == 4 and math.isfinite(dev["TAE"])
    d, K = contest_case()
    sc = {"pred": d, "gt": d, "poses": np.tile(np.eye(4, dtype=F32), (2, 1, 1)), "K": K, "fit": (1.0, 0.0)}
    dev = _device(engine, sc)
    _same(dev, _mirror(sc))
    assert dev["warp"][0, 0, 0] == d[0, :2, :2].min() and dev["warp"][0, 1, 2] == d[0, 2, 3:6].min()


@pytest.mark.parametrize("kw", [{"space": "disparity"}, {"space": "disparity", "disp_clip_min": 0.3},
                                {"space": "disparity", "disp_clip_min": 0.3, "post_clip_min": 2.0, "post_clip_max": 3.0},
                                {"post_clip_min": 2.0, "post_clip_max": 3.2}, {"post_clip_max": 3.0, "max_depth": 3.1}, {"max_depth": None}])
def test_disparity_flag_floor_and_post_clips(engine, kw):
    sc = disparity_scene() if kw.get("space") == "disparity" else make_scene(*SMALL_CASES[1][:3], SMALL_CASES[1][4])
    ref = _mirror(sc, **kw)
    _same(_device(engine, sc, **kw), ref)
    assert ref["TAE pairs"] == 6


def _raw(engine, sc, fields=None, guard=0, **over):
    """ug_eval_tae called directly; ``fields`` sets option fields, ``over`` replaces single arguments (None: a NULL pointer)"""
    from unigeo_amd._lib import TaeOptsC, _ptr
    from unigeo_amd.harness import relative_poses
    T, H, W = sc["gt"].shape
    o = TaeOptsC()
    engine.lib.ug_tae_opts_default(C.byref(o))
    for k, v in (fields or {}).items():
        setattr(o, k, v)
    stride = max(int(o.stride), 1)
    rel = np.ascontiguousarray(relative_poses(sc["poses"], stride))
    P = rel.shape[0]
    a = {"pred": np.ascontiguousarray(sc["pred"], F32), "gt": np.ascontiguousarray(sc["gt"], F32), "mask": None, "K": np.ascontiguousarray(sc["K"], F32),
         "rel": rel if P else np.zeros((1, 3, 4)), "T": T, "H": H, "W": W, "opts": o, "out4": np.full(4, -7.0), "pair": np.full((max(P, 1), 2), -7.0),
         "warp": np.full(P * H * W + guard, -777.0, F32), "err": np.full(P * H * W + guard, -777.0, F32)}
    a.update(over)
    p = lambda x: None if x is None else _ptr(x)      # noqa: E731
    rc = engine.lib.ug_eval_tae(engine.ctx, p(a["pred"]), p(a["gt"]), p(a["mask"]), p(a["K"]), p(a["rel"]), a["T"], a["H"], a["W"],
                                None if a["opts"] is None else C.byref(a["opts"]), p(a["out4"]), p(a["pair"]), p(a["warp"]), p(a["err"]))
    return rc, engine.lib.ug_last_error(engine.ctx).decode(), a


def test_defaults_and_guard_margins(engine):
    from unigeo_amd._lib import TaeOptsC
    o = TaeOptsC()
    engine.lib.ug_tae_opts_default(C.byref(o))
    assert (o.s, o.t, o.flags, o.max_depth, o.stride) == (1.0, 0.0, 0, 80.0, 1)
    assert all(math.isnan(v) for v in (o.disp_clip_min, o.post_clip_min, o.post_clip_max))
    T, H, W, stride, seed = SMALL_CASES[1]
    sc = make_scene(T, H, W, seed)
    rc, msg, a = _raw(engine, sc, {"s": float(sc["fit"][0]), "t": float(sc["fit"][1])}, guard=4096)
    assert rc == 0, msg
    n = 2 * (T - 1) * H * W
    ref = _mirror({**sc, "mask": None})
    assert (a["warp"][n:] == F32(-777.0)).all() and (a["err"][n:] == F32(-777.0)).all()      # nothing past the end was written
    assert same_bytes(a["warp"][:n].reshape(ref["warp"].shape), ref["warp"]) and same_bytes(a["err"][:n].reshape(ref["err"].shape), ref["err"])
    assert a["out4"][1:].tolist() == [ref["TAE pairs"], ref["TAE pairs total"], ref["TAE pixels"]]


ERRORS = [("options", {"opts": None}, None), ("gt_depth", {"gt": None}, None), ("intrinsics", {"K": None}, None), ("rel", {"rel": None}, None),
          ("out4", {"out4": None}, None), ("positive", {"T": 0}, None), ("positive", {"H": -1}, None), ("positive", {"W": 0}, None),
          ("stride", {}, {"stride": 0}), ("flag", {}, {"flags": 2}), ("disp_clip_min", {}, {"flags": 1, "disp_clip_min": 0.0}),
          ("disp_clip_min", {}, {"flags": 1, "disp_clip_min": -0.5}), ("disp_clip_min", {}, {"flags": 1, "disp_clip_min": float("inf")}),
          ("disp_clip_min", {}, {"flags": 0, "disp_clip_min": 0.01}), ("resident", {"pred": None}, None),
          ("2^31", {"H": 32768, "W": 16384}, None)]      # 4 pairs x 2^29 pixels; rejected before any pointer is read


def test_every_error_is_reported_and_the_context_stays_usable(engine):
    T, H, W, stride, seed = SMALL_CASES[0]
    sc = make_scene(T, H, W, seed)
    ref = _mirror(sc)
    for word, over, fields in ERRORS:
        rc, msg, _ = _raw(engine, sc, fields, **over)
        assert rc != 0 and word in msg, (word, over, fields, rc, msg)
        _same(_device(engine, sc), ref)      # a valid call afterwards succeeds
    with pytest.raises(ValueError):
        engine.eval_tae(sc["gt"], sc["poses"], sc["K"], sc["fit"], pred=sc["pred"], disp_clip_min=0.1)


def test_a_workspace_too_small_names_the_bytes_needed():
    from unigeo_amd._lib import Engine
    small = Engine(0, workspace_bytes=1 << 20, persist_bytes=1 << 20)
    try:
        big, tiny = make_scene(3, 128, 128, 0), make_scene(*SMALL_CASES[0][:3], SMALL_CASES[0][4])
        with pytest.raises(RuntimeError, match=r"needs \d+ bytes"):
            _device(small, big)
        _same(_device(small, tiny), _mirror(tiny))
    finally:
        small.close()


# ---------------------------------------------------------------------------------------------------------------- resident outputs, harness
@pytest.fixture(scope="module")
def tiny_plugin():
    from unigeo_amd import weights as W
    from unigeo_amd.model import DepthCrafter
    m = DepthCrafter(synthetic_weights=True, cfgs=W.tiny_cfgs(), num_inference_steps=2, workspace_bytes=3 << 30)
    yield m
    m.pipeline.engine.close()


def test_resident_depth_and_resident_disparity(tiny_plugin):
    from unigeo_amd.synthetic import synthetic_clip
    tiny_plugin.forward(synthetic_clip(3, 64, 64, seed=1))
    eng = tiny_plugin.pipeline.engine
    sc = make_scene(3, 64, 64, 0)
    _, depth, _ = eng.get_outputs(frames=False, depth=True)
    disp = eng.get_disparity()
    for space, pred in (("depth", depth), ("disparity", disp)):
        _, fit = eng.eval_depth(sc["gt"], sc["mask"], alignment="median", space=space)      # the device's own (s, t), s > 0
        one = {**sc, "pred": pred, "fit": (F32(fit[0]), F32(fit[1]))}
        ref = _mirror(one, space=space)
        _conditions(one, ref, space=space)
        dev = _device(eng, one, pred=None, space=space)
        _same(dev, ref)
        _same(_device(eng, one, space=space), ref)      # the same array passed explicitly
        print(space, "fit", fit, "scored fraction", (ref["pair_values"][:, 1] / (64 * 64)).tolist())
        assert ref["TAE pairs"] == 4 and (ref["pair_values"][:, 1] > 0).all()


class _Recording:
    """the plugin, remembering the depth of every clip it ran"""

    def __init__(self, plugin):
        self.plugin, self.pipeline, self.depths = plugin, plugin.pipeline, []

    def forward(self, data):
        out = self.plugin.forward(data)
        self.depths.append(out["pred_depths"].numpy().astype(F32))
        return out


def test_harness_device_metrics_fill_tae(tiny_plugin, tmp_path):
    from unigeo_amd.harness import SyntheticGeometryDataset, evaluate, prepare_gt_label, temporal_alignment_error
    cfg = {"root": "x", "h": 64, "w": 64, "clip_length": 3, "clip_overlap": 1, "eval_depth": {"metric_names": ["Abs Rel"], "depth_alignment": "median"},
           "eval_temporal": {"metric_names": ["TAE", "TAE gt"]}}
    ds = SyntheticGeometryDataset(clip_length=3, clip_overlap=1, input_size=(64, 64), num_frames=5)
    model = _Recording(tiny_plugin)
    rows, _ = evaluate(cfg, dataset=ds, model=model, save_dir=str(tmp_path), verbose=False, device_metrics=True)
    eng = tiny_plugin.pipeline.engine
    assert len(rows) == len(model.depths) == 3
    for i, r in enumerate(rows):
        gt = prepare_gt_label(ds[i])
        g, m, poses = gt["gt_depths"].numpy(), gt["gt_masks"].numpy(), gt["gt_poses"].numpy()
        K = np.stack([np.asarray(k, F32) for k in ds[i]["intrinsics"]], 0)
        _, fit = eng.eval_depth(g, m, pred=model.depths[i], alignment="median")      # the fit the device returns for these outputs
        want = temporal_alignment_error(model.depths[i], g, poses, K, (F32(fit[0]), F32(fit[1])), custom_mask=m)
        floor = temporal_alignment_error(g, g, poses, K, (1.0, 0.0), custom_mask=m)
        print("clip", i, "TAE device", r["TAE"], "mirror", want["TAE"], "TAE gt", r["TAE gt"], floor["TAE"])
        assert r["TAE"] == pytest.approx(want["TAE"], rel=REL) and r["TAE gt"] == pytest.approx(floor["TAE"], rel=REL)
        assert (r["TAE pairs"], r["TAE pairs total"], r["TAE pixels"]) == (want["TAE pairs"], 4, want["TAE pixels"])
    assert (tmp_path / "metrics.csv").read_text().splitlines()[0] == ",Abs Rel,TAE,TAE gt"
