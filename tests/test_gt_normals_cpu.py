"""CPU: normals fitted from depth (unigeo_amd/harness/normals.py) - ``fit_normals`` against the reference's
``get_surface_normal_np`` (tests/golden/gt_normals_golden.npz, written by tests/golden/make_gt_normals_golden.py), against the analytic planes
of the fixtures' scene and against a per-pixel restatement; the masking rules; ``normals="depth"`` of the five RGB-D loaders; and
``prepare_gt_label`` / ``evaluate`` with the fit's validity mask.  The kernel is compared with the mirror bit for bit in
tests/test_gt_normals_gpu.py."""
import os

import numpy as np
import pytest

import gt_normals_fixtures as fx
from unigeo_amd.harness import evaluate, prepare_gt_label
from unigeo_amd.harness import rgbd
from unigeo_amd.harness.eval import parse_dataset_config
from unigeo_amd.harness.metrics import normal_evaluation
from unigeo_amd.harness.normals import default_min_count, fit_normals, fit_normals_counts, world_normals
from unigeo_amd.harness.scannetpp import _resize

G = os.path.join(os.path.dirname(__file__), "golden")
LAYOUTS = sorted(fx.SCENE)
NORMAL_KEYS = ["normal mean", "normal median", "normal rmse", "angle < 5", "angle < 7.5", "angle < 11.25", "angle < 22.5", "angle < 30"]


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(G, "gt_normals_golden.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def scene():
    """The fixtures' scene at focal 40: points, mask, and the default fit with its count map; read-only."""
    c, mask = fx.backproject(fx.scene_raw()[0], fx.K40)
    n, nm, cnt = fit_normals_counts(c, mask)
    return {"c": c, "mask": mask, "n": n, "nm": nm > 0, "cnt": cnt}


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    """layout -> root of a temporary scene; written once."""
    base = tmp_path_factory.mktemp("gt_normals_scenes")
    out = {}
    for L in LAYOUTS:
        out[L] = str(base / L)
        fx.write_scene(out[L], L)
    return out


@pytest.fixture(scope="module")
def native_samples(roots):
    """layout -> the first clip at native size with normals="depth"; fitted once per layout, read-only."""
    cache = {}

    def get(L):
        if L not in cache:
            cache[L] = _dataset(roots, L, normals="depth")[0]
        return cache[L]
    return get


def _dataset(roots, L, **kw):
    return rgbd.LAYOUTS[L](roots[L], scenes=[fx.SCENE[L]], clip_length=fx.T, clip_overlap=0, **kw)


# ---------------------------------------------------------------------------------------------------------------- 1. the reference pin
def test_full_window_fit_matches_the_reference(gold):
    """edge=None and a full mask: on pixels at least ``radius`` from the border the fit is the reference's system.  The bound is twice the
    reference's own float32 noise, which the golden script measured against its float64 run."""
    I = (slice(2, fx.H - 2), slice(2, fx.W - 2))
    assert gold["points"].shape == (3, 3, fx.H, fx.W) and fx.H % 4 == 0 and fx.W % 4 == 0
    for k in range(3):
        n, nm = fit_normals(gold["points"][k], np.ones((fx.H, fx.W), bool), edge=None)
        assert n.dtype == np.float32 and nm.dtype == np.float32 and nm[I].min() == 1
        ang = fx.angle_deg(n.transpose(1, 2, 0)[I], gold["ref32"][k][I]).max()
        print(f"frame {k}: max angle to the reference {ang:.3e} deg, the reference's float32 noise {gold['noise_deg'][k]:.3e} deg")
        assert 0 < gold["noise_deg"][k] < 1e-2
        assert ang <= 2 * gold["noise_deg"][k]


# ---------------------------------------------------------------------------------------------------------------- 2. analytic planes
def test_valid_normals_lie_on_the_analytic_planes(gold, scene):
    """Per plane, away from the step: the distance from the true normal is at most what an unquantised float64 fit of the same windows is
    away (the fit's own bias: the regulariser, the window's shape) plus what the millimetre quantisation costs, measured once by the golden
    script - by the reference on full windows (``quant_deg``; asserted on the pixels whose window is full) and by an independent per-pixel
    solver on the scene's cut windows (``quant_scene_deg``; asserted on every valid pixel)."""
    d = fx.scene_depth()
    u, v = np.meshgrid(np.arange(fx.W), np.arange(fx.H))
    exact = np.stack([(u - fx.K40[0, 2]) * d / fx.K40[0, 0], -(v - fx.K40[1, 2]) * d / fx.K40[1, 1], -d], -1)      # float64, unquantised
    Nu, oku, _ = fx.loop_fit(exact, scene["mask"])
    nv = scene["n"].transpose(1, 2, 0)
    assert scene["nm"].mean() > 0.9
    for k, (cols, n_cv) in enumerate(((slice(0, fx.STEP - 2), fx.N_TILT), (slice(fx.STEP + 2, fx.W), fx.N_FRONT))):
        truth = fx.truth_gl(n_cv)
        ok = scene["nm"][:, cols]
        assert ok.sum() > 150 and np.array_equal(ok, oku[:, cols])
        err = fx.angle_deg(nv[:, cols], truth)
        bias = fx.angle_deg(Nu[:, cols], truth)
        full = ok & (scene["cnt"][:, cols] == 25)
        print(f"plane {k}: max error {err[ok].max():.4f} deg (full windows {err[full].max():.4f}), unquantised fit {bias[ok].max():.4f} "
              f"(full {bias[full].max():.4f}), quantisation {gold['quant_scene_deg'][k]:.4f} (full windows, the reference: {gold['quant_deg'][k]:.4f})")
        assert full.sum() > 100
        assert err[full].max() <= bias[full].max() + gold["quant_deg"][k]
        assert err[ok].max() <= bias[ok].max() + gold["quant_scene_deg"][k]
    valid = scene["nm"]
    dot = (scene["n"].astype(np.float64) * scene["c"].astype(np.float64)).sum(0)
    assert (dot[valid] < 0).all()                             # every valid normal faces the camera


def test_the_mirror_agrees_with_a_per_pixel_solver(scene):
    """The vectorised sums and the closed-form solve against numpy.linalg.solve one pixel at a time: the same validity, the same counts, and
    normals within 1e-4 degrees - five orders above float64 rounding at this conditioning, three below the quantisation's effect."""
    for kw in (dict(), dict(radius=1), dict(radius=4, edge=None), dict(radius=3, min_count=9)):
        n, nm, cnt = fit_normals_counts(scene["c"], scene["mask"], **kw)
        N, ok, cl = fx.loop_fit(scene["c"].transpose(1, 2, 0), scene["mask"], **kw)
        assert np.array_equal(nm > 0, ok) and np.array_equal(cnt, cl) and ok.any(), kw
        assert fx.angle_deg(n.transpose(1, 2, 0)[ok], N[ok]).max() <= 1e-4, kw


# ---------------------------------------------------------------------------------------------------------------- 3. masking
def test_masking_rules(scene):
    c, mask, nm, cnt = scene["c"], scene["mask"], scene["nm"], scene["cnt"]
    assert default_min_count(2) == 13 and default_min_count(1) == 5 and default_min_count(8) == 145
    assert not (nm & ~mask).any()                             # normal_mask is a subset of mask
    assert (cnt[nm] >= 13).all() and (cnt[mask & ~nm] < 13).all() and not cnt[~mask].any()
    assert not mask[fx.HOLE].any() and not nm[fx.HOLE].any() and not mask[fx.SENTINEL]      # raw 0 and raw 65535 (65.535 m > 20 m): masked
    assert nm[10, 10] and cnt[10, 10] == 25 and cnt[0, 0] == 9 and not nm[0, 0]              # a corner keeps 9 of 25: below the majority
    assert not scene["n"][:, ~nm].any() and np.abs(np.linalg.norm(scene["n"][:, nm], axis=0) - 1).max() < 1e-5
    # no neighbour across the step: the count is the number of valid pixels of the window on the centre's own side
    side = np.arange(fx.W) >= fx.STEP
    own = np.zeros((fx.H, fx.W), int)
    for i, j in zip(*np.nonzero(mask)):
        rows, cols = slice(max(0, i - 2), i + 3), slice(max(0, j - 2), j + 3)
        own[i, j] = (mask[rows, cols] & (side[cols] == side[j])[None, :]).sum()
    assert np.array_equal(cnt, own)
    _, _, wide = fit_normals_counts(c, mask, edge=None)
    assert (wide[:, fx.STEP - 2:fx.STEP + 2] > cnt[:, fx.STEP - 2:fx.STEP + 2])[mask[:, fx.STEP - 2:fx.STEP + 2]].all()      # without the test they do take part
    # the frame of zeros and the raw 65535 pixel
    z, zm = fx.backproject(fx.scene_raw()[1], fx.K40)
    n0, nm0 = fit_normals(z, zm)
    assert not zm.any() and not nm0.any() and not n0.any()
    bonn, bm = fx.backproject(fx.scene_raw(divisor=5000.0)[0], fx.K40, divisor=5000.0)         # 65535 / 5000 = 13.1 m: valid, far from its neighbours
    _, nmb, cb = fit_normals_counts(bonn, bm)
    assert bm[fx.SENTINEL] and cb[fx.SENTINEL] == 1 and not nmb[fx.SENTINEL]
    # a masked pixel may hold anything
    dirty = c.copy()
    dirty[:, ~mask] = np.nan
    a, b = fit_normals(dirty, mask)
    assert a.tobytes() == scene["n"].tobytes() and np.array_equal(b > 0, nm)


def test_a_flipped_zero_component_is_minus_zero():
    """A one-column frame with cx = 0: every x is 0, so n0 = 0 / det = +0 and the flip towards the camera makes it -0 - the value the
    device's UG_PREP_ZOOMED rule is about."""
    raw = fx.quantise(fx.plane_depth(fx.N_TILT, fx.D_TILT, np.array([[40.0, 0, 0], [0, 40.0, 12.0], [0, 0, 1]]), fx.H, 1))
    c, mask = fx.backproject(raw, np.array([[40.0, 0, 0], [0, 40.0, 12.0], [0, 0, 1]]))
    n, nm = fit_normals(c, mask, radius=2, min_count=3)
    assert nm.all() and not n[0].any() and np.signbit(n[0]).all() and not np.signbit(n[2]).any()


def test_parameter_errors(scene):
    c, mask = scene["c"], scene["mask"]
    for bad in (0, 9, -1, 2.0, True):
        with pytest.raises(ValueError, match="radius"):
            fit_normals(c, mask, radius=bad)
    with pytest.raises(ValueError, match="edge"):
        fit_normals(c, mask, edge=-0.1)
    with pytest.raises(ValueError, match="edge"):
        fit_normals(c, mask, edge=float("nan"))
    with pytest.raises(ValueError, match="min_count"):
        fit_normals(c, mask, min_count=0)
    with pytest.raises(ValueError, match="float32"):
        fit_normals(c.astype(np.float64), mask)
    with pytest.raises(ValueError, match="mask"):
        fit_normals(c, mask[:-1])
    assert fit_normals(c, mask, radius=8)[1].any() and fit_normals(c, mask, radius=1)[1].any()


def test_world_normals_are_one_rounding_of_a_float64_sum(scene):
    rng = np.random.default_rng(2)
    M = rng.normal(size=(4, 4)).astype(np.float32)
    w = world_normals(scene["n"], M)
    g = scene["n"].astype(np.float64)
    for j in range(3):
        m = [float(x) for x in M[j, :3]]
        assert np.array_equal(w[j], ((m[0] * g[0] + m[1] * g[1]) + m[2] * g[2]).astype(np.float32))
    assert w.dtype == np.float32 and not w[:, ~scene["nm"]].any()


# ---------------------------------------------------------------------------------------------------------------- 4. the loaders
@pytest.mark.parametrize("L", LAYOUTS)
def test_loader_option_adds_the_three_keys(roots, native_samples, L):
    plain = _dataset(roots, L)[0]
    s = native_samples(L)
    assert "cam_normal" not in plain and "world_normal" not in plain and "normal_mask" not in plain
    keys = list(s.keys())
    assert [k for k in keys if k not in ("cam_normal", "world_normal", "normal_mask")] == list(plain.keys())
    assert keys.index("cam_normal") + 1 == keys.index("cam_coord") and keys.index("world_normal") + 1 == keys.index("world_coord")
    assert keys.index("mask") + 1 == keys.index("normal_mask")
    for k in plain:                                           # everything else equals today's sample, bit for bit
        if isinstance(plain[k], list) and isinstance(plain[k][0], np.ndarray):
            assert np.stack(plain[k]).tobytes() == np.stack(s[k]).tobytes(), k
        else:
            assert plain[k] == s[k], k
    h, w = (480, 640) if L == "scannetv2" else (fx.H, fx.W)
    for k, shape in (("cam_normal", (3, h, w)), ("world_normal", (3, h, w)), ("normal_mask", (h, w))):
        assert len(s[k]) == fx.T and all(a.dtype == np.float32 and a.shape == shape for a in s[k]), k
    nm, mask = np.stack(s["normal_mask"]) > 0, np.stack(s["mask"]) > 0
    assert nm[0].mean() > 0.85 and not nm[1].any() and not (nm & ~mask).any()                # the scene; the frame of zeros
    # the fit ran on the full native frame, before the crop
    raw = fx.layout_raw(L)
    K = fx.LAYOUT_K[L].astype(np.float32)
    if L == "bonn":
        c = rgbd._backproject_gl(rgbd.depth_metres(raw[0], rgbd.BonnLayout()), K)
    else:
        c = rgbd._backproject_gl(raw[0].astype(np.float32) / np.float32(1000), K)
    full, bad = rgbd._masked_frame(c)
    n, valid = fit_normals(full, ~bad)
    x1 = 4 if L == "replica" else 0
    assert s["cam_normal"][0].tobytes() == np.ascontiguousarray(n[:, :, x1:x1 + w]).tobytes()
    assert s["normal_mask"][0].tobytes() == np.ascontiguousarray(valid[:, x1:x1 + w]).tobytes()
    if L == "replica":
        assert valid[:, x1].mean() > 0.8                     # the first kept column fits across the crop's edge
    # world_normal: M33 of the matrix the loader applies to cam_coord
    seq = _dataset(roots, L).samples[0][0]
    ext = [np.asarray(seq.extrinsics[i]).astype(np.float32) for i in seq.clips[0]]
    for j in range(fx.T):
        assert s["world_normal"][j].tobytes() == world_normals(s["cam_normal"][j], ext[0] @ np.linalg.inv(ext[j])).tobytes()


@pytest.mark.parametrize("L", LAYOUTS)
def test_loader_target_size_resizes_the_three_arrays(roots, native_samples, L):
    size = (12, 16)
    native = native_samples(L)
    s = _dataset(roots, L, normals="depth", input_size=size, target_size=size)[0]
    for k in ("cam_normal", "world_normal", "normal_mask"):
        for j in range(fx.T):
            assert s[k][j].dtype == np.float32 and s[k][j].shape[-2:] == size
            np.testing.assert_array_equal(s[k][j], _resize(native[k][j], *size, 0, False))
    assert np.stack(s["normal_mask"])[0].mean() > 0.8


def test_loader_options_reach_the_fit_and_bad_ones_raise(roots):
    a = _dataset(roots, "7scenes", normals="depth", normals_radius=1, normals_edge=None, normals_min_count=4)[0]
    raw = fx.layout_raw("7scenes")
    full, bad = rgbd._masked_frame(rgbd._backproject_gl(raw[0].astype(np.float32) / np.float32(1000), fx.LAYOUT_K["7scenes"].astype(np.float32)))
    n, _ = fit_normals(full, ~bad, radius=1, edge=None, min_count=4)
    assert a["cam_normal"][0].tobytes() == n.tobytes()
    for kw, word in ((dict(normals="mesh"), "normals"), (dict(normals=True), "normals"), (dict(normals="depth", normals_radius=0), "radius"),
                     (dict(normals="depth", normals_radius=9), "radius"),
                     (dict(normals="depth", normals_edge=-1.0), "edge"), (dict(normals="depth", normals_min_count=0), "min_count")):
        with pytest.raises(ValueError, match=word):
            _dataset(roots, "7scenes", **kw)
    plain = _dataset(roots, "7scenes", normals_radius=12, normals_edge=-1.0, normals_min_count=0)      # without normals= they are not looked at
    assert plain.normals is None and "cam_normal" not in plain[0]
    cfg = {"root": "x", "h": 12, "w": 16, "normals": "depth", "normals_radius": 3, "normals_edge": 0.1, "normals_min_count": 20}
    out = parse_dataset_config(cfg)
    assert {k: out[k] for k in ("normals", "normals_radius", "normals_edge", "normals_min_count")} == {k: cfg[k] for k in cfg if k.startswith("normals")}
    assert "normals" not in parse_dataset_config({"root": "x", "h": 12, "w": 16})
    with pytest.raises(ValueError, match="normals"):
        parse_dataset_config(dict(cfg, normals="mesh"))


# ---------------------------------------------------------------------------------------------------------------- 5. the evaluation
class _Model:
    """Predicts the ground truth's normals where the fit is valid and the opposite direction everywhere else: the normal metrics are 0 iff
    they are taken on ``mask & normal_mask``."""

    def forward(self, data):
        import torch
        n = np.stack(data["cam_normal"]).transpose(0, 2, 3, 1)
        nm = np.stack(data["normal_mask"]) > 0
        pred = np.where(nm[..., None], n, np.float32([0, 0, -1])).astype(np.float32)
        d = np.stack([-np.asarray(c)[2] for c in data["cam_coord"]], 0)
        return {"pred_depths": torch.from_numpy(d + 1.0).float(), "pred_normals": torch.from_numpy(pred)}


def _cfg(roots, **kw):
    return dict({"dataset": "sevenScenesDataset", "root": roots["7scenes"], "scenes": [fx.SCENE["7scenes"]], "h": 12, "w": 16,
                 "clip_length": fx.T, "clip_overlap": 0, "split": "test", "model_name": "DepthCrafter", "model_params": {},
                 "eval_normal": {"metric_names": NORMAL_KEYS}}, **kw)


def test_prepare_gt_label_gives_the_normal_masks(roots):
    s = _dataset(roots, "7scenes", normals="depth")[0]
    gt = prepare_gt_label(s)
    assert list(gt) == ["gt_world_pts", "gt_masks", "gt_poses", "gt_depths", "gt_rgbs", "gt_normals", "gt_normal_masks"]
    m = gt["gt_normal_masks"].numpy()
    assert m.dtype == bool and m.shape == (fx.T, fx.H, fx.W)
    assert np.array_equal(m, (np.stack(s["mask"]) > 0) & (np.stack(s["normal_mask"]) > 0)) and 0 < m.sum() < gt["gt_masks"].numpy().sum()
    assert "gt_normal_masks" not in prepare_gt_label(_dataset(roots, "7scenes")[0])


def test_evaluate_scores_normals_on_the_fitted_mask(roots, tmp_path):
    rows, _ = evaluate(_cfg(roots, normals="depth"), model=_Model(), save_dir=str(tmp_path), verbose=False)
    assert len(rows) == 1 and [k for k in rows[0] if k != "seq_name"] == NORMAL_KEYS
    ds = rgbd.sevenScenesDataset(roots["7scenes"], scenes=[fx.SCENE["7scenes"]], clip_length=fx.T, clip_overlap=0, input_size=(12, 16),
                                 target_size=(12, 16), normals="depth")
    data = ds[0]
    gt = prepare_gt_label(data)
    out = _Model().forward(data)
    by_hand = normal_evaluation(out["pred_normals"], gt["gt_normals"], custom_mask=gt["gt_masks"] & gt["gt_normal_masks"])
    assert {k: rows[0][k] for k in NORMAL_KEYS} == by_hand
    old = normal_evaluation(out["pred_normals"], gt["gt_normals"], custom_mask=gt["gt_masks"])
    print("on mask & normal_mask:", by_hand, "\non mask alone:", old)
    # equal unit vectors score arccos(1 / (1 + 1e-6)) = 0.081 degrees, the metric's own regulariser; four float32 ulps of the cosine on top
    floor = np.degrees(np.arccos(1 / (1 + 1e-6) - 4 * 2.0 ** -24))
    assert by_hand["normal mean"] <= floor < 0.1 and by_hand["angle < 5"] == 100.0 and old["normal mean"] > 1.0


def test_without_the_option_the_old_error_still_fires(roots, tmp_path):
    with pytest.raises(ValueError, match=r"7scenes.*cam_normal"):
        evaluate(_cfg(roots), model=_Model(), save_dir=str(tmp_path), verbose=False)


def test_the_new_symbol_is_declared_bound_and_listed():
    from test_lib_exports import header_symbols
    from unigeo_amd import _lib
    for sym in ("ug_gt_normals_opts_default", "ug_prep_gt_normals"):
        assert sym in header_symbols(("unigeo_hip.h",)) and sym in _lib.EXPORTS
    assert hasattr(_lib.Engine, "prep_gt_normals")
    with open(os.path.join(os.path.dirname(G), "..", "unigeo_amd", "csrc", "Makefile")) as f:
        assert "kernels/gt_normals.hip" in f.read()
