"""GPU: the exact L1 scale-and-shift alignment on the device (ug_op_l1_fit, ug_eval_depth_ex with UG_ALIGN_L1; k_l1_* in kernels/metrics.hip,
DESIGN.md section 23) against the host mirror (harness.metrics.l1_fit / depth_evaluation): the same pivots, the same step count and the same
bits of (s, t).  Every quantity the kernels accumulate is an integer, so nothing here has a tolerance except the float32 metrics pass."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
A = np.load(os.path.join(GOLD, "depth_alignment_golden.npz"), allow_pickle=False)
G = np.load(os.path.join(GOLD, "depth_l1_golden.npz"), allow_pickle=False)
KEYS = [str(k) for k in G["keys"]]
CLIPS = dict(zip(("pre_clip_min", "pre_clip_max", "post_clip_min", "post_clip_max"), (float(c) for c in G["clips"])))
BIG = (2, 384, 512)          # 393 216 pixels: above the 1024 x 256 grid cap, so every loop over the pixels takes a second trip


def _bits64(x):
    return np.float64(x).tobytes()


def _host_fit(pred, gt, max_depth=80.0, lo=None, hi=None):
    from unigeo_amd.harness.metrics import l1_fit
    pred, gt = np.asarray(pred, np.float32).reshape(-1), np.asarray(gt, np.float32).reshape(-1)
    m1 = (gt > 0) & (gt < max_depth) if max_depth is not None else gt > 0
    p = pred[m1]
    if lo is not None:
        p = np.maximum(p, np.float32(lo))
    if hi is not None:
        p = np.minimum(p, np.float32(hi))
    return l1_fit(p, gt[m1])


def _check_fit(engine, pred, gt, max_depth=80.0, lo=None, hi=None):
    from unigeo_amd.harness.metrics import L1_MAX_STEPS
    s, t, info = engine.op_l1_fit(gt, pred=pred, max_depth=max_depth, pre_clip_min=lo, pre_clip_max=hi)
    hs, ht, hinfo = _host_fit(pred, gt, max_depth, lo, hi)
    print(f"device (s, t) = ({s!r}, {t!r}) {info}; host ({hs!r}, {ht!r}) {hinfo}")
    assert info == hinfo
    assert _bits64(s) == _bits64(hs) and _bits64(t) == _bits64(ht)
    assert info["certified"] == 1 and info["steps"] <= L1_MAX_STEPS
    return s, t, info


def _noisy(n, seed):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.5, 6.0, n).astype(np.float32)
    pred = (0.7 * gt + 0.3 + 0.2 * rng.standard_normal(n)).astype(np.float32)
    return pred, gt


@pytest.mark.parametrize("n", [1, 2, 255, 257, 1680])
def test_fit_equals_the_host_mirror_at_small_sizes(engine, n):
    pred, gt = _noisy(n, n)
    _, _, info = _check_fit(engine, pred, gt)
    assert (info["steps"] == 0 and info["k"] == -1) if n == 1 else (info["steps"] >= 1 and info["k"] >= 0)


@pytest.fixture(scope="module")
def big():
    """Mixed-sign predictions, 10 % invalid ground truth, 2 % gross outliers."""
    rng = np.random.default_rng(23)
    gt = rng.uniform(0.5, 6.0, BIG).astype(np.float32)
    pred = (0.7 * gt - 2.0 + 0.2 * rng.standard_normal(BIG)).astype(np.float32)          # about a third of the predictions are negative
    out = rng.uniform(size=BIG) < 0.02
    pred[out] *= rng.uniform(3.0, 10.0, int(out.sum())).astype(np.float32)
    gt[rng.uniform(size=BIG) < 0.1] = 0.0
    assert (pred < 0).mean() > 0.1 and (pred > 0).mean() > 0.1
    return pred, gt


def test_fit_equals_the_host_mirror_above_the_grid_cap(engine, big):
    pred, gt = big
    _check_fit(engine, pred, gt)


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("tag", ["a", "q", "e"])
def test_fit_equals_the_host_mirror_on_the_fixtures(engine, tag, clip):
    kw = {"lo": CLIPS["pre_clip_min"], "hi": CLIPS["pre_clip_max"]} if clip else {}
    _check_fit(engine, A[f"{tag}_pred"], A[f"{tag}_gt"], **kw)


def test_fit_on_the_degenerate_integer_input(engine):
    """Many points share each line of this input: the vertex check has tied points to ask."""
    _, _, info = _check_fit(engine, G["int_pred"], G["int_gt"])
    assert info["k"] >= 0


def test_fit_with_all_predictions_equal(engine):
    gt = np.random.default_rng(5).uniform(0.5, 6.0, 300).astype(np.float32)
    s, t, info = _check_fit(engine, np.full(300, 1.25, np.float32), gt)
    assert s == 0.0 and t == float(np.sort(gt)[149]) and info == {"j": 0, "k": -1, "steps": 0, "certified": 1}
    _check_fit(engine, np.zeros(300, np.float32), gt)
    pred, _ = _noisy(300, 6)
    s, t, info = _check_fit(engine, pred, gt, lo=100.0)          # a pre-clip above every prediction collapses them all
    assert s == 0.0 and info["steps"] == 0


def test_fit_without_a_valid_pixel(engine):
    s, t, info = _check_fit(engine, np.ones(257, np.float32), np.zeros(257, np.float32))
    assert (s, t) == (0.0, 0.0) and info == {"j": -1, "k": -1, "steps": 0, "certified": 1}
    res, st, emap = engine.eval_depth(np.zeros((1, 4, 4), np.float32), np.ones((1, 4, 4), bool), pred=np.ones((1, 4, 4), np.float32),
                                      alignment="l1", return_error_map=True)
    assert st == (0.0, 0.0) and res["valid_pixels"] == 0 and all(res[k] == 0 for k in KEYS[:8]) and not emap.any()


def test_fit_with_max_depth_off(engine):
    pred, gt = _noisy(1680, 9)
    gt[::7] = 90.0 + gt[::7]                     # beyond max_depth = 80: valid only when the bound is off
    gt[::11] = 0.0
    a = _check_fit(engine, pred, gt, max_depth=None)
    b = _check_fit(engine, pred, gt)
    assert a[:2] != b[:2]


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("tag", ["a", "q", "e"])
def test_eval_depth_l1_matches_the_host_function(engine, tag, clip):
    from unigeo_amd.harness import depth_evaluation
    p, g, m = A[f"{tag}_pred"], A[f"{tag}_gt"], A[f"{tag}_mask"]
    kw = CLIPS if clip else {}
    res, (s, t), emap = engine.eval_depth(g, m, pred=p, alignment="l1", return_error_map=True, **kw)
    ref, (sh, th), emap_h = depth_evaluation(p, g, custom_mask=m, align_with_l1=True, return_error_map=True, **kw)
    assert np.float32(s).tobytes() == np.float32(sh).tobytes() and np.float32(t).tobytes() == np.float32(th).tobytes()
    assert s == float(np.float32(s)) and t == float(np.float32(t))          # rounded once to float32
    for k in KEYS[:8]:
        print(f"{tag} {k}: device {res[k]:.9g} host {ref[k]:.9g}")
        assert res[k] == pytest.approx(ref[k], rel=3e-5, abs=1e-6), k
    assert res["valid_pixels"] == ref["valid_pixels"]
    np.testing.assert_allclose(emap, emap_h, rtol=1e-5)
    assert engine.l1_info["certified"] == 1 and engine.l1_info["steps"] >= 1


def test_eval_depth_l1_above_the_grid_cap(engine, big):
    from unigeo_amd.harness import depth_evaluation
    pred, gt = big
    res, (s, t) = engine.eval_depth(gt, pred=pred, alignment="l1")
    hs, ht, _ = _host_fit(pred, gt)
    assert np.float32(s).tobytes() == np.float32(hs).tobytes() and np.float32(t).tobytes() == np.float32(ht).tobytes()
    assert res["valid_pixels"] == int(((gt > 0) & (gt < 80)).sum())
    ls = depth_evaluation(pred, gt, align_with_lstsq=True)[1]
    assert (s, t) != ls


def test_two_calls_give_the_same_bits_and_a_rejected_alignment_leaves_the_context_usable(engine):
    p, g, m = A["q_pred"], A["q_gt"], A["q_mask"]
    a = engine.eval_depth(g, m, pred=p, alignment="l1", return_error_map=True)
    with pytest.raises(ValueError):
        engine.eval_depth(g, m, pred=p, alignment="lad")
    b = engine.eval_depth(g, m, pred=p, alignment="l1", return_error_map=True)
    assert a[0] == b[0] and a[1] == b[1] and a[2].tobytes() == b[2].tobytes()
    f1, f2 = engine.op_l1_fit(g, pred=p), engine.op_l1_fit(g, pred=p)
    assert f1 == f2 and _bits64(f1[0]) == _bits64(f2[0]) and _bits64(f1[1]) == _bits64(f2[1])
    assert np.float32(f1[0]) == np.float32(a[1][0]) and np.float32(f1[1]) == np.float32(a[1][1])


def test_more_tied_points_than_the_cap_is_uncertified_and_warns_once():
    """5 000 collinear points: 4 999 of them tie at the first vertex, above the cap of 4 096.  Device and mirror both stop there with the
    vertex they stand on (which here is the minimiser, F = 0) and certified = 0; ``Engine.eval_depth`` says so once per engine."""
    import warnings
    from unigeo_amd._lib import Engine
    from unigeo_amd.harness.metrics import l1_fit
    pred = np.arange(5000, dtype=np.float32)
    gt = 2 * pred + 1
    eng = Engine(0, 64 << 20, 1 << 20)
    try:
        assert eng.l1_info is None
        fit = eng.op_l1_fit(gt, pred=pred, max_depth=None)
        assert fit == l1_fit(pred, gt) == (2.0, 1.0, {"j": 2499, "k": 0, "steps": 1, "certified": 0})
        with pytest.warns(RuntimeWarning, match="uncertified"):
            _, st = eng.eval_depth(gt, pred=pred, max_depth=None, alignment="l1")
        assert st == (2.0, 1.0) and eng.l1_info == fit[2]
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert eng.eval_depth(gt, pred=pred, max_depth=None, alignment="l1")[1] == st
    finally:
        eng.close()


def test_a_workspace_too_small_is_an_error_not_a_crash(big):
    from unigeo_amd._lib import Engine
    pred, gt = big
    small = Engine(0, 4 << 20, 1 << 20)          # the two uploads of the big input fit, the compacted points do not
    try:
        with pytest.raises(RuntimeError, match="arena"):
            small.op_l1_fit(gt, pred=pred)
        s, t, info = small.op_l1_fit(gt.reshape(-1)[:1000], pred=pred.reshape(-1)[:1000])          # the context still works
        assert info["certified"] == 1
    finally:
        small.close()


@pytest.fixture(scope="module")
def tiny_plugin():
    from unigeo_amd import weights as W
    from unigeo_amd.model import DepthCrafter
    m = DepthCrafter(synthetic_weights=True, cfgs=W.tiny_cfgs(), num_inference_steps=2, workspace_bytes=3 << 30)
    yield m
    m.pipeline.engine.close()


def test_resident_depth_equals_the_downloaded_depth(tiny_plugin):
    from unigeo_amd.synthetic import synthetic_clip
    tiny_plugin.forward(synthetic_clip(3, 64, 64, seed=1))
    eng = tiny_plugin.pipeline.engine
    _, depth, _ = eng.get_outputs(frames=False, depth=True)
    rng = np.random.default_rng(0)
    gt = rng.uniform(0.5, 6.0, depth.shape).astype(np.float32); gt[0, :5] = 0.0
    mask = rng.uniform(size=depth.shape) > 0.2
    a = eng.eval_depth(gt, mask, alignment="l1", return_error_map=True)
    b = eng.eval_depth(gt, mask, pred=depth, alignment="l1", return_error_map=True)
    assert a[0] == b[0] and a[1] == b[1] and a[2].tobytes() == b[2].tobytes()
    assert a[0]["valid_pixels"] > 0 and np.isfinite(a[0]["Abs Rel"])
    fa, fb = eng.op_l1_fit(gt), eng.op_l1_fit(gt, pred=depth)
    assert fa == fb and _bits64(fa[0]) == _bits64(fb[0]) and _bits64(fa[1]) == _bits64(fb[1])
    assert fa[2] == _host_fit(depth, gt)[2]


def test_harness_device_metrics_take_the_l1_mode(tiny_plugin, tmp_path):
    from unigeo_amd.harness import SyntheticGeometryDataset, evaluate
    cfg = {"root": "x", "h": 64, "w": 64, "clip_length": 3, "clip_overlap": 1,
           "eval_depth": {"metric_names": ["Abs Rel", "delta < 1.25"], "depth_alignment": "l1"}}
    ds = SyntheticGeometryDataset(clip_length=3, clip_overlap=1, input_size=(64, 64), num_frames=5)
    host, _ = evaluate(cfg, dataset=ds, model=tiny_plugin, save_dir=str(tmp_path / "h"), verbose=False)
    dev, _ = evaluate(cfg, dataset=ds, model=tiny_plugin, save_dir=str(tmp_path / "d"), verbose=False, device_metrics=True)
    assert len(host) == len(dev) == len(ds)
    for h, d in zip(host, dev):
        for k in ("Abs Rel", "delta < 1.25"):
            assert d[k] == pytest.approx(h[k], rel=2e-4), k          # the bound of the other modes' harness test
        assert d["valid_pixels"] == h["valid_pixels"]
