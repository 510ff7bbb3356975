"""GPU: the depth alignment modes on the device (ug_eval_depth_ex, ug_op_masked_median; kernels/metrics.hip) against
the reference's own outputs (tests/golden/depth_alignment_golden.npz), against numpy's sort, and against the host mirror
(harness.metrics.depth_evaluation) at clip-frame size."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "depth_alignment_golden.npz"), allow_pickle=False)
KEYS = [str(k) for k in G["keys"]]
HOST = {"metric": {"metric_scale": True}, "median": {}, "scale": {"align_with_scale": True}, "lstsq": {"align_with_lstsq": True}}
CLIPS = dict(zip(("pre_clip_min", "pre_clip_max", "post_clip_min", "post_clip_max"), (float(c) for c in G["clips"])))
BIG = (2, 384, 512)          # 393 216 pixels: above the 1024 x 256 grid cap, so every kernel's grid-stride loop takes a second trip


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _check_median(engine, pred, gt, lo=None, hi=None, max_depth=80.0, want_parity=None):
    pred, gt = np.asarray(pred, np.float32).reshape(-1), np.asarray(gt, np.float32).reshape(-1)
    mp, mg, cnt = engine.op_masked_median(pred, gt, max_depth=max_depth, pre_clip_min=lo, pre_clip_max=hi)
    m1 = (gt > 0) & (gt < max_depth)
    assert cnt == int(m1.sum())
    if want_parity is not None:
        assert cnt % 2 == want_parity
    p = pred[m1]
    if lo is not None:
        p = np.maximum(p, np.float32(lo))
    if hi is not None:
        p = np.minimum(p, np.float32(hi))
    k = (cnt - 1) // 2
    assert _bits(mg) == _bits(np.sort(gt[m1])[k]), (mg, np.sort(gt[m1])[k])
    assert _bits(mp) == _bits(np.sort(p)[k]), (mp, np.sort(p)[k])
    return mp, mg, cnt


@pytest.mark.parametrize("n,parity", [(1, 1), (255, 1), (255, 0), (257, 1), (257, 0), (1680, 1), (1680, 0), (BIG[0] * BIG[1] * BIG[2], 0),
                                      (BIG[0] * BIG[1] * BIG[2], 1)])
def test_masked_median_equals_sorted_element(engine, n, parity):
    rng = np.random.default_rng(n + parity)
    gt = rng.uniform(0.5, 6.0, n).astype(np.float32)
    pred = (0.7 * gt + 0.3 + rng.standard_normal(n)).astype(np.float32)            # mixed sign
    if n > 1:
        bad = rng.choice(n, n // 10, replace=False)
        gt[bad[::2]] = 0.0; gt[bad[1::2]] = 90.0
        valid = np.flatnonzero((gt > 0) & (gt < 80))
        if valid.size % 2 != parity:
            gt[valid[0]] = 0.0
    _check_median(engine, pred, gt, want_parity=parity)


def test_masked_median_ties_signs_and_clips(engine):
    rng = np.random.default_rng(5)
    n = 1680
    gt = rng.uniform(0.5, 6.0, n).astype(np.float32)
    # every value equal
    mp, _, _ = _check_median(engine, np.full(n, 2.5, np.float32), gt)
    assert mp == 2.5
    mp, mg, _ = _check_median(engine, np.full(n, -1.25, np.float32), np.full(n, 3.0, np.float32))
    assert (mp, mg) == (-1.25, 3.0)
    # the fixture's 8-level prediction: the median bin is full of ties
    mp, _, _ = _check_median(engine, G["q_pred"], G["q_gt"])
    assert mp in np.unique(G["q_pred"])
    # mixed sign with both zeros: 30 % negative, 10 % zeros of either sign, 60 % positive -> a positive median above all of them
    pred = np.concatenate([-rng.uniform(1e-30, 5, 504), np.zeros(84), -np.zeros(84), rng.uniform(1e-30, 5, 1008)]).astype(np.float32)
    pred = pred[rng.permutation(n)]
    assert (_bits(pred) == 0x80000000).sum() == 84 and (_bits(pred) == 0).sum() == 84
    mp, _, _ = _check_median(engine, pred, gt)
    assert mp > 0
    _check_median(engine, -pred, gt)                                                # mirrored: a negative median below all the zeros
    # the median IS a zero (45 % negative, 10 % zeros, 45 % positive): numpy leaves the order of -0.0 and 0.0 open, so compare the value
    pred = np.concatenate([-rng.uniform(1e-30, 5, 756), np.zeros(84), -np.zeros(84), rng.uniform(1e-30, 5, 756)]).astype(np.float32)
    pred = pred[rng.permutation(n)]
    mp, mg, cnt = engine.op_masked_median(pred, gt)
    assert cnt == n and mp == 0.0 and _bits(mg) == _bits(np.sort(gt)[(n - 1) // 2])
    # a pre-clip that collapses 30 % of the values onto the lower bound; then 60 %, so that the median is the bound itself
    pred = rng.uniform(0.0, 1.0, n).astype(np.float32)
    _check_median(engine, pred, gt, lo=float(np.quantile(pred, 0.3)))
    mp, _, _ = _check_median(engine, pred, gt, lo=0.6)
    assert mp == np.float32(0.6)
    mp, _, _ = _check_median(engine, pred, gt, hi=0.3)
    assert mp == np.float32(0.3)
    _check_median(engine, pred - 0.5, gt, lo=-0.2, hi=0.25)
    # max_depth off: gt = 90 counts
    gt2 = gt.copy(); gt2[:200] = 90.0
    _, _, c_on = _check_median(engine, pred, gt2)
    mp, mg, c_off = engine.op_masked_median(pred, gt2, max_depth=None)
    assert (c_on, c_off) == (n - 200, n) and _bits(mg) == _bits(np.sort(gt2)[(n - 1) // 2]) and _bits(mp) == _bits(np.sort(pred)[(n - 1) // 2])


def test_masked_median_without_a_valid_pixel(engine):
    mp, mg, cnt = engine.op_masked_median(np.ones(257, np.float32), np.zeros(257, np.float32))
    assert cnt == 0
    res, st = engine.eval_depth(np.zeros(257, np.float32), pred=np.ones(257, np.float32), alignment="median")
    assert res["valid_pixels"] == 0 and all(res[k] == 0 for k in KEYS[:8]) and st == (0.0, 0.0)


@pytest.mark.parametrize("mode", ["metric", "median", "scale", "lstsq"])
def test_no_valid_pixel_convention_on_the_device(engine, mode):
    res, st, emap = engine.eval_depth(np.zeros((1, 4, 4), np.float32), np.ones((1, 4, 4), bool), pred=np.ones((1, 4, 4), np.float32),
                                      alignment=mode, return_error_map=True, **CLIPS)
    assert res["valid_pixels"] == 0 and all(res[k] == 0 for k in KEYS[:8])
    assert st == ((1.0, 0.0) if mode == "metric" else (0.0, 0.0)) and not emap.any()


@pytest.mark.parametrize("clip", ["noclip", "clip"])
@pytest.mark.parametrize("mode", ["metric", "median", "lstsq"])
@pytest.mark.parametrize("tag", ["a", "q", "e"])
def test_device_modes_match_the_reference(engine, tag, mode, clip):
    """The reference's own results at the existing device bound (rel 3e-5, abs 1e-6); error map rtol 1e-5 - with the absolute term
    1e-6 under lstsq only, where the reference's (s, t) come out of a float32 LAPACK solve and the device's out of float64 normal
    equations (see tests/test_depth_alignment_cpu.py::test_host_modes_match_the_reference for the reasoning)."""
    res, (s, t), emap = engine.eval_depth(G[f"{tag}_gt"], G[f"{tag}_mask"], pred=G[f"{tag}_pred"], alignment=mode, return_error_map=True,
                                          **(CLIPS if clip == "clip" else {}))
    want = G[f"{tag}_{mode}_{clip}_vals"]
    for k, w in zip(KEYS[:8], want):
        print(f"{tag} {mode} {clip} {k}: device {res[k]:.9g} reference {w:.9g}")
        assert res[k] == pytest.approx(w, rel=3e-5, abs=1e-6), k
    assert res["valid_pixels"] == int(want[8])
    ref_map = G[f"{tag}_{mode}_{clip}_emap"]
    print(f"{tag} {mode} {clip} error map: max abs diff {np.abs(emap - ref_map).max():.3e}")
    np.testing.assert_allclose(emap, ref_map, rtol=1e-5, atol=1e-6 if mode == "lstsq" else 0)
    if mode != "lstsq":
        assert _bits(s) == _bits(G[f"{tag}_{mode}_{clip}_s"]) and t == 0.0


@pytest.mark.parametrize("clip", ["noclip", "clip"])
@pytest.mark.parametrize("tag", ["a", "q", "e"])
def test_device_scale_mode_within_twice_the_measured_distance(engine, tag, clip):
    """``scale`` against the reference at twice the reference-vs-restatement distance stored in the fixture (the same bound as the CPU test)."""
    bound = 2.0 * float(G["scale_distance"])
    p, g = G[f"{tag}_pred"], G[f"{tag}_gt"]
    res, (s, t), emap = engine.eval_depth(g, G[f"{tag}_mask"], pred=p, alignment="scale", return_error_map=True, **(CLIPS if clip == "clip" else {}))
    want = G[f"{tag}_scale_{clip}_vals"]
    for k, w in zip(KEYS[:8], want):
        print(f"{tag} scale {clip} {k}: device {res[k]:.9g} reference {w:.9g} rel {abs(res[k] - w) / max(abs(w), 1e-12):.3e}")
        assert res[k] == pytest.approx(w, rel=bound, abs=1e-6), k
    assert res["valid_pixels"] == int(want[8]) and t == 0.0
    assert s == pytest.approx(float(G[f"{tag}_scale_{clip}_s"]), rel=bound)
    m1 = (g > 0) & (g < 80)
    ref = np.zeros_like(g)
    ref[m1] = np.abs(p[m1] * np.float32(s) - g[m1]) / g[m1]          # the stated formula at the returned s
    np.testing.assert_allclose(emap, ref, rtol=1e-5)


def _big_input(seed=11):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.5, 6.0, BIG).astype(np.float32)
    gt[rng.uniform(size=BIG) < 0.05] = 0.0
    pred = (0.7 * gt + 0.3 + 0.2 * rng.standard_normal(BIG)).astype(np.float32)
    out = rng.uniform(size=BIG) < 0.02                                  # 2 % outlier predictions
    pred[out] *= rng.uniform(3.0, 10.0, int(out.sum())).astype(np.float32)
    mask = rng.uniform(size=BIG) > 0.2
    return pred, gt, mask


@pytest.fixture(scope="module")
def big():
    return _big_input()


def _out11(engine, pred, gt, mask, ex):
    from unigeo_amd._lib import DepthEvalOptsC, _f32, _ptr
    p, g = _f32(pred), _f32(gt)
    m = np.ascontiguousarray(mask.astype(np.uint8))
    out = np.full(11, -1.0, np.float64)
    if ex:
        o = DepthEvalOptsC()
        engine.lib.ug_depth_eval_opts_default(C.byref(o))
        assert o.alignment == 0 and o.max_depth == 80.0 and all(np.isnan(getattr(o, f)) for f in ("pre_clip_min", "pre_clip_max", "post_clip_min", "post_clip_max"))
        rc = engine.lib.ug_eval_depth_ex(engine.ctx, _ptr(p), _ptr(g), _ptr(m), g.size, C.byref(o), _ptr(out), None)
    else:
        rc = engine.lib.ug_eval_depth(engine.ctx, _ptr(p), _ptr(g), _ptr(m), g.size, 80.0, _ptr(out))
    assert rc == 0
    return out


def test_default_options_equal_ug_eval_depth_bytes(engine, big):
    for pred, gt, mask in ((G["a_pred"], G["a_gt"], G["a_mask"]), big):
        assert _out11(engine, pred, gt, mask, True).tobytes() == _out11(engine, pred, gt, mask, False).tobytes()


@pytest.mark.parametrize("mode", ["median", "metric"])
def test_device_matches_the_host_mirror_at_frame_size(engine, big, mode):
    from unigeo_amd.harness import depth_evaluation
    pred, gt, mask = big
    res, (s, t) = engine.eval_depth(gt, mask, pred=pred, alignment=mode)
    ref, (sh, th) = depth_evaluation(pred, gt, custom_mask=mask, **HOST[mode])
    assert _bits(s) == _bits(sh) and (t, th) == (0.0, 0.0)
    for k in KEYS[:8]:
        assert res[k] == pytest.approx(ref[k], rel=2e-4), k
    assert res["valid_pixels"] == ref["valid_pixels"]
    clipped, _ = engine.eval_depth(gt, mask, pred=pred, alignment=mode, **CLIPS)
    ref_c, _ = depth_evaluation(pred, gt, custom_mask=mask, **HOST[mode], **CLIPS)
    for k in KEYS[:8]:
        assert clipped[k] == pytest.approx(ref_c[k], rel=2e-4), k
    assert clipped["Abs Rel"] != res["Abs Rel"]


def test_device_scale_within_the_order_spread_of_the_restatement(engine, big):
    """``scale`` moves with the summation order alone.  The spread is measured HERE on the host restatement -
    index order and two seeded permutations - never on the device; the device's fixed order is a fourth draw from the same
    distribution, hence the factor 3.  Two device runs are equal bit for bit."""
    from unigeo_amd.harness.metrics import _scale_l1
    pred, gt, mask = big
    m1 = (gt > 0) & (gt < 80)
    p, g = pred[m1], gt[m1]
    hosts = [_scale_l1(p, g)]
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(p.size)
        hosts.append(_scale_l1(p[perm], g[perm]))
    spread = max(abs(a - b) for a in hosts for b in hosts)
    r1 = engine.eval_depth(gt, mask, pred=pred, alignment="scale")
    r2 = engine.eval_depth(gt, mask, pred=pred, alignment="scale")
    s = r1[1][0]
    print(f"scale at {p.size} pixels: host s {hosts}, relative order spread {spread / hosts[0]:.3e}, device s {s!r}, "
          f"device - host(index order) relative {abs(s - hosts[0]) / hosts[0]:.3e}")
    assert spread > 0
    assert abs(s - hosts[0]) <= 3.0 * spread
    assert r1 == r2                                                     # the same bits twice


def test_device_scale_equals_the_host_at_1680_pixels(engine):
    """On a well-conditioned small input the order spread is ~1e-8: the device's s is the host's to rel 1e-6."""
    from unigeo_amd.harness import depth_evaluation
    rng = np.random.default_rng(3)
    gt = rng.uniform(0.5, 6.0, (3, 20, 28)).astype(np.float32)
    gt[0, :3] = 0.0; gt[1, 5, 5] = 90.0
    pred = (0.7 * gt + 0.3 + 0.2 * rng.standard_normal(gt.shape)).astype(np.float32)
    mask = rng.uniform(size=gt.shape) > 0.2
    res, (s, _) = engine.eval_depth(gt, mask, pred=pred, alignment="scale")
    ref, (sh, _) = depth_evaluation(pred, gt, custom_mask=mask, align_with_scale=True)
    print(f"scale at 1680 pixels: device s {s!r} host s {sh!r} rel {abs(s - sh) / sh:.3e}")
    assert s == pytest.approx(sh, rel=1e-6)
    for k in KEYS[:8]:
        assert res[k] == pytest.approx(ref[k], rel=3e-5, abs=1e-6), k


def test_unknown_alignment_code_is_an_error_not_a_crash(engine):
    from unigeo_amd._lib import DepthEvalOptsC, _ptr
    o = DepthEvalOptsC()
    engine.lib.ug_depth_eval_opts_default(C.byref(o))
    o.alignment = 7
    g = np.ones(16, np.float32); out = np.zeros(11, np.float64)
    rc = engine.lib.ug_eval_depth_ex(engine.ctx, _ptr(g), _ptr(g), None, 16, C.byref(o), _ptr(out), None)
    assert rc != 0 and "alignment" in engine.lib.ug_last_error(engine.ctx).decode()
    with pytest.raises(ValueError):
        engine.eval_depth(g, pred=g, alignment="lad")
    res, st = engine.eval_depth(g, pred=g, alignment="metric")           # the context still works
    assert res["Abs Rel"] == 0.0 and st == (1.0, 0.0)


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
    for mode in ("median", "scale", "metric"):
        a = eng.eval_depth(gt, mask, alignment=mode, return_error_map=True)
        b = eng.eval_depth(gt, mask, pred=depth, alignment=mode, return_error_map=True)
        assert a[0] == b[0] and a[1] == b[1] and a[2].tobytes() == b[2].tobytes(), mode
        assert a[0]["valid_pixels"] > 0 and np.isfinite(a[0]["Abs Rel"])


def test_harness_device_metrics_honour_depth_alignment(tiny_plugin, tmp_path):
    from unigeo_amd.harness import SyntheticGeometryDataset, evaluate
    cfg = {"root": "x", "h": 64, "w": 64, "clip_length": 3, "clip_overlap": 1,
           "eval_depth": {"metric_names": ["Abs Rel", "delta < 1.25"], "depth_alignment": "median"}}
    ds = SyntheticGeometryDataset(clip_length=3, clip_overlap=1, input_size=(64, 64), num_frames=5)
    host, _ = evaluate(cfg, dataset=ds, model=tiny_plugin, save_dir=str(tmp_path / "h"), verbose=False)
    dev, _ = evaluate(cfg, dataset=ds, model=tiny_plugin, save_dir=str(tmp_path / "d"), verbose=False, device_metrics=True)
    lsq, _ = evaluate({**cfg, "eval_depth": {"metric_names": ["Abs Rel", "delta < 1.25"]}}, dataset=ds, model=tiny_plugin,
                      save_dir=str(tmp_path / "l"), verbose=False, device_metrics=True)
    assert len(host) == len(dev) == 3
    for h_, d_, l_ in zip(host, dev, lsq):
        for k in ("Abs Rel", "delta < 1.25"):
            assert d_[k] == pytest.approx(h_[k], rel=2e-4), k
        assert d_["valid_pixels"] == h_["valid_pixels"] and d_["Abs Rel"] != l_["Abs Rel"]      # median, not the old least squares
