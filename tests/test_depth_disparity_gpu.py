"""GPU: depth evaluation in disparity space on the device (ug_eval_depth_ex2, ug_dc_get_disparity; k_disp_target / k_disp_metrics in
kernels/metrics.hip, k_disparity_from_frames in kernels/misc.hip) against the reference's own outputs
(tests/golden/depth_disparity_golden.npz), against the host mirror (harness.metrics.depth_evaluation(align_space="disparity")) at
clip-frame size, on the resident disparity of a tiny run, and through the harness loop."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "depth_disparity_golden.npz"), allow_pickle=False)
KEYS = [str(k) for k in G["keys"]]
HOST = {"metric": {"metric_scale": True}, "median": {}, "scale": {"align_with_scale": True}, "lstsq": {"align_with_lstsq": True},
        "l1": {"align_with_l1": True}}
CLIPS = dict(zip(("pre_clip_min", "pre_clip_max", "post_clip_min", "post_clip_max"), (float(c) for c in G["clips"])))
BIG = (2, 384, 512)          # 393 216 pixels: above the 1024 x 256 grid cap, so every kernel's grid-stride loop takes a second trip
f32 = np.float32


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _host(pred, gt, mask, mode, **kw):
    from unigeo_amd.harness import depth_evaluation
    return depth_evaluation(pred, gt, custom_mask=mask, align_space="disparity", return_error_map=True, **HOST[mode], **kw)


def _dev(engine, pred, gt, mask, mode, **kw):
    return engine.eval_depth(gt, mask, pred=pred, alignment=mode, space="disparity", return_error_map=True, **kw)


def _min_abs_a(pred, gt, s, t, pre=None):
    """The smallest |aligned disparity| on mask1, of the pre-clipped prediction (the metrics) and of the original one (the error map)."""
    m1 = (gt > 0) & (gt < 80)
    p = pred[m1]
    pc = np.minimum(np.maximum(p, f32(pre[0])), f32(pre[1])) if pre else p
    return min(float(np.abs(f32(s) * pc + f32(t)).min()), float(np.abs(p * f32(s) + f32(t)).min()))


# ------------------------------------------------------------------------------------------------- golden cases
@pytest.mark.parametrize("clip", ["noclip", "clip"])
@pytest.mark.parametrize("mode", ["metric", "median", "lstsq"])
@pytest.mark.parametrize("tag", ["a", "q", "e"])
def test_device_modes_match_the_reference(engine, tag, mode, clip):
    """The reference's own ``disp_input=True`` results at the existing device bound (rel 3e-5, abs 1e-6); error map rtol 1e-5, with the
    absolute term 1e-6 under lstsq only; s bits equal where the mode has no shift."""
    res, (s, t), emap = _dev(engine, G[f"{tag}_pred"], G[f"{tag}_gt"], G[f"{tag}_mask"], mode, **(CLIPS if clip == "clip" else {}))
    want = G[f"{tag}_{mode}_{clip}_vals"]
    worst = max(abs(res[k] - w) / max(abs(w), 1e-12) for k, w in zip(KEYS[:8], want))
    ref_map = G[f"{tag}_{mode}_{clip}_emap"]
    print(f"{tag} {mode} {clip}: largest relative distance of a metric to the reference {worst:.3e}; error map max abs diff "
          f"{np.abs(emap - ref_map).max():.3e}")
    for k, w in zip(KEYS[:8], want):
        assert res[k] == pytest.approx(w, rel=3e-5, abs=1e-6), k
    assert res["valid_pixels"] == int(want[8])
    np.testing.assert_allclose(emap, ref_map, rtol=1e-5, atol=1e-6 if mode == "lstsq" else 0)
    if mode != "lstsq":
        assert _bits(s) == _bits(G[f"{tag}_{mode}_{clip}_s"]) and t == 0.0


@pytest.mark.parametrize("clip", ["noclip", "clip"])
@pytest.mark.parametrize("tag", ["a", "q", "e"])
def test_device_scale_mode_within_twice_the_measured_distance(engine, tag, clip):
    from unigeo_amd.harness.metrics import disparity_to_depth
    bound = 2.0 * float(G["scale_distance"])
    p, g = G[f"{tag}_pred"], G[f"{tag}_gt"]
    res, (s, t), emap = _dev(engine, p, g, G[f"{tag}_mask"], "scale", **(CLIPS if clip == "clip" else {}))
    want = G[f"{tag}_scale_{clip}_vals"]
    for k, w in zip(KEYS[:8], want):
        print(f"{tag} scale {clip} {k}: device {res[k]:.9g} reference {w:.9g} rel {abs(res[k] - w) / max(abs(w), 1e-12):.3e}")
        assert res[k] == pytest.approx(w, rel=bound, abs=1e-6), k
    assert res["valid_pixels"] == int(want[8]) and t == 0.0
    assert s == pytest.approx(float(G[f"{tag}_scale_{clip}_s"]), rel=bound)
    m1 = (g > 0) & (g < 80)
    ref = np.zeros_like(g)
    ref[m1] = np.abs(disparity_to_depth(p[m1] * f32(s)) - g[m1]) / g[m1]          # the stated formula at the returned s: the same float32 operations
    assert emap.tobytes() == ref.tobytes()


# ------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("n", [1, 257, 1680])
def test_one_thread_a_block_boundary_and_a_partial_last_block(engine, n):
    rng = np.random.default_rng(n)
    gt = rng.uniform(0.5, 4.0, n).astype(f32)
    pred = (0.5 / gt + 0.2 + 0.01 * rng.standard_normal(n)).astype(f32)
    mask = np.ones(n, bool)
    if n > 1:
        pred[rng.uniform(size=n) < 0.03] *= f32(-1)
        gt[rng.uniform(size=n) < 0.1] = 0.0
        mask = rng.uniform(size=n) > 0.2
    for mode in ("metric", "median", "l1"):
        ref, (sh, th), ref_map = _host(pred, gt, mask, mode, post_clip_max=80.0, disp_clip_min=1e-3)
        res, (s, t), emap = _dev(engine, pred, gt, mask, mode, post_clip_max=80.0, disp_clip_min=1e-3)
        assert (_bits(s), _bits(t)) == (_bits(sh), _bits(th)), mode
        assert emap.tobytes() == ref_map.tobytes(), mode
        assert res["valid_pixels"] == ref["valid_pixels"]
        for k in KEYS[:8]:
            assert res[k] == pytest.approx(ref[k], rel=3e-5, abs=1e-6), (mode, k)


@pytest.mark.parametrize("mode", ["metric", "median", "scale", "lstsq", "l1"])
def test_no_valid_pixel_convention_on_the_device(engine, mode):
    res, st, emap = _dev(engine, np.ones((1, 4, 4), f32), np.zeros((1, 4, 4), f32), np.ones((1, 4, 4), bool), mode, **CLIPS)
    assert res["valid_pixels"] == 0 and all(res[k] == 0 for k in KEYS[:8])
    assert st == ((1.0, 0.0) if mode == "metric" else (0.0, 0.0)) and not emap.any()


# ------------------------------------------------------------------------------------------------- frame size
def _big_input(seed=11):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.5, 4.0, BIG).astype(f32)
    pred = (0.5 / gt + 0.2 + 0.01 * rng.standard_normal(BIG)).astype(f32)
    out = rng.uniform(size=BIG) < 0.02                                  # 2 % outlier predictions
    pred[out] *= rng.uniform(1.5, 3.0, int(out.sum())).astype(f32)
    neg = rng.uniform(size=BIG) < 0.01
    pred[neg] = -pred[neg]
    gt[rng.uniform(size=BIG) < 0.05] = 0.0
    mask = rng.uniform(size=BIG) > 0.2
    return pred, gt, mask


@pytest.fixture(scope="module")
def big():
    return _big_input()


@pytest.fixture(scope="module")
def big_host(big):
    """The host mirror's answers on the frame-size input, computed once per mode and shared."""
    cache = {}

    def get(mode, **kw):
        key = (mode, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = _host(*big, mode, **kw)
            s, t = cache[key][1]
            a = _min_abs_a(big[0], big[1], s, t, (kw["pre_clip_min"], kw["pre_clip_max"]) if "pre_clip_min" in kw else None)
            print(f"frame size, {mode} {kw}: host (s, t) = ({s!r}, {t!r}), min |a| = {a:.4f}")
            assert a >= 0.1, (mode, a)          # the comparison below means something only away from a = 0
        return cache[key]
    return get


@pytest.mark.parametrize("mode", ["metric", "median", "l1"])
def test_device_equals_the_host_mirror_at_frame_size(engine, big, big_host, mode):
    """(s, t) bit-equal; with equal (s, t) the error map is byte-equal - the unfused s * p + t and the IEEE division; metrics within the
    project's frame-size bound between float64 sums and float32 means (rel 2e-4)."""
    ref, (sh, th), ref_map = big_host(mode)
    res, (s, t), emap = _dev(engine, *big, mode)
    assert (_bits(s), _bits(t)) == (_bits(sh), _bits(th))
    assert emap.tobytes() == ref_map.tobytes()
    assert int((big[0][(big[1] > 0)] * f32(s) + f32(t) <= 0).sum()) > 1000          # the a <= 0 -> 0 branch is well exercised
    for k in KEYS[:8]:
        assert res[k] == pytest.approx(ref[k], rel=2e-4), k
    assert res["valid_pixels"] == ref["valid_pixels"]
    if mode == "l1":
        assert engine.l1_info["certified"] == 1


def test_device_lstsq_is_the_double_solve_rounded_once(engine, big, big_host):
    """Device: float64 normal equations; here: numpy's float64 least squares on the same float32 values.  Two float64 solves of a system
    whose normal matrix has a condition number of a few tens agree to ~1e-9 before the single rounding: equal or adjacent float32
    values, bounded at 2 ulps.  Metrics against the host mirror (float32 solve) within rel 2e-4."""
    from unigeo_amd.harness.metrics import _lstsq_f32
    pred, gt, mask = big
    m1 = (gt > 0) & (gt < 80)
    gd = f32(1) / (gt[m1] + f32(1e-8))
    s64, t64 = _lstsq_f32(pred[m1], gd, solve_dtype=np.float64)
    A = np.stack([pred[m1].astype(np.float64), np.ones(int(m1.sum()))], 1)
    print(f"lstsq at frame size: condition number of the normal matrix {np.linalg.cond(A.T @ A):.1f}")
    ref, (sh, th), _ = big_host("lstsq")
    res, (s, t), emap = _dev(engine, pred, gt, mask, "lstsq")
    ds, dt = abs(float(f32(s)) - float(s64)) / float(np.spacing(s64)), abs(float(f32(t)) - float(t64)) / float(np.spacing(t64))
    print(f"lstsq at frame size: device (s, t) = ({float(f32(s))!r}, {float(f32(t))!r}) as float32, float64 solve ({float(s64)!r}, {float(t64)!r}), host float32 solve "
          f"({sh!r}, {th!r}); device - float64 solve = ({ds:.0f}, {dt:.0f}) ulps")
    assert ds <= 2 and dt <= 2
    for k in KEYS[:8]:
        assert res[k] == pytest.approx(ref[k], rel=2e-4), k
    assert res["valid_pixels"] == ref["valid_pixels"]


def test_device_scale_within_the_order_spread_of_the_restatement(engine, big):
    """The procedure of tests/test_depth_alignment_gpu.py: the spread is measured on the host restatement - index order and two seeded
    permutations - never on the device; the bound is 3 x the spread; two device runs are equal bit for bit."""
    from unigeo_amd.harness.metrics import _scale_l1
    pred, gt, mask = big
    m1 = (gt > 0) & (gt < 80)
    p, g = pred[m1], f32(1) / (gt[m1] + f32(1e-8))
    hosts = [_scale_l1(p, g)]
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(p.size)
        hosts.append(_scale_l1(p[perm], g[perm]))
    spread = max(abs(a - b) for a in hosts for b in hosts)
    r1 = _dev(engine, pred, gt, mask, "scale")
    r2 = _dev(engine, pred, gt, mask, "scale")
    s = r1[1][0]
    print(f"scale in disparity space at {p.size} pixels: host s {hosts}, relative order spread {spread / hosts[0]:.3e}, device s {s!r}, "
          f"device - host(index order) relative {abs(s - hosts[0]) / hosts[0]:.3e}")
    assert spread > 0
    assert abs(s - hosts[0]) <= 3.0 * spread
    assert r1[:2] == r2[:2] and r1[2].tobytes() == r2[2].tobytes()          # the same bits twice


def test_floor_and_clips_on_the_device(engine, big, big_host):
    kw = {"disp_clip_min": 1e-3, "post_clip_max": 80.0}
    ref, (sh, th), ref_map = big_host("median", **kw)
    res, (s, t), emap = _dev(engine, *big, "median", **kw)
    plain = big_host("median")[0]
    assert ref["Abs Rel"] != plain["Abs Rel"] and res["Abs Rel"] != pytest.approx(plain["Abs Rel"], rel=1e-3)      # a <= 0 is far now, not near
    assert (_bits(s), _bits(t)) == (_bits(sh), _bits(th)) and emap.tobytes() == ref_map.tobytes()
    assert float(emap.max()) > 100.0                                                                               # 1 / 1e-3 against gt < 4, unclipped in the map
    for k in KEYS[:8]:
        assert res[k] == pytest.approx(ref[k], rel=2e-4), k
    assert res["valid_pixels"] == ref["valid_pixels"]
    # all four clips and the floor together
    ref, (sh, th), ref_map = big_host("median", disp_clip_min=0.05, **CLIPS)
    res, (s, t), emap = _dev(engine, *big, "median", disp_clip_min=0.05, **CLIPS)
    assert (_bits(s), _bits(t)) == (_bits(sh), _bits(th)) and emap.tobytes() == ref_map.tobytes()
    for k in KEYS[:8]:
        assert res[k] == pytest.approx(ref[k], rel=2e-4), k


# ------------------------------------------------------------------------------------------------- the C call itself
def _ex2(engine, pred, gt, mask, flags=0, floor=float("nan"), alignment=None, expect_ok=True):
    from unigeo_amd._lib import DepthEvalOpts2C, _f32, _ptr
    p = None if pred is None else _f32(pred)
    g = _f32(gt)
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
    o = DepthEvalOpts2C()
    engine.lib.ug_depth_eval_opts2_default(C.byref(o))
    assert o.base.alignment == 0 and o.base.max_depth == 80.0 and o.flags == 0 and np.isnan(o.disp_clip_min)
    assert all(np.isnan(getattr(o.base, f)) for f in ("pre_clip_min", "pre_clip_max", "post_clip_min", "post_clip_max"))
    o.flags, o.disp_clip_min = flags, floor
    if alignment is not None:
        o.base.alignment = alignment
    out = np.full(11, -1.0, np.float64)
    rc = engine.lib.ug_eval_depth_ex2(engine.ctx, _ptr(p), _ptr(g), _ptr(m), g.size, C.byref(o), _ptr(out), None)
    assert (rc == 0) == expect_ok, engine.lib.ug_last_error(engine.ctx).decode()
    return out, engine.lib.ug_last_error(engine.ctx).decode()


def _ex(engine, pred, gt, mask, alignment=0):
    from unigeo_amd._lib import DepthEvalOptsC, _f32, _ptr
    p, g = _f32(pred), _f32(gt)
    m = np.ascontiguousarray(mask.astype(np.uint8))
    o = DepthEvalOptsC()
    engine.lib.ug_depth_eval_opts_default(C.byref(o))
    o.alignment = alignment
    out = np.full(11, -1.0, np.float64)
    assert engine.lib.ug_eval_depth_ex(engine.ctx, _ptr(p), _ptr(g), _ptr(m), g.size, C.byref(o), _ptr(out), None) == 0
    return out


def test_without_the_flag_the_call_is_ug_eval_depth_ex(engine, big):
    for pred, gt, mask in ((G["a_pred"], G["a_gt"], G["a_mask"]), big):
        for alignment in (0, 1, 4):
            assert _ex2(engine, pred, gt, mask, alignment=alignment)[0].tobytes() == _ex(engine, pred, gt, mask, alignment).tobytes()
    # and with it, it is not
    assert _ex2(engine, *big, flags=1)[0].tobytes() != _ex(engine, *big).tobytes()


def test_errors_leave_the_context_usable():
    from unigeo_amd._lib import Engine
    eng = Engine(0, workspace_bytes=256 << 20, persist_bytes=64 << 20)          # its own context: nothing has run on it
    try:
        g = np.array([1.0, 2.0, 4.0, 0.0], f32)
        p = np.array([1.0, 0.5, 0.25, 1.0], f32)

        def still_works():
            res, st = eng.eval_depth(g, pred=p, alignment="metric", space="disparity")
            assert res["valid_pixels"] == 3 and res["Abs Rel"] == pytest.approx(0.0, abs=1e-6) and st == (1.0, 0.0)
            res, st = eng.eval_depth(g, pred=g, alignment="metric")
            assert res["Abs Rel"] == 0.0 and st == (1.0, 0.0)
        still_works()
        assert "flag" in _ex2(eng, p, g, None, flags=2, expect_ok=False)[1]                        # an unknown flag bit
        still_works()
        assert "flag" in _ex2(eng, p, g, None, flags=1 | 4, expect_ok=False)[1]
        still_works()
        for floor in (0.0, -1e-3, float("inf")):
            assert "disp_clip_min" in _ex2(eng, p, g, None, flags=1, floor=floor, expect_ok=False)[1]        # a floor <= 0 (or infinite)
            still_works()
        assert "disp_clip_min" in _ex2(eng, p, g, None, flags=0, floor=1e-3, expect_ok=False)[1]   # a floor without the flag
        still_works()
        assert "resident" in _ex2(eng, None, g, None, flags=1, expect_ok=False)[1]                 # a resident request before any run
        still_works()
        with pytest.raises(RuntimeError):
            eng.get_disparity()
        still_works()
        assert "alignment" in _ex2(eng, p, g, None, flags=1, alignment=7, expect_ok=False)[1]      # what ug_eval_depth_ex rejects
        still_works()
        with pytest.raises(ValueError):
            eng.eval_depth(g, pred=p, space="disparity", disp_clip_min=0.0)
        with pytest.raises(ValueError):
            eng.eval_depth(g, pred=p, disp_clip_min=1e-3)
        with pytest.raises(ValueError):
            eng.eval_depth(g, pred=p, space="inverse")
        still_works()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------- resident disparity
@pytest.fixture(scope="module")
def tiny_plugins():
    """Two tiny plugins on ONE engine's weights would need two loads; one plugin serves, its option toggled by the tests that need it."""
    from unigeo_amd import weights as W
    from unigeo_amd.model import DepthCrafter
    m = DepthCrafter(synthetic_weights=True, cfgs=W.tiny_cfgs(), num_inference_steps=2, workspace_bytes=3 << 30)
    assert m.return_disparity is False
    yield m
    m.pipeline.engine.close()


def test_resident_disparity(tiny_plugins):
    from unigeo_amd.synthetic import synthetic_clip
    m = tiny_plugins
    eng = m.pipeline.engine
    clip = synthetic_clip(3, 64, 64, seed=1)
    clip["_index"] = 0
    out = m.forward(clip)
    assert "pred_disps" not in out                                                  # the default forward returns no such key
    _, depth, _ = eng.get_outputs(frames=False, depth=True)
    assert out["pred_depths"].numpy().tobytes() == depth.tobytes()                  # ... and the depth it always returned
    x = eng.get_disparity()
    assert x.shape == depth.shape and x.dtype == np.float32
    assert float(x.min()) == 0.0 and float(x.max()) == 1.0
    assert (f32(1) / (x + f32(0.1))).tobytes() == depth.tobytes()                   # the depth is made from exactly this x
    assert eng.get_outputs(frames=False, depth=True)[1].tobytes() == depth.tobytes()          # asking for it left the depth alone
    rng = np.random.default_rng(0)
    gt = rng.uniform(0.5, 6.0, depth.shape).astype(f32); gt[0, :5] = 0.0
    mask = rng.uniform(size=depth.shape) > 0.2
    for mode in ("median", "lstsq", "l1"):
        a = eng.eval_depth(gt, mask, alignment=mode, space="disparity", return_error_map=True)
        b = eng.eval_depth(gt, mask, pred=x, alignment=mode, space="disparity", return_error_map=True)
        assert a[0] == b[0] and a[1] == b[1] and a[2].tobytes() == b[2].tobytes(), mode
        assert a[0]["valid_pixels"] > 0 and np.isfinite(a[0]["Abs Rel"])
        # without the flag pred=None is still the resident DEPTH
        c = eng.eval_depth(gt, mask, alignment=mode, return_error_map=True)
        d = eng.eval_depth(gt, mask, pred=depth, alignment=mode, return_error_map=True)
        assert c[0] == d[0] and c[1] == d[1] and c[2].tobytes() == d[2].tobytes() and c[0] != a[0], mode
    # the plugin's option: the same clip and seed again, now with the disparity
    m.return_disparity = True
    try:
        out2 = m.forward(clip)
    finally:
        m.return_disparity = False
    assert out2["pred_depths"].numpy().tobytes() == depth.tobytes()
    assert tuple(out2["pred_disps"].shape) == depth.shape and out2["pred_disps"].numpy().tobytes() == eng.get_disparity().tobytes() == x.tobytes()


def test_harness_loop_in_disparity_space(tiny_plugins, tmp_path):
    from unigeo_amd.harness import SyntheticGeometryDataset, evaluate
    m = tiny_plugins
    names = ["Abs Rel", "RMSE", "delta < 1.25"]
    cfg = {"root": "x", "h": 64, "w": 64, "clip_length": 3, "clip_overlap": 1,
           "eval_depth": {"metric_names": names, "space": "disparity", "depth_alignment": "lstsq"}}
    ds = SyntheticGeometryDataset(clip_length=3, clip_overlap=1, input_size=(64, 64), num_frames=5)
    dev, _ = evaluate(cfg, dataset=ds, model=m, save_dir=str(tmp_path / "d"), verbose=False, device_metrics=True)      # the plugin needs no option
    with pytest.raises(ValueError, match="return_disparity"):
        evaluate(cfg, dataset=ds, model=m, save_dir=str(tmp_path / "e"), verbose=False)
    m.return_disparity = True
    try:
        host, _ = evaluate(cfg, dataset=ds, model=m, save_dir=str(tmp_path / "h"), verbose=False)
    finally:
        m.return_disparity = False
    depth, _ = evaluate({**cfg, "eval_depth": {"metric_names": names, "depth_alignment": "lstsq"}}, dataset=ds, model=m,
                        save_dir=str(tmp_path / "z"), verbose=False, device_metrics=True)
    assert len(host) == len(dev) == len(depth) == len(ds) == 3
    for h_, d_, z_ in zip(host, dev, depth):
        for k in names:
            print(f"{h_['seq_name']} {k}: host {h_[k]:.9g} device {d_[k]:.9g} (space: depth {z_[k]:.9g})")
            assert d_[k] == pytest.approx(h_[k], rel=2e-4), k
        assert d_["valid_pixels"] == h_["valid_pixels"] and d_["Abs Rel"] != z_["Abs Rel"]
