"""GPU: depth evaluation in global coordinates on the device (ug_eval_depth_global; k_world_radius / k_radius_metrics in kernels/metrics.hip,
DESIGN.md section 14) against the reference's own outputs (tests/golden/depth_global_golden.npz), against the host mirror
(harness.metrics.depth_evaluation_in_global_coord) at frame size and at tiny shapes, and through the harness loop.  Bounds as in
tests/test_depth_global_cpu.py; device against host mirror at frame size rel 2e-4, as the camera-coordinate tests use."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "depth_global_golden.npz"), allow_pickle=False)
KEYS = [str(k) for k in G["keys"]]
CLIPS = dict(zip(("pre_clip_min", "pre_clip_max", "post_clip_min", "post_clip_max"), (float(c) for c in G["clips"])))
METRIC_REL = max(3e-5, 2.0 * float(G["metric_distance"]))
MAP_RTOL = max(1e-5, 2.0 * float(G["map_distance"]))
BIG = (2, 384, 512)          # 393 216 pixels: above the 1024 x 256 grid cap, so every kernel's grid-stride loop takes a second trip


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * kx + (1 - np.cos(angle)) * kx @ kx


def _radius(depth, K, poses):
    T, H, W = depth.shape
    col, row = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
    z = depth.astype(np.float64)
    K, poses = K.astype(np.float64), poses.astype(np.float64)
    x = (col - K[:, None, None, 0, 2]) * z / K[:, None, None, 0, 0]
    y = (row - K[:, None, None, 1, 2]) * z / K[:, None, None, 1, 1]
    world = np.einsum("tij,thwj->thwi", poses[:, :3, :3], np.stack([x, y, z], -1)) + poses[:, None, None, :3, 3]
    return np.linalg.norm(world, axis=-1).astype(np.float32)


def _scene(shape, seed):
    """Seeded inputs with a different K and a different rotated, translated pose per frame; the world origin lies about 3 behind
    the camera (plus a per-frame offset of at most 1.5), so every ground-truth radius is at least 2."""
    rng = np.random.default_rng(seed)
    T, H, W = shape
    gt = rng.uniform(0.5, 6.0, shape).astype(np.float32)
    if gt.size > 1:
        gt[rng.uniform(size=shape) < 0.05] = 0.0
        gt[0, 0, 0] = 1.0
    pred = (0.7 * gt + 0.3 + 0.2 * rng.standard_normal(shape)).astype(np.float32) * (1.0 + 0.1 * np.arange(T, dtype=np.float32))[:, None, None]
    mask = rng.uniform(size=shape) > 0.2
    mask[0, 0, 0] = True
    f = 0.9 * max(H, W)
    K = np.stack([np.array([[f + 3 * k, 0, W / 2.0 + 0.5 * k], [0, f - 2 * k, H / 2.0 - 0.25 * k], [0, 0, 1]], np.float32) for k in range(T)], 0)
    poses = np.tile(np.eye(4, dtype=np.float32), (T, 1, 1))
    for k in range(T):
        R = _rotation((0.3 + k, 1.0, 0.2 * k), 0.25 + 0.2 * k)
        poses[k, :3, :3] = R.astype(np.float32)
        poses[k, :3, 3] = (R @ np.array([0.0, 0.0, 3.0]) + np.array([0.8 * k - 0.5, -0.6, 0.7])).astype(np.float32)
    return pred, gt, _radius(gt, K, poses), poses, K, mask


def _host(pred, gt, gr, poses, K, mask, **kw):
    from unigeo_amd.harness import depth_evaluation_in_global_coord
    return depth_evaluation_in_global_coord(pred, gt, gr, poses, K, custom_mask=mask, align_with_lstsq=True, return_fits=True, **kw)


@pytest.mark.parametrize("clip", ["noclip", "clip"])
def test_device_matches_the_reference(engine, clip):
    res, fit_r, fit_d, rmap = engine.eval_depth_global(G["gt"], G["gt_radius"], G["poses"], G["K"], G["mask"], pred=G["pred"],
                                                       return_radius_map=True, **(CLIPS if clip == "clip" else {}))
    want = G[f"{clip}_vals"]
    for k, w_ in zip(KEYS[:8], want):
        print(f"{clip} {k}: device {res[k]:.9g} reference {w_:.9g} rel {abs(res[k] - w_) / max(abs(w_), 1e-12):.3e}")
    emu = [float(v) for v in G[f"{clip}_emu_fits"]]
    print(f"{clip} (s_r, t_r) device {fit_r} emulation {emu[:2]}; (s_d, t_d) device {fit_d} emulation {emu[2:]}")
    ref = G[f"{clip}_map"]
    print(f"{clip} radius map: max rel diff {(np.abs(rmap - ref) / np.abs(ref)).max():.3e}, bit-equal on {(rmap.view(np.uint32) == ref.view(np.uint32)).sum()} of {ref.size}")
    for k, w_ in zip(KEYS[:8], want):
        assert res[k] == pytest.approx(w_, rel=METRIC_REL, abs=1e-6), k
    assert res["valid_pixels"] == int(want[8])
    assert fit_r == pytest.approx(emu[:2], rel=1e-5) and fit_d == pytest.approx(emu[2:], rel=1e-5)
    np.testing.assert_allclose(rmap, ref, rtol=MAP_RTOL, atol=1e-6)


@pytest.fixture(scope="module")
def big():
    return _scene(BIG, 11)


def _out13(engine, pred, gt, gr, poses, K, mask, want_map=True):
    from unigeo_amd._lib import DepthEvalOptsC, _f32, _ptr
    o = DepthEvalOptsC()
    engine.lib.ug_depth_eval_opts_default(C.byref(o))
    T, H, W = gt.shape
    out = np.full(13, -1.0, np.float64)
    rmap = np.full(gt.shape, -1.0, np.float32) if want_map else None
    m = np.ascontiguousarray(mask.astype(np.uint8))
    rc = engine.lib.ug_eval_depth_global(engine.ctx, _ptr(_f32(pred)), _ptr(_f32(gt)), _ptr(_f32(gr)), _ptr(_f32(poses)), _ptr(_f32(K)), _ptr(m),
                                         T, H, W, C.byref(o), _ptr(out), _ptr(rmap))
    assert rc == 0, engine.lib.ug_last_error(engine.ctx).decode()
    return out, rmap


def test_device_matches_the_host_mirror_at_frame_size_and_repeats_its_bytes(engine, big):
    pred, gt, gr, poses, K, mask = big
    assert gr[(gt > 0) & (gt < 80)].min() >= 0.3
    res, fit_r, fit_d, rmap = engine.eval_depth_global(gt, gr, poses, K, mask, pred=pred, return_radius_map=True)
    ref, ref_map, ref_r, ref_d = _host(pred, gt, gr, poses, K, mask)
    for k in KEYS[:8]:
        print(f"{BIG} {k}: device {res[k]:.9g} host {ref[k]:.9g}")
        assert res[k] == pytest.approx(ref[k], rel=2e-4), k
    assert res["valid_pixels"] == ref["valid_pixels"]
    assert fit_r == pytest.approx(ref_r, rel=2e-4) and fit_d == pytest.approx(ref_d, rel=2e-4)
    np.testing.assert_allclose(rmap, ref_map, rtol=2e-4)
    clipped, _, _ = engine.eval_depth_global(gt, gr, poses, K, mask, pred=pred, **CLIPS)
    ref_c = _host(pred, gt, gr, poses, K, mask, **CLIPS)[0]
    for k in KEYS[:8]:
        assert clipped[k] == pytest.approx(ref_c[k], rel=2e-4), k
    assert clipped["Abs Rel"] != res["Abs Rel"]
    a, b = _out13(engine, *big), _out13(engine, *big)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()          # the same bits twice
    assert a[0][0] == res["Abs Rel"] and a[1].tobytes() == rmap.tobytes()
    assert _out13(engine, *big, want_map=False)[0].tobytes() == a[0].tobytes()             # the map is optional


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 3, 5)])
def test_tiny_shapes_match_the_host_mirror(engine, shape):
    """One pixel is the rank-1 case of both fits (minimum-norm solution on either side)."""
    pred, gt, gr, poses, K, mask = _scene(shape, 5)
    res, fit_r, fit_d, rmap = engine.eval_depth_global(gt, gr, poses, K, mask, pred=pred, return_radius_map=True)
    ref, ref_map, ref_r, ref_d = _host(pred, gt, gr, poses, K, mask)
    assert res["valid_pixels"] == ref["valid_pixels"] > 0
    for k in KEYS[:8]:
        assert res[k] == pytest.approx(ref[k], rel=3e-5, abs=1e-6), k
    assert fit_r == pytest.approx(ref_r, rel=1e-5, abs=1e-6) and fit_d == pytest.approx(ref_d, rel=1e-5, abs=1e-6)
    np.testing.assert_allclose(rmap, ref_map, rtol=1e-5, atol=1e-6)


def test_no_valid_pixel_convention_on_the_device(engine):
    gt = np.zeros((2, 4, 5), np.float32)
    res, fit_r, fit_d, rmap = engine.eval_depth_global(gt, np.ones_like(gt), G["poses"][:2], G["K"][:2], np.ones(gt.shape, bool), pred=np.ones_like(gt),
                                                       return_radius_map=True, **CLIPS)
    assert res["valid_pixels"] == 0 and all(res[k] == 0 for k in KEYS[:8])
    assert fit_r == (0.0, 0.0) and fit_d == (0.0, 0.0) and not rmap.any()


def test_errors_are_reported_and_the_context_stays_usable(engine):
    from unigeo_amd._lib import DepthEvalOptsC, _ptr
    pred, gt, gr, poses, K = (np.ascontiguousarray(G[k]) for k in ("pred", "gt", "gt_radius", "poses", "K"))
    out = np.zeros(13, np.float64)
    o = DepthEvalOptsC()
    engine.lib.ug_depth_eval_opts_default(C.byref(o))
    call = lambda opts, cam, k, t=3, p=pred, r=gr: engine.lib.ug_eval_depth_global(engine.ctx, _ptr(p), _ptr(gt), _ptr(r), _ptr(cam), _ptr(k), None, t, 20, 28,
                                                                                   opts, _ptr(out), None)
    err = lambda: engine.lib.ug_last_error(engine.ctx).decode()
    o.alignment = 1                                                                 # UG_ALIGN_MEDIAN
    assert call(C.byref(o), poses, K) != 0 and "alignment" in err()
    o.alignment = 0
    assert call(C.byref(o), None, K) != 0 and "NULL" in err()
    assert call(C.byref(o), poses, None) != 0 and "NULL" in err()
    assert call(C.byref(o), poses, K, r=None) != 0 and "NULL" in err()
    assert call(None, poses, K) != 0 and "NULL" in err()
    assert call(C.byref(o), poses, K, t=0) != 0 and "positive" in err()
    res, _, _ = engine.eval_depth_global(gt, gr, poses, K, G["mask"], pred=pred)     # the context still works
    assert res["Abs Rel"] == pytest.approx(float(G["noclip_vals"][0]), rel=METRIC_REL)


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
    _, gt, gr, poses, K, mask = _scene(depth.shape, 0)
    a = eng.eval_depth_global(gt, gr, poses, K, mask, return_radius_map=True)
    b = eng.eval_depth_global(gt, gr, poses, K, mask, pred=depth, return_radius_map=True)
    assert a[:3] == b[:3] and a[3].tobytes() == b[3].tobytes()
    assert a[0]["valid_pixels"] > 0 and np.isfinite(a[0]["Abs Rel"])
    with pytest.raises(RuntimeError, match="resident"):                             # another shape than the resident depth's
        eng.eval_depth_global(gt[:2], gr[:2], poses[:2], K[:2])


def test_harness_device_metrics_in_global_coordinates(tiny_plugin, tmp_path):
    from unigeo_amd.harness import SyntheticGeometryDataset, evaluate
    cfg = {"root": "x", "h": 64, "w": 64, "clip_length": 3, "clip_overlap": 1,
           "eval_depth": {"metric_names": ["Abs Rel", "delta < 1.25"], "coord": "global"}}
    ds = SyntheticGeometryDataset(clip_length=3, clip_overlap=1, input_size=(64, 64), num_frames=5)
    host, _ = evaluate(cfg, dataset=ds, model=tiny_plugin, save_dir=str(tmp_path / "h"), verbose=False)
    dev, _ = evaluate(cfg, dataset=ds, model=tiny_plugin, save_dir=str(tmp_path / "d"), verbose=False, device_metrics=True)
    cam, _ = evaluate({**cfg, "eval_depth": {"metric_names": ["Abs Rel", "delta < 1.25"], "coord": "camera"}}, dataset=ds, model=tiny_plugin,
                      save_dir=str(tmp_path / "c"), verbose=False, device_metrics=True)
    assert len(host) == len(dev) == len(cam) == 3
    for h_, d_, c_ in zip(host, dev, cam):
        for k in ("Abs Rel", "delta < 1.25"):
            assert d_[k] == pytest.approx(h_[k], rel=2e-4), k
        assert d_["valid_pixels"] == h_["valid_pixels"] and d_["Abs Rel"] != c_["Abs Rel"]      # global, not camera coordinates
