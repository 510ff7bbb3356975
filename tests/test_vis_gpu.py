"""GPU: the visualisation panels composed on the device (ug_vis_depth_range / ug_vis_panels; k_vis_range / k_vis_panel in kernels/vis.hip,
DESIGN.md section 15) against the reference's own panels (tests/golden/vis_golden.npz), against the host mirror (harness/vis.py) at tiny
shapes and at frame size, on the resident tensors of a run, and through the harness loop.  Bytes are compared for equality, the range bit
for bit: every step is one float32 operation on both sides."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "vis_golden.npz"), allow_pickle=False)
BIG = (2, 384, 512)          # 393 216 pixels, 314 304 four-pixel groups with Wc = 96 (Wp = 1637): above the 1024 x 256 grid cap, so both kernels' grid-stride loops take a second trip


def _inputs(shape, Wc, seed):
    rng = np.random.default_rng(seed)
    T, H, W = shape
    depth = rng.uniform(0.5, 12.0, shape).astype(np.float32)
    n = rng.standard_normal((T, H, W, 3))
    normals = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    rgbs = rng.integers(0, 256, (T, H, W, 3)).astype(np.float32) / np.float32(255)
    cbar = rng.uniform(size=(H, Wc, 3)).astype(np.float32) if Wc else None
    return depth, normals, rgbs, cbar


def _same_bits(a, b):
    return np.float32(a).tobytes() == np.float32(b).tobytes()


def test_range_equals_the_fixture_bit_for_bit(engine):
    vmin, vmax = engine.vis_depth_range(G["depth"])
    assert _same_bits(vmin, G["vmin"]) and _same_bits(vmax, G["vmax"])


@pytest.mark.parametrize("with_cbar", [True, False])
@pytest.mark.parametrize("with_rgb", [True, False])
def test_panels_equal_the_reference_byte_for_byte(engine, with_rgb, with_cbar):
    got = engine.vis_panels(G["vmin"], G["vmax"], G["lut"], depth=G["depth"], normals=G["normals"], rgbs=G["rgbs"] if with_rgb else None,
                            cbar=G["cbar"] if with_cbar else None)
    want = G["panels_rgb" if with_rgb else "panels_norgb"]
    if not with_cbar:
        want = want[:, :, :want.shape[2] - 5 - G["cbar"].shape[1]]
    assert got.dtype == np.uint8 and got.shape == want.shape
    print("differing bytes:", int((got != want).sum()))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("shape,Wc", [((1, 1, 1), 0), ((1, 1, 3), 0), ((2, 5, 7), 1), ((1, 3, 64), 2)])
def test_tiny_shapes_equal_the_host_mirror(engine, shape, Wc):
    from unigeo_amd.harness import vis
    depth, normals, rgbs, cbar = _inputs(shape, Wc, 3)
    vmin, vmax = engine.vis_depth_range(depth)
    assert _same_bits(vmin, depth.min()) and _same_bits(vmax, depth.max())
    for r in (rgbs, None):
        got = engine.vis_panels(vmin, vmax, G["lut"], depth=depth, normals=normals, rgbs=r, cbar=cbar)
        want = vis.panels_u8(depth, normals, vmin, vmax, G["lut"], rgbs=r, cbar=cbar)
        assert got.shape == want.shape == (*shape[:2], vis.panel_width(shape[2], r is not None, cbar), 3)
        assert np.array_equal(got, want)


def test_frame_size_equals_the_host_mirror(engine):
    from unigeo_amd.harness import vis
    depth, normals, rgbs, cbar = _inputs(BIG, 96, 11)
    vmin, vmax = engine.vis_depth_range(depth)
    assert _same_bits(vmin, depth.min()) and _same_bits(vmax, depth.max())
    got = engine.vis_panels(vmin, vmax, G["lut"], depth=depth, normals=normals, rgbs=rgbs, cbar=cbar)
    want = vis.panels_u8(depth, normals, vmin, vmax, G["lut"], rgbs=rgbs, cbar=cbar)
    assert got.shape == (2, 384, 3 * 512 + 5 + 96, 3)
    print("differing bytes:", int((got != want).sum()))
    assert np.array_equal(got, want)
    assert np.array_equal(engine.vis_panels(vmin, vmax, G["lut"], depth=depth, normals=normals), want[:, :, 512:1536])


def test_nan_depth_and_degenerate_range(engine):
    from unigeo_amd.harness import vis
    depth, normals, _, _ = _inputs((2, 5, 7), 0, 5)
    clean = depth.copy()
    depth[0, 0, 0] = depth[1, 4, 6] = depth[1, 2, 3] = np.nan
    depth[0, 0, 1], depth[1, 4, 5] = 0.25, 13.0                                     # the extremes sit next to NaN pixels
    vmin, vmax = engine.vis_depth_range(depth)
    assert _same_bits(vmin, 0.25) and _same_bits(vmax, 13.0)                        # NaN pixels are ignored by the range
    got = engine.vis_panels(vmin, vmax, G["lut"], depth=depth, normals=normals)
    assert np.array_equal(got, vis.panels_u8(depth, normals, vmin, vmax, G["lut"]))
    sec = got[:, :, 7:]
    assert not sec[0, 0, 0].any() and not sec[1, 4, 6].any() and not sec[1, 2, 3].any()      # NaN depth is black
    assert sec.reshape(-1, 3).any(axis=1).sum() == depth.size - 3                    # and nothing else is (no Spectral_r entry is 0,0,0)
    nan = np.full((1, 2, 3), np.nan, np.float32)
    assert engine.vis_depth_range(nan) == (0.0, 0.0) and engine.vis_depth_range(np.zeros((0,), np.float32)) == (0.0, 0.0)
    flat = np.full_like(clean, 2.5)
    vmin, vmax = engine.vis_depth_range(flat)
    assert vmin == vmax == 2.5
    got = engine.vis_panels(vmin, vmax, G["lut"], depth=flat, normals=normals)
    assert not got[:, :, 7:].any() and got[:, :, :7].any()                          # an all-equal depth: a black section, normals untouched
    zero = engine.vis_panels(0.0, 0.0, G["lut"], depth=np.zeros_like(clean), normals=normals)      # StableNormal's all-zero pred_depths
    assert np.array_equal(zero, got)


def test_errors_are_reported_and_the_context_stays_usable(engine):
    from unigeo_amd._lib import _ptr
    d, n, r, lut, cb = (np.ascontiguousarray(G[k]) for k in ("depth", "normals", "rgbs", "lut", "cbar"))
    T, H, W = d.shape
    Wc = cb.shape[1]
    out = np.zeros((T, H, 3 * W + 5 + Wc, 3), np.uint8)
    err = lambda: engine.lib.ug_last_error(engine.ctx).decode()

    def call(depth=d, normals=n, rgbs=r, mode=1, t=T, h=H, w=W, lut_=lut, cbar=cb, wc=Wc, out_=out):
        return engine.lib.ug_vis_panels(engine.ctx, _ptr(depth), _ptr(normals), _ptr(rgbs), mode, t, h, w, 0.9, 10.0, _ptr(lut_), _ptr(cbar), wc, _ptr(out_))

    bad = [(dict(lut_=None), "NULL"), (dict(out_=None), "NULL"), (dict(t=0), "positive"), (dict(h=0), "positive"), (dict(w=-1), "positive"),
           (dict(wc=-1), "Wc"), (dict(wc=0), "Wc"), (dict(mode=3), "rgb_mode"), (dict(mode=-1), "rgb_mode"), (dict(rgbs=None), "NULL"),
           (dict(depth=None), "resident depth"), (dict(normals=None), "resident normals"), (dict(mode=2), "resident input frames"),
           (dict(t=1, h=32768, w=10923, mode=0, cbar=None), "2^31")]
    for kw, word in bad:                                                            # H = 20 is no multiple of 64: nothing resident has this shape
        assert call(**kw) != 0, kw
        assert word in err(), (kw, err())
    assert call() == 0 and np.array_equal(out, G["panels_rgb"])                     # the context still works
    out2 = np.zeros(2, np.float32)
    rng = lambda depth, cnt, o: engine.lib.ug_vis_depth_range(engine.ctx, _ptr(depth), cnt, _ptr(o))
    assert rng(d, d.size, None) != 0 and "NULL" in err()
    assert rng(d, -1, out2) != 0 and "negative" in err()
    assert rng(None, d.size, out2) != 0 and "resident" in err()
    assert rng(d, d.size, out2) == 0 and _same_bits(out2[0], G["vmin"]) and _same_bits(out2[1], G["vmax"])


@pytest.fixture(scope="module")
def tiny_plugin():
    from unigeo_amd import weights as W
    from unigeo_amd.model import DepthCrafter
    m = DepthCrafter(synthetic_weights=True, cfgs=W.tiny_cfgs(), num_inference_steps=2, workspace_bytes=3 << 30)
    yield m
    m.pipeline.engine.close()


def test_resident_tensors_equal_the_downloaded_ones(tiny_plugin):
    from unigeo_amd.synthetic import synthetic_clip
    data = synthetic_clip(3, 64, 64, seed=1)
    frames = tiny_plugin.prepare_input(data)
    K = np.stack(data["intrinsics"], 0)
    pipe, eng = tiny_plugin.pipeline, tiny_plugin.pipeline.engine
    run = lambda normals: pipe(frames, height=64, width=64, num_inference_steps=2, window_size=3, seed=5, intrinsics=K, with_normals=normals, return_frames=False)
    res = run(True)
    vmin, vmax = eng.vis_depth_range()
    assert _same_bits(vmin, res.depth.min()) and _same_bits(vmax, res.depth.max()) and vmin < vmax
    cbar = np.random.default_rng(0).uniform(size=(64, 16, 3)).astype(np.float32)
    a = eng.vis_panels(vmin, vmax, G["lut"], rgbs="resident", cbar=cbar)
    b = eng.vis_panels(vmin, vmax, G["lut"], depth=res.depth, normals=res.normals, rgbs=frames, cbar=cbar)
    assert a.shape == (3, 64, 3 * 64 + 5 + 16, 3) and np.array_equal(a, b)
    assert np.array_equal(eng.vis_panels(vmin, vmax, G["lut"]), b[:, :, 64:192])    # no rgb, no colour bar
    assert len(np.unique(a[:, :, 128:192].reshape(-1, 3), axis=0)) > 8               # a real picture, not one colour
    res = run(False)
    with pytest.raises(RuntimeError, match="resident normals"):                     # the last run computed none
        eng.vis_panels(vmin, vmax, G["lut"])
    with pytest.raises(RuntimeError, match="resident depth"):                       # another shape than the resident depth's
        eng.vis_panels(vmin, vmax, G["lut"], normals=G["normals"])
    c = eng.vis_panels(vmin, vmax, G["lut"], normals=np.zeros((3, 64, 64, 3), np.float32), rgbs="resident")      # the context still works
    assert np.array_equal(c[:, :, :64], b[:, :, :64]) and (c[:, :, 64:128] == 127).all()


def test_harness_device_panels_equal_the_host_panels(tiny_plugin, tmp_path, monkeypatch):
    from unigeo_amd.harness import SyntheticGeometryDataset, evaluate
    from unigeo_amd.harness import eval as harness_eval
    seen = []
    real = harness_eval.save_depth_normal_maps

    def capture(*a, **kw):
        seen.append((kw.get("engine") is not None, real(*a, **kw)))
        return seen[-1][1]
    monkeypatch.setattr(harness_eval, "save_depth_normal_maps", capture)
    cfg = {"root": "x", "h": 64, "w": 64, "clip_length": 3, "clip_overlap": 1, "vis_depth": True,
           "eval_depth": {"metric_names": ["Abs Rel"]}, "eval_normal": {"metric_names": ["normal mean"]}}
    ds = SyntheticGeometryDataset(clip_length=3, clip_overlap=1, input_size=(64, 64), num_frames=5)
    host, _ = evaluate(cfg, dataset=ds, model=tiny_plugin, save_dir=str(tmp_path / "h"), verbose=False)
    dev, _ = evaluate(cfg, dataset=ds, model=tiny_plugin, save_dir=str(tmp_path / "d"), verbose=False, device_metrics=True)
    n = len(host)
    assert n == len(dev) >= 2 and [s[0] for s in seen] == [False] * n + [True] * n
    for k in range(n):
        assert seen[k][1].shape == seen[n + k][1].shape and seen[k][1].shape[:2] == (3, 64)
        assert np.array_equal(seen[k][1], seen[n + k][1])
        assert len(os.listdir(tmp_path / "d" / f"depth_{dev[k]['seq_name']}")) == 3
