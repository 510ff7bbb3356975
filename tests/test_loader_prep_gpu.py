"""GPU: ``prep="device"`` of the ScanNet++ loader - ``ug_prep_resize_frames`` against the float64 restatement of the
host resize and against ``_resize`` itself, ``ug_prep_gt`` against ``load_clip`` + the order-0 resize and the reference's golden, the
dataset and ``evaluate()`` end to end, and the error paths.  The tables themselves are pinned on the CPU in tests/test_loader_prep_cpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

from unigeo_amd.harness.scannetpp import (ScannetPPDataset, ScannetPPSequence, _backproject_gl, _resize, decode_clip, resize_pick,
                                          resize_restated, resize_taps)

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.join(G, "scannetpp_scene")
DS = dict(scenes=["sceneA"], clip_length=3, clip_overlap=1)

# (T, Hi, Wi, Ho, Wo): one pixel; plain; ragged; up-scaling (no filter, mirrored zoom taps at the border); one axis untouched; radius 4;
# gaussian radius >= axis length (the ones tests/test_loader_prep_cpu.py confirms against scipy)
SMALL = [(1, 1, 1, 1, 1), (2, 24, 32, 12, 16), (1, 37, 53, 12, 16), (2, 20, 28, 24, 40), (1, 64, 96, 64, 32), (3, 146, 219, 48, 64),
         (1, 5, 7, 1, 2), (2, 3, 64, 2, 5), (1, 2, 2, 1, 1)]


def _frames(T, hi, wi, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (T, hi, wi, 3), dtype=np.uint8)


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _check_resize(engine, T, hi, wi, ho, wo):
    f = _frames(T, hi, wi, seed=hi * 7 + wi)
    got = engine.prep_resize_frames(f, ho, wo)
    assert got.dtype == np.float32 and got.shape == (T, 3, ho, wo)
    ref = resize_restated(f.transpose(0, 3, 1, 2), ho, wo)
    err = np.abs(got.astype(np.float64) - ref) / _ulp32(ref)
    print(f"{(T, hi, wi, ho, wo)}: max |device - restated| = {err.max():.3f} float32 ulp")
    assert err.max() <= 1.0
    return f, got, ref


@pytest.mark.parametrize("T,hi,wi,ho,wo", SMALL)
def test_resize_frames_within_one_ulp_of_the_restatement(engine, T, hi, wi, ho, wo):
    _check_resize(engine, T, hi, wi, ho, wo)


def test_resize_frames_at_the_real_scale_and_against_the_host_resize(engine):
    """2 x 1168 x 1752 -> 384 x 512: both passes have more outputs than the capped grid has threads, so every grid-stride loop makes a
    second trip; also against ``_resize`` on float32 input, the host loader's own arithmetic."""
    f, got, ref = _check_resize(engine, 2, 1168, 1752, 384, 512)
    host = _resize(f.transpose(0, 3, 1, 2).astype(np.float32), 384, 512, 1, True)
    assert host.dtype == np.float32
    host_err = np.abs(host.astype(np.float64) - ref).max()
    dev_err = np.abs(got.astype(np.float64) - host.astype(np.float64)).max()
    print(f"max |_resize(float32) - restated| = {host_err:.3e}; max |device - _resize(float32)| = {dev_err:.3e}")
    print(f"outputs that differ after truncation to uint8: {int((got.astype(np.uint8) != host.astype(np.uint8)).sum())} of {got.size}")
    assert dev_err <= 2 * host_err


# ---------------------------------------------------------------------------------------------------------------- ground truth
def _clip_inputs(ci):
    """What the loader hands ug_prep_gt for clip ``ci`` of the golden scene: decoded files, view 0's intrinsics, source camera -> key view."""
    seq = ScannetPPSequence(ROOT, "sceneA", clip_length=3, clip_overlap=1)
    ids = list(seq.clips.values())[ci]
    frames, normals, depth = decode_clip(ROOT, seq, ids)
    ext = [seq.extrinsics[i].astype(np.float32) for i in ids]
    K0 = np.broadcast_to(seq.intrinsics[ids[0]].astype(np.float32), (len(ids), 3, 3))
    M = np.stack([ext[0] @ np.linalg.inv(e) for e in ext]).astype(np.float32)
    return frames, normals, depth, K0, M


def _host_gt(depth_u16, normals_u8, K0, M, max_depth=80):
    """``load_clip``'s per-frame arithmetic on decoded arrays, with the depth bound as a parameter (``load_clip`` has 80 built in);
    test_host_gt_mirror_is_load_clip pins it to ``load_clip`` itself."""
    out = [[], [], [], [], []]
    for j in range(len(depth_u16)):
        raw = normals_u8[j].astype(np.float32)
        hole = np.all(raw < 1e-3, axis=2)
        n = raw / 255.0 * 2 - 1
        n[hole] = 0
        n = n.astype(np.float32).transpose(2, 0, 1)
        c = _backproject_gl(depth_u16[j].astype(np.float32) / 1000, K0[j])
        wn = (M[j][:3, :3] @ n.reshape(3, -1)).reshape(n.shape)
        wc = (M[j][:3, :3] @ c.reshape(3, -1) + M[j][:3, 3][:, None]).reshape(c.shape)
        d = -1 * c[2]
        bad = np.isnan(n).any(0) | np.isnan(c).any(0) | (d < 1e-3) | (d > max_depth)
        for a in (n, c, wn, wc):
            a[:, bad] = 0
        for lst, a in zip(out, (n, c, wn, wc, (~bad).astype(np.float32))):
            lst.append(a)
    return [np.stack(a) for a in out]


def _world_bound(M, v, with_t):
    """5 * 2^-24 * (sum_j |M_ij v_j| + |t_i|) per element, in float64: the forward error of the host's float32 three-term product-and-add
    plus the device's one rounding.  v: [T,3,h,w]."""
    A = np.abs(M[:, :3, :3].astype(np.float64))
    b = np.einsum("tij,tjhw->tihw", A, np.abs(v.astype(np.float64)))
    if with_t:
        b = b + np.abs(M[:, :3, 3].astype(np.float64))[:, :, None, None]
    return 5 * 2.0 ** -24 * b


def _check_gt(dev, host, M):
    cn, cc, wn, wc, mask = dev
    hn, hc, hwn, hwc, hmask = host
    for name, a, b in (("cam_normal", cn, hn), ("cam_coord", cc, hc), ("mask", mask, hmask)):
        assert a.dtype == np.float32 and a.shape == b.shape, name
        assert np.array_equal(a.view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), name            # bit for bit
    valid = hmask[:, None] > 0
    for name, a, b, v, with_t in (("world_normal", wn, hwn, hn, False), ("world_coord", wc, hwc, hc, True)):
        bound = np.where(valid, _world_bound(M, v, with_t), 0.0)                                          # masked pixels: exactly 0
        err = np.abs(a.astype(np.float64) - b.astype(np.float64))
        print(f"{name}: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert a.dtype == np.float32 and a.shape == b.shape and (err <= bound).all(), name


@pytest.fixture(scope="module")
def host_native():
    ds = ScannetPPDataset(ROOT, **DS)
    return [ds[0], ds[1]]


def _host_sample_gt(sample, size=None):
    keys = ("cam_normal", "cam_coord", "world_normal", "world_coord", "mask")
    if size is None:
        return [np.stack(sample[k]) for k in keys]
    return [np.stack([_resize(x, size[0], size[1], 0, False) for x in sample[k]]) for k in keys]


def test_host_gt_mirror_is_load_clip(host_native):
    """CPU-only check of this file's own reference: the mirror with a depth bound equals ``load_clip`` at 80."""
    _, normals, depth, K0, M = _clip_inputs(0)
    for a, b in zip(_host_gt(depth, normals, K0, M), _host_sample_gt(host_native[0])):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("size", [None, (12, 16), (7, 9), (30, 40)])
def test_gt_matches_the_host_loader(engine, host_native, size):
    for ci in range(2):
        _, normals, depth, K0, M = _clip_inputs(ci)
        hi, wi = depth.shape[1:]
        th, tw = size or (hi, wi)
        dev = engine.prep_gt(depth, normals, K0, M, resize_pick(hi, th), resize_pick(wi, tw))
        assert dev[0].shape == (len(depth), 3, th, tw) and dev[4].shape == (len(depth), th, tw)
        _check_gt(dev, _host_sample_gt(host_native[ci], size), M)


def test_gt_matches_the_reference_golden_at_native_size(engine):
    gold = np.load(os.path.join(G, "scannetpp_golden.npz"))
    for ci in range(2):
        _, normals, depth, K0, M = _clip_inputs(ci)
        cn, cc, wn, wc, mask = engine.prep_gt(depth, normals, K0, M, resize_pick(24, 24), resize_pick(32, 32))
        for k, a in (("cam_normal", cn), ("cam_coord", cc), ("mask", mask)):
            np.testing.assert_array_equal(a, gold[f"c{ci}_{k}"], err_msg=k)
        for k, a in (("world_normal", wn), ("world_coord", wc)):
            np.testing.assert_allclose(a, gold[f"c{ci}_{k}"], rtol=0, atol=1e-5, err_msg=k)
    assert mask[:, 5, 5].max() == 0 and mask[:, 6, 6].min() == 1                     # the scene's depth-0 pixel and its 65 m pixel


@pytest.mark.parametrize("size", [None, (7, 9)])
def test_gt_zero_normal_pixel_and_depth_bound(engine, size):
    """A normal map with an all-zero pixel (invalid normal on a valid depth: zero normals, mask stays 1) and max_depth = 60, which masks
    the scene's 65 m pixel; without normals the normal outputs are 0 and the rest is unchanged."""
    _, normals, depth, K0, M = _clip_inputs(0)
    normals = normals.copy()
    normals[:, 3, 4] = 0
    normals[:, 8, 8] = 0                                                             # a source pixel the 7 x 9 target keeps
    assert 8 in resize_pick(24, 7) and 8 in resize_pick(32, 9)
    assert depth[0, 6, 6] > 60000 and depth[0, 3, 4] > 0
    th, tw = size or (24, 32)
    ri, ci = resize_pick(24, th), resize_pick(32, tw)
    host = [np.stack([_resize(x, th, tw, 0, False) for x in a]) for a in _host_gt(depth, normals, K0, M, max_depth=60)]
    dev = engine.prep_gt(depth, normals, K0, M, ri, ci, max_depth=60.0)
    _check_gt(dev, host, M)
    if size is None:
        assert dev[4][0, 6, 6] == 0 and dev[4][0, 3, 4] == 1 and not dev[0][0, :, 3, 4].any() and not dev[2][0, :, 3, 4].any()
        assert engine.prep_gt(depth, normals, K0, M, ri, ci, max_depth=80.0)[4][0, 6, 6] == 1
    bare = engine.prep_gt(depth, None, K0, M, ri, ci, max_depth=60.0)
    assert not bare[0].any() and not bare[2].any()
    for k in (1, 3, 4):
        np.testing.assert_array_equal(bare[k], dev[k])


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_dataset_device_prep_matches_host_prep(engine):
    size = (12, 16)
    host = ScannetPPDataset(ROOT, input_size=size, target_size=size, **DS)
    dev = ScannetPPDataset(ROOT, input_size=size, target_size=size, prep="device", engine=engine, **DS)
    assert len(dev) == len(host) == 2
    for ci in range(2):
        h, d = host[ci], dev[ci]
        assert list(h.keys()) == list(d.keys())
        frames, _, _, _, M = _clip_inputs(ci)
        for k in h:
            if isinstance(h[k], list) and isinstance(h[k][0], np.ndarray):
                assert isinstance(d[k], list) and len(d[k]) == len(h[k]), k
                assert all(a.dtype == b.dtype and a.shape == b.shape for a, b in zip(d[k], h[k])), k
            else:
                assert d[k] == h[k], k
        for k in ("intrinsics", "extrinsics"):                                       # stay on the host: the same arithmetic
            np.testing.assert_array_equal(np.stack(d[k]), np.stack(h[k]), err_msg=k)
        ref = resize_restated(frames.transpose(0, 3, 1, 2), *size)
        img_d, img_h = np.stack(d["images"]).astype(np.float64), np.stack(h["images"]).astype(np.float64)
        assert (np.abs(img_d - ref) <= _ulp32(ref)).all()
        host_err = np.abs(img_h - ref).max()
        print(f"clip {ci}: max |_resize(float32) - restated| = {host_err:.3e}, max |device - _resize(float32)| = {np.abs(img_d - img_h).max():.3e}")
        assert np.abs(img_d - img_h).max() <= 2 * host_err
        keys = ("cam_normal", "cam_coord", "world_normal", "world_coord", "mask")
        _check_gt([np.stack(d[k]) for k in keys], [np.stack(h[k]) for k in keys], M)
    assert set(dev.last_timing) == {"decode", "resize", "gt"}


def test_dataset_device_prep_without_a_resize(engine, host_native):
    """input_size = target_size = None still goes through the device calls, with identity tables: the images are the bytes as float32."""
    dev = ScannetPPDataset(ROOT, prep="device", engine=engine, **DS)
    for ci in range(2):
        d = dev[ci]
        np.testing.assert_array_equal(np.stack(d["images"]), np.stack(host_native[ci]["images"]))
        np.testing.assert_array_equal(np.stack(d["intrinsics"]), np.stack(host_native[ci]["intrinsics"]))
        keys = ("cam_normal", "cam_coord", "world_normal", "world_coord", "mask")
        _check_gt([np.stack(d[k]) for k in keys], [np.stack(host_native[ci][k]) for k in keys], _clip_inputs(ci)[4])


def test_evaluate_rows_do_not_depend_on_prep(tmp_path):
    """``prep: device`` in the YAML-shaped config: evaluate() builds the dataset, which brings its own weight-less engine."""
    import torch
    from unigeo_amd.harness import evaluate

    class GT:
        def forward(self, data):
            d = np.stack([-np.asarray(c)[2] for c in data["cam_coord"]], 0)
            n = np.stack([np.asarray(c).transpose(1, 2, 0) for c in data["cam_normal"]], 0)
            return {"pred_depths": torch.from_numpy(2.0 * d + 0.5).float(), "pred_normals": torch.from_numpy(n).float()}

    cfg = {"dataset": "ScannetPPDataset", "root": ROOT, "h": 12, "w": 16, "clip_length": 3, "clip_overlap": 1, "split": "test", "scenes": "all",
           "model_name": "DepthCrafter", "model_params": {},
           "eval_depth": {"metric_names": ["Abs Rel", "delta < 1.25"], "depth_alignment": "lstsq"},
           "eval_normal": {"metric_names": ["normal mean", "angle < 11.25"]}}
    rows = {}
    for prep in ("host", "device"):
        rows[prep], _ = evaluate(dict(cfg, prep=prep), model=GT(), save_dir=str(tmp_path / prep), verbose=False)
        assert os.path.isfile(tmp_path / prep / "metrics.csv")
    assert [r["seq_name"] for r in rows["device"]] == [r["seq_name"] for r in rows["host"]] == ["000_sceneA", "001_sceneA"]
    for rd, rh in zip(rows["device"], rows["host"]):
        assert rd.keys() == rh.keys()
        for k in rh:
            if k != "seq_name":
                assert abs(rd[k] - rh[k]) <= 1e-6, (k, rd[k], rh[k])


# ---------------------------------------------------------------------------------------------------------------- error paths
def test_errors_leave_the_engine_usable(engine):
    f = _frames(2, 24, 32)
    ri, rw = resize_taps(24, 12)
    bad = ri.copy(); bad[5, 1] = 24                                                  # one past the last source row
    with pytest.raises(RuntimeError, match="outside the source"):
        engine.prep_resize_frames(f, 12, 16, row_taps=(bad, rw))
    bad[5, 1] = -1
    with pytest.raises(RuntimeError, match="outside the source"):
        engine.prep_resize_frames(f, 12, 16, row_taps=(bad, rw))
    with pytest.raises(RuntimeError, match="positive"):                              # T = 0
        engine.prep_resize_frames(f[:0], 12, 16)
    ci, cw = resize_taps(32, 16)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = engine.lib.ug_prep_resize_frames(engine.ctx, p(f), 2, 24, 32, 12, 16, p(ri), p(rw), ri.shape[1], p(ci), p(cw), ci.shape[1], None)
    assert rc != 0 and b"NULL" in engine.lib.ug_last_error(engine.ctx)

    _, normals, depth, K0, M = _clip_inputs(0)
    rows, cols = resize_pick(24, 12), resize_pick(32, 16)
    for r_, c_ in ((np.int32([0, 24]), cols), (rows, np.int32([-1, 3]))):
        with pytest.raises(RuntimeError, match="outside the source"):
            engine.prep_gt(depth, normals, K0, M, r_, c_)
    with pytest.raises(RuntimeError, match="positive"):                              # T = 0
        engine.prep_gt(depth[:0], normals[:0], K0[:0], M[:0], rows, cols)
    o3 = np.empty((3, 3, 12, 16), np.float32)
    k, m = np.ascontiguousarray(K0, dtype=np.float32), np.ascontiguousarray(M)
    rc = engine.lib.ug_prep_gt(engine.ctx, p(depth), 1000.0, p(normals), p(k), p(m), 3, 24, 32, p(rows), 12, p(cols), 16, 80.0,
                               p(o3), p(o3), p(o3), p(o3), None)                     # NULL mask; nothing is written before the check
    assert rc != 0 and b"NULL" in engine.lib.ug_last_error(engine.ctx)

    _check_resize(engine, 2, 24, 32, 12, 16)
    _check_gt(engine.prep_gt(depth, normals, K0, M, rows, cols),
              _host_sample_gt(ScannetPPDataset(ROOT, **DS)[0], (12, 16)), M)
