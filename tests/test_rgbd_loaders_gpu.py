"""GPU: the two switches of ``ug_prep_gt_ex`` (UG_PREP_DEPTH_F64, UG_PREP_ZOOMED), ``ug_prep_gt`` as a call into it, ``prep="device"`` of the
five RGB-D loaders against ``prep="host"``, ``evaluate()`` end to end and the error paths.  The host loaders themselves
are pinned to the reference on the CPU in tests/test_rgbd_loaders_cpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

from unigeo_amd._lib import PREP_DEPTH_F64, PREP_ZOOMED
from unigeo_amd.harness import rgbd
from unigeo_amd.harness.scannetpp import ScannetPPSequence, _backproject_gl, resize_pick, resize_restated
from unigeo_amd.harness.scannetpp import decode_clip as decode_scannetpp

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
SCENES = os.path.join(G, "rgbd_scenes")
SCENE = {"7scenes": "chess/seq-03", "bonn": "rgbd_bonn_balloon2", "neuralrgbd": "breakfast_room", "replica": "room_0", "scannetv2": "scene0707_00"}
LAYOUTS = sorted(SCENE)
CLIP = dict(clip_length=3, clip_overlap=0)
GT = ("cam_coord", "world_coord", "mask")


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _world_bound(M, v, with_t):
    """5 * 2^-24 * (sum_j |M_ij v_j| + |t_i|) per element, in float64: the forward error of the host's float32 three-term product-and-add
    plus the device's one rounding.  v: [T,3,h,w]."""
    A = np.abs(M[:, :3, :3].astype(np.float64))
    b = np.einsum("tij,tjhw->tihw", A, np.abs(v.astype(np.float64)))
    if with_t:
        b = b + np.abs(M[:, :3, 3].astype(np.float64))[:, :, None, None]
    return 5 * 2.0 ** -24 * b


def _check_gt(dev, host, M, what=""):
    """dev, host: (cam_coord, world_coord, mask).  cam_coord and mask bit for bit, world_coord within the forward-error bound."""
    cc, wc, mask = dev
    hc, hwc, hmask = (np.ascontiguousarray(x) for x in host)
    for name, a, b in (("cam_coord", cc, hc), ("mask", mask, hmask)):
        assert a.dtype == np.float32 and a.shape == b.shape, (what, name)
        assert np.array_equal(_bits(a), _bits(b)), (what, name)
    bound = np.where(hmask[:, None] > 0, _world_bound(M, hc, True), 0.0)                         # masked pixels: exactly 0
    err = np.abs(wc.astype(np.float64) - hwc.astype(np.float64))
    print(f"{what} world_coord: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert wc.dtype == np.float32 and wc.shape == hwc.shape and (err <= bound).all(), what


def _dataset(L, **kw):
    return rgbd.LAYOUTS[L](os.path.join(SCENES, L), scenes=[SCENE[L]], **CLIP, **kw)


def _clip(L, ci):
    """Decoded files and cameras of clip ``ci``: frames, depth, view 0's intrinsics per frame, source camera -> key view."""
    root = os.path.join(SCENES, L)
    seq = rgbd.RGBDSequence(root, SCENE[L], rgbd.LAYOUTS[L].layout, **CLIP)
    ids = list(seq.clips.values())[ci]
    frames, depth = rgbd.decode_clip(root, seq, ids)
    ext = [np.asarray(seq.extrinsics[i]).astype(np.float32) for i in ids]
    K0 = np.broadcast_to(np.asarray(seq.intrinsics[ids[0]]).astype(np.float32), (len(ids), 3, 3))
    M = np.stack([ext[0] @ np.linalg.inv(e) for e in ext]).astype(np.float32)
    return frames, depth, K0, M


@pytest.fixture(scope="module")
def host_native():
    """layout -> the two clips at native size with prep="host"; read-only."""
    return {L: [_dataset(L)[ci] for ci in range(2)] for L in LAYOUTS}


def _raw_ex(engine, depth, K, M, rows, cols, flags, divisor=1000.0, max_depth=20.0, normals=None, fn="ug_prep_gt_ex", null=()):
    """ug_prep_gt_ex / ug_prep_gt through raw ctypes -> (return code, the five outputs)."""
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    T, hi, wi = depth.shape
    depth, k, m = np.ascontiguousarray(depth), np.ascontiguousarray(K, dtype=np.float32), np.ascontiguousarray(M, dtype=np.float32)
    rows, cols = np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(cols, dtype=np.int32)
    out = {n: np.zeros((T, 3, rows.size, cols.size), np.float32) for n in ("cam_normal", "cam_coord", "world_normal", "world_coord")}
    out["mask"] = np.zeros((T, rows.size, cols.size), np.float32)
    ptr = {n: (None if n in null else p(a)) for n, a in out.items()}
    args = [engine.ctx, p(depth), divisor, p(normals), p(k), p(m), T, hi, wi, p(rows), rows.size, p(cols), cols.size, max_depth,
            ptr["cam_normal"], ptr["cam_coord"], ptr["world_normal"], ptr["world_coord"], ptr["mask"]]
    rc = getattr(engine.lib, fn)(*(args + ([flags] if fn == "ug_prep_gt_ex" else [])))
    return rc, out


# ---------------------------------------------------------------------------------------------------------------- the two switches
def test_depth_f64_flag_matches_the_bonn_host_loader(engine, host_native):
    _, depth, K0, M = _clip("bonn", 0)
    depth, K0, M = depth[:2], K0[:2], M[:2]
    assert depth.shape == (2, 24, 32) and K0[0, 0, 0] == np.float32(542.822841)
    host = [np.stack(host_native["bonn"][0][k][:2]) for k in GT]
    rows, cols = np.arange(24, dtype=np.int32), np.arange(32, dtype=np.int32)
    _, cc, _, wc, mask = engine.prep_gt(depth, None, K0, M, rows, cols, depth_divisor=5000.0, max_depth=20.0, depth_f64=True)
    _check_gt((cc, wc, mask), host, M, "UG_PREP_DEPTH_F64")
    assert mask[:, 5, 5].max() == 0 and not _bits(cc[:, :, 5, 5]).any()                          # raw 0: masked, +0
    rc, raw = _raw_ex(engine, depth, K0, M, rows, cols, PREP_DEPTH_F64, divisor=5000.0)
    assert rc == 0 and all(np.array_equal(_bits(raw[k]), _bits(a)) for k, a in (("cam_coord", cc), ("world_coord", wc), ("mask", mask)))
    _, c32, _, _, m32 = engine.prep_gt(depth, None, K0, M, rows, cols, depth_divisor=5000.0, max_depth=20.0)
    valid = host[2] > 0
    n = int((c32[:, 0][valid] != host[0][:, 0][valid]).sum())
    print(f"flags = 0: x differs from the host in {n} of {int(valid.sum())} valid pixels")
    assert n >= 1 and np.array_equal(m32, host[2]) and np.array_equal(c32[:, 2], host[0][:, 2])


def test_zoomed_flag_decides_the_sign_of_zero(engine):
    """Crop tables (rows 4..19 of 24, columns 4..27 of 32) change the size without a zoom: without the flag the y of the principal row is -0,
    as the host's slicing keeps it; with the flag it is +0; nothing else changes."""
    _, depth, _, M = _clip("7scenes", 0)
    K = np.broadcast_to(np.float32([[40, 0, 16.5], [0, 40, 8], [0, 0, 1]]), (3, 3, 3))          # integer cy = 8: source row 8 = output row 4
    rows, cols = 4 + np.arange(16, dtype=np.int32), 4 + np.arange(24, dtype=np.int32)
    plain = engine.prep_gt(depth, None, K, M, rows, cols, max_depth=20.0, zoomed=False)
    zoom = engine.prep_gt(depth, None, K, M, rows, cols, max_depth=20.0, zoomed=True)
    by_size = engine.prep_gt(depth, None, K, M, rows, cols, max_depth=20.0)                      # zoomed=None: the size rule of ug_prep_gt
    mask = plain[4]
    row = mask[:, 4] > 0
    assert row.sum() >= 3 * 24 - 3
    assert not plain[1][:, 1, 4].any() and np.signbit(plain[1][:, 1, 4][row]).all()               # -0 on valid pixels
    assert not np.signbit(plain[1][:, 1, 4][~row]).any()                                         # masked pixels are +0 either way
    assert not _bits(zoom[1][:, 1, 4]).any()                                                     # +0
    other = np.ones(plain[1].shape, bool)
    other[:, 1, 4] = False
    assert np.array_equal(_bits(plain[1])[other], _bits(zoom[1])[other])
    for k in (0, 2, 3, 4):
        assert np.array_equal(_bits(plain[k]), _bits(zoom[k])), k
    for k in range(5):
        assert np.array_equal(_bits(by_size[k]), _bits(zoom[k])), k
    host = np.stack([_backproject_gl(d.astype(np.float32) / 1000, K[0]) for d in depth])[:, :, 4:20, 4:28]      # the host's crop: a slice
    d = -host[:, 2]
    host[np.broadcast_to(((d < 1e-3) | (d > 20))[:, None], host.shape)] = 0
    assert np.array_equal(_bits(plain[1]), _bits(host))


def test_ug_prep_gt_is_ug_prep_gt_ex_with_the_size_rule(engine):
    root = os.path.join(G, "scannetpp_scene")
    seq = ScannetPPSequence(root, "sceneA", clip_length=3, clip_overlap=1)
    ids = list(seq.clips.values())[0]
    _, normals, depth = decode_scannetpp(root, seq, ids)
    ext = [seq.extrinsics[i].astype(np.float32) for i in ids]
    K0 = np.broadcast_to(seq.intrinsics[ids[0]].astype(np.float32), (3, 3, 3))
    M = np.stack([ext[0] @ np.linalg.inv(e) for e in ext]).astype(np.float32)
    for size, flags in ((None, 0), ((12, 16), PREP_ZOOMED), ((7, 9), PREP_ZOOMED)):
        th, tw = size or (24, 32)
        rows, cols = resize_pick(24, th), resize_pick(32, tw)
        rc0, old = _raw_ex(engine, depth, K0, M, rows, cols, None, max_depth=80.0, normals=normals, fn="ug_prep_gt")
        rc1, new = _raw_ex(engine, depth, K0, M, rows, cols, flags, max_depth=80.0, normals=normals)
        assert rc0 == 0 and rc1 == 0
        for k in old:
            assert old[k].any() and np.array_equal(_bits(old[k]), _bits(new[k])), (size, k)
        if size is None:                                                                         # cy = 12: the scene has the -0 the rule is about
            assert np.signbit(old["cam_coord"][:, 1, 12][old["mask"][:, 12] > 0]).all()
        if size == (7, 9):
            assert 12 in rows and not np.signbit(old["cam_coord"][:, 1, list(rows).index(12)]).any()


# ---------------------------------------------------------------------------------------------------------------- the datasets
@pytest.mark.parametrize("resized", [False, True], ids=["native", "resized"])
@pytest.mark.parametrize("L", LAYOUTS)
def test_device_prep_matches_host_prep(engine, host_native, L, resized):
    size = None if not resized else ((48, 64) if L == "scannetv2" else (12, 16))
    host = _dataset(L, input_size=size, target_size=size) if resized else None
    dev = _dataset(L, input_size=size, target_size=size, prep="device", engine=engine)
    assert len(dev) == 2
    for ci in range(2):
        h, d = (host[ci] if resized else host_native[L][ci]), dev[ci]
        assert list(h.keys()) == list(d.keys())
        for k in h:
            if isinstance(h[k], list) and isinstance(h[k][0], np.ndarray):
                assert isinstance(d[k], list) and len(d[k]) == len(h[k]), k
                assert all(a.dtype == b.dtype and a.shape == b.shape for a, b in zip(d[k], h[k])), k
            else:
                assert d[k] == h[k], k
        for k in ("intrinsics", "extrinsics"):
            np.testing.assert_array_equal(np.stack(d[k]), np.stack(h[k]), err_msg=k)
        frames, _, _, M = _clip(L, ci)                                                           # ScanNetv2: after the Pillow pre-resize
        x1, y1, x2, y2 = rgbd._crop_box(dev.layout, *frames.shape[1:3])
        src = frames.transpose(0, 3, 1, 2)[:, :, y1:y2, x1:x2]
        img_d, img_h = np.stack(d["images"]), np.stack(h["images"])
        if not resized:
            assert np.array_equal(img_d, img_h) and np.array_equal(img_d, src.astype(np.float32))
            assert (x2 - x1, y2 - y1) == ((32, 24) if L != "scannetv2" else (640, 480))
        else:
            ref = resize_restated(src, *size)
            img_d, img_h = img_d.astype(np.float64), img_h.astype(np.float64)
            assert (np.abs(img_d - ref) <= _ulp32(ref)).all()
            host_err = np.abs(img_h - ref).max()
            print(f"{L} clip {ci}: max |_resize(float32) - restated| = {host_err:.3e}, max |device - _resize(float32)| = {np.abs(img_d - img_h).max():.3e}")
            assert np.abs(img_d - img_h).max() <= 2 * host_err
        _check_gt([np.stack(d[k]) for k in GT], [np.stack(h[k]) for k in GT], M, f"{L} clip {ci}")
    assert set(dev.last_timing) == {"decode", "resize", "gt"}


def test_evaluate_rows_do_not_depend_on_prep(tmp_path):
    """``prep: device`` in the YAML-shaped config on the Replica fixture (the crop): evaluate() builds the dataset, which brings its own engine."""
    import torch
    from unigeo_amd.harness import evaluate

    class Stub:
        def forward(self, data):
            d = np.stack([-np.asarray(c)[2] for c in data["cam_coord"]], 0)
            return {"pred_depths": torch.from_numpy(2.0 * d + 0.5).float(), "pred_normals": torch.zeros(d.shape + (3,))}

    cfg = {"dataset": "replicaDataset", "root": os.path.join(SCENES, "replica"), "scenes": [SCENE["replica"]], "h": 12, "w": 16, "clip_length": 3,
           "clip_overlap": 0, "split": "test", "model_name": "DepthCrafter", "model_params": {},
           "eval_depth": {"metric_names": ["Abs Rel", "delta < 1.25"], "depth_alignment": "lstsq"}}
    rows = {}
    for prep in ("host", "device"):
        rows[prep], _ = evaluate(dict(cfg, prep=prep), model=Stub(), save_dir=str(tmp_path / prep), verbose=False)
        assert os.path.isfile(tmp_path / prep / "metrics.csv")
    assert [r["seq_name"] for r in rows["device"]] == [r["seq_name"] for r in rows["host"]] == ["000_room_0", "001_room_0"]
    for rd, rh in zip(rows["device"], rows["host"]):
        assert rd.keys() == rh.keys()
        for k in rh:
            if k != "seq_name":
                assert abs(rd[k] - rh[k]) <= 1e-6, (k, rd[k], rh[k])


# ---------------------------------------------------------------------------------------------------------------- error paths
def test_errors_leave_the_engine_usable(engine, host_native):
    _, depth, K0, M = _clip("7scenes", 0)
    rows, cols = np.arange(24, dtype=np.int32), np.arange(32, dtype=np.int32)
    host = [np.stack(host_native["7scenes"][0][k]) for k in GT]

    def valid_call():
        rc, out = _raw_ex(engine, depth, K0, M, rows, cols, 0)
        assert rc == 0
        _check_gt([out[k] for k in GT], host, M, "after an error")

    rc, out = _raw_ex(engine, depth, K0, M, rows, cols, 4 | PREP_ZOOMED)
    assert rc != 0 and b"0x4" in engine.lib.ug_last_error(engine.ctx) and not out["mask"].any()   # the bit is named; nothing was written
    valid_call()
    rc, _ = _raw_ex(engine, depth, K0, M, rows, cols, 0, null=("cam_coord",))
    assert rc != 0 and b"NULL" in engine.lib.ug_last_error(engine.ctx)
    valid_call()
