"""GPU: ``ug_prep_gt_normals`` (kernels/gt_normals.hip) against its host mirror ``fit_normals`` + ``world_normals`` + crop
and pick, bit for bit; ``prep="device", normals="depth"`` of the RGB-D loaders against ``prep="host"``; the error paths; and ``evaluate`` with
the normal metrics on the device.  The mirror itself is pinned to the reference on the CPU in tests/test_gt_normals_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import gt_normals_fixtures as fx
from unigeo_amd._lib import PREP_DEPTH_F64, PREP_ZOOMED, GtNormalsOptsC
from unigeo_amd.harness import rgbd
from unigeo_amd.harness.normals import fit_normals, world_normals
from unigeo_amd.harness.scannetpp import _backproject_gl, _resize, resize_pick

pytestmark = pytest.mark.gpu

NORMAL_KEYS = ["normal mean", "normal median", "normal rmse", "angle < 5", "angle < 7.5", "angle < 11.25", "angle < 22.5", "angle < 30"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _cams(T, K):
    """View 0's intrinsics per frame and a different rigid source-to-key matrix per frame."""
    M = np.stack([np.linalg.inv(fx._pose(0)) @ fx._pose(i) for i in range(T)]).astype(np.float32)
    return np.broadcast_to(np.asarray(K, np.float32), (T, 3, 3)), M


def _host(raw, K, M, rows, cols, zoomed, divisor=1000.0, depth_f64=False, max_depth=20.0, **opts):
    """The mirror on every full native frame, then the pick; with ``zoomed`` through the host's order-0 ``_resize`` when the tables are a
    plain zoom (checked against the pick), which is where a -0 turns into +0."""
    cn, wn, nm = [], [], []
    K32 = np.asarray(K, np.float32)
    for t in range(raw.shape[0]):
        if depth_f64:
            c = _backproject_gl(rgbd.depth_metres(raw[t], rgbd.BonnLayout()), K32)
        else:
            c = _backproject_gl(raw[t].astype(np.float32) / np.float32(divisor), K32)
        bad = np.isnan(c).any(0)
        d = -c[2]
        d[np.isnan(d)] = 0
        bad |= (d < 1e-3) | (d > max_depth)
        c[:, bad] = 0
        n, valid = fit_normals(c, ~bad, **opts)
        w = world_normals(n, M[t])
        pick = lambda a: np.ascontiguousarray(a[..., rows, :][..., cols])
        out = [pick(n), pick(w), pick(valid)]
        if zoomed:
            out = [a + np.float32(0) for a in out]            # the zoom's sum 0 + 1 * v: -0 -> +0, nothing else changes
        cn.append(out[0]); wn.append(out[1]); nm.append(out[2])
    return np.stack(cn), np.stack(wn), np.stack(nm)


def _check(dev, host, what):
    for name, a, b in zip(("cam_normal", "world_normal", "normal_mask"), dev, host):
        assert a.dtype == np.float32 and a.shape == b.shape, (what, name)
        same = _bits(a) == _bits(b)
        assert same.all(), (what, name, int((~same).sum()), float(np.abs(a.astype(np.float64) - b).max()))


# ---------------------------------------------------------------------------------------------------------------- 6. bit equality
TABLES = {"identity": (np.arange(fx.H), np.arange(fx.W), False),
          "zoom": (resize_pick(fx.H, 12), resize_pick(fx.W, 16), True),
          "crop": (3 + np.arange(16), 5 + np.arange(24), False)}


@pytest.mark.parametrize("radius,edge,min_count", [(1, 0.05, None), (2, 0.05, None), (2, None, None), (4, 0.05, 30), (8, None, None), (8, 0.05, 60)])
@pytest.mark.parametrize("tables", sorted(TABLES))
def test_kernel_equals_the_mirror_bit_for_bit(engine, tables, radius, edge, min_count):
    """24 x 32 with radius up to 8: the window leaves the frame on all four sides; 2 frames x 768 pixels = 6 blocks of 256 threads."""
    rows, cols, zoomed = TABLES[tables]
    raw = fx.scene_raw()
    K, M = _cams(fx.T, fx.K40)
    opts = dict(radius=radius, edge=edge, min_count=min_count)
    dev = engine.prep_gt_normals(raw, K, M, rows, cols, max_depth=20.0, zoomed=zoomed, **opts)
    host = _host(raw, fx.K40, M, rows, cols, zoomed, **opts)
    assert dev[2][0].mean() > 0.5 and not dev[2][1].any()     # the scene has valid normals; the frame of zeros has none
    _check(dev, host, (tables, opts))
    if tables == "zoom":                                      # the tables are _resize's: the host's own order-0 zoom gives the same arrays
        full = _host(raw, fx.K40, M, np.arange(fx.H), np.arange(fx.W), False, **opts)
        for a, b in zip(dev, full):
            assert np.array_equal(_bits(a), _bits(np.stack([_resize(x, 12, 16, 0, False) for x in b])))


def test_depth_f64_flag_on_the_bonn_scene(engine):
    raw = fx.scene_raw(fx.K40, 5000.0)
    K, M = _cams(fx.T, fx.K40)
    rows, cols = np.arange(fx.H), np.arange(fx.W)
    dev = engine.prep_gt_normals(raw, K, M, rows, cols, depth_divisor=5000.0, max_depth=20.0, depth_f64=True)
    _check(dev, _host(raw, fx.K40, M, rows, cols, False, divisor=5000.0, depth_f64=True), "UG_PREP_DEPTH_F64")
    d32 = engine.prep_gt_normals(raw, K, M, rows, cols, depth_divisor=5000.0, max_depth=20.0)
    _check(d32, _host(raw, fx.K40, M, rows, cols, False, divisor=5000.0), "float32 depth, divisor 5000")
    n = int((_bits(dev[0]) != _bits(d32[0])).sum())
    print(f"float64 depth changes {n} of {dev[0].size} normal components")
    assert n >= 1 and dev[2][0].mean() > 0.9


def test_zoomed_flag_turns_minus_zero_into_plus_zero(engine):
    """The principal row (integer cy) makes y = -0 in the points; a one-column frame with cx = 0 makes n0 = -0 on every valid pixel
    (tests/test_gt_normals_cpu.py shows why).  Without the flag the device keeps the -0, as the host's slicing does; with it the -0 comes
    out as +0, as the host's order-0 zoom makes it; nothing else changes."""
    Kc = np.array([[40.0, 0, 0], [0, 40.0, 12.0], [0, 0, 1]])
    raw = np.stack([fx.quantise(fx.plane_depth(fx.N_TILT, fx.D_TILT, Kc, fx.H, 1))] * 2)
    K, M = _cams(2, Kc)
    M = np.broadcast_to(np.eye(4, dtype=np.float32), (2, 4, 4))      # world_normal = cam_normal: its -0 shows too
    rows, cols = np.arange(fx.H), np.arange(1)
    opts = dict(radius=2, min_count=3)
    plain = engine.prep_gt_normals(raw, K, M, rows, cols, max_depth=20.0, zoomed=False, **opts)
    zoom = engine.prep_gt_normals(raw, K, M, rows, cols, max_depth=20.0, zoomed=True, **opts)
    _check(plain, _host(raw, Kc, M, rows, cols, False, **opts), "plain")
    _check(zoom, _host(raw, Kc, M, rows, cols, True, **opts), "zoomed")
    assert plain[2].all() and not plain[0][:, 0].any() and np.signbit(plain[0][:, 0]).all()           # -0
    assert not _bits(zoom[0][:, 0]).any() and not _bits(zoom[1][:, 0]).any()                          # +0
    assert np.array_equal(_bits(plain[0][:, 1:]), _bits(zoom[0][:, 1:])) and np.array_equal(plain[2], zoom[2])
    # the same through a real zoom of the two-plane scene, integer cy
    Ki = np.array([[40.0, 0, 15.5], [0, 40.0, 12.0], [0, 0, 1]])
    raw = fx.scene_raw(Ki)
    K, M = _cams(fx.T, Ki)
    rows, cols = resize_pick(fx.H, 12), resize_pick(fx.W, 16)
    _check(engine.prep_gt_normals(raw, K, M, rows, cols, max_depth=20.0), _host(raw, Ki, M, rows, cols, True), "zoom, integer cy")


# ---------------------------------------------------------------------------------------------------------------- 7. the loaders
@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    base = tmp_path_factory.mktemp("gt_normals_scenes_gpu")
    out = {}
    for L in ("7scenes", "bonn"):
        out[L] = str(base / L)
        fx.write_scene(out[L], L, n_clip=3)
    out["raw7"] = fx.write_raw_7scenes(str(base / "raw7"))
    return out


def _same(dev, host):
    assert list(dev.keys()) == list(host.keys())
    for k in ("cam_normal", "world_normal", "normal_mask", "cam_coord", "mask"):
        a, b = np.stack(dev[k]), np.stack(host[k])
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), k


@pytest.mark.parametrize("size", [None, (12, 16)], ids=["native", "resized"])
@pytest.mark.parametrize("L", ["7scenes", "bonn"])
def test_device_loader_equals_the_host_loader(engine, roots, L, size):
    kw = dict(scenes=[fx.SCENE[L]], clip_length=3, clip_overlap=0, input_size=size, target_size=size, normals="depth")
    host = rgbd.LAYOUTS[L](roots[L], **kw)
    dev = rgbd.LAYOUTS[L](roots[L], prep="device", engine=engine, **kw)
    h, d = host[0], dev[0]
    _same(d, h)
    nm = np.stack(d["normal_mask"])
    assert nm[0].mean() > 0.8 and not nm[1].any() and nm[2].mean() > 0.8
    assert set(dev.last_timing) == {"decode", "resize", "gt", "normals"} and dev.last_timing["normals"] > 0
    plain = rgbd.LAYOUTS[L](roots[L], prep="device", engine=engine, **dict(kw, normals=None))
    assert "cam_normal" not in plain[0] and set(plain.last_timing) == {"decode", "resize", "gt"}


def test_device_loader_with_device_registration(engine, roots):
    """7-Scenes raw depth at 480 x 640: the registered clip feeds both paths; a 96 x 128 target keeps the host's resize small."""
    from register_fixtures import SCENE
    kw = dict(scenes=[SCENE], clip_length=2, clip_overlap=0, input_size=(96, 128), target_size=(96, 128), normals="depth")
    host = rgbd.sevenScenesDataset(roots["raw7"], register="host", **kw)
    dev = rgbd.sevenScenesDataset(roots["raw7"], register="device", prep="device", engine=engine, **kw)
    h, d = host[0], dev[0]
    _same(d, h)
    assert np.stack(d["normal_mask"]).mean() > 0.5 and set(dev.last_timing) == {"decode", "resize", "gt", "normals", "register"}


# ---------------------------------------------------------------------------------------------------------------- 8. error paths
def _raw_call(engine, raw, K, M, rows, cols, radius=2, edge=0.05, min_count=0, flags=0, null=(), opts=True):
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    T, hi, wi = raw.shape
    raw, k, m = np.ascontiguousarray(raw), np.ascontiguousarray(K, dtype=np.float32), np.ascontiguousarray(M, dtype=np.float32)
    rows, cols = np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(cols, dtype=np.int32)
    out = {"cam_normal": np.full((T, 3, rows.size, cols.size), 7, np.float32), "world_normal": np.full((T, 3, rows.size, cols.size), 7, np.float32),
           "normal_mask": np.full((T, rows.size, cols.size), 7, np.float32)}
    ptr = {n: (None if n in null else p(a)) for n, a in out.items()}
    o = GtNormalsOptsC(radius, edge, min_count)
    rc = engine.lib.ug_prep_gt_normals(engine.ctx, None if "depth" in null else p(raw), 1000.0, p(k), p(m), T, hi, wi, p(rows), rows.size, p(cols),
                                       cols.size, 20.0, C.byref(o) if opts else None, ptr["cam_normal"], ptr["world_normal"], ptr["normal_mask"], flags)
    return rc, out


def test_errors_leave_the_engine_usable(engine):
    raw = fx.scene_raw()
    K, M = _cams(fx.T, fx.K40)
    rows, cols = np.arange(fx.H), np.arange(fx.W)
    host = _host(raw, fx.K40, M, rows, cols, False)
    err = lambda: engine.lib.ug_last_error(engine.ctx)

    def valid_call():
        rc, out = _raw_call(engine, raw, K, M, rows, cols, opts=False)                         # opts NULL: the defaults
        assert rc == 0
        _check([out[k] for k in ("cam_normal", "world_normal", "normal_mask")], host, "after an error")

    valid_call()
    for kw, word in ((dict(radius=0), b"radius"), (dict(radius=9), b"radius"), (dict(flags=4 | PREP_ZOOMED), b"0x4"), (dict(min_count=-1), b"min_count"),
                     (dict(edge=float("nan")), b"edge"), (dict(null=("normal_mask",)), b"NULL"), (dict(null=("depth",)), b"NULL")):
        rc, out = _raw_call(engine, raw, K, M, rows, cols, **kw)
        assert rc != 0 and word in err(), (kw, err())
        assert all((a == 7).all() for a in out.values()), kw                                     # nothing was written
        valid_call()
    for r_, c_ in ((np.r_[rows[:-1], fx.H], cols), (rows, np.r_[-1, cols[1:]])):                 # a pick index outside the source
        rc, out = _raw_call(engine, raw, K, M, r_, c_)
        assert rc != 0 and b"outside the source" in err() and all((a == 7).all() for a in out.values())
        valid_call()
    with pytest.raises(ValueError, match="radius"):
        engine.prep_gt_normals(raw, K, M, rows, cols, radius=9)
    o = GtNormalsOptsC()
    engine.lib.ug_gt_normals_opts_default(C.byref(o))
    assert (o.radius, o.edge, o.min_count) == (2, 0.05, 0)
    assert PREP_DEPTH_F64 == 1


# ---------------------------------------------------------------------------------------------------------------- 9. device metrics
def test_device_normal_metrics_use_the_fitted_mask(engine, roots, tmp_path):
    """``evaluate(device_metrics=True)`` hands ``ug_eval_normal`` ``gt_normal_masks``: the same eight columns as the host path - the five percentages
    exactly, the three angle statistics within the bound the project's other host-against-device normal metrics use
    (tests/test_pipeline_gpu.py: rel 2e-4, abs 1e-3).  The model
    predicts the opposite direction wherever the fit is invalid, so a path that scored on ``mask`` alone would read degrees, not zero."""
    import torch
    from unigeo_amd.harness import evaluate

    class Resident:
        """The engine as evaluate() sees a plugin's: the prediction is the one the model just made."""
        pred = None

        def eval_normal(self, gt, mask):
            return engine.eval_normal(gt, mask, pred=self.pred)

    class Model:
        class pipeline:
            engine = Resident()

        def forward(self, data):
            n = np.stack(data["cam_normal"]).transpose(0, 2, 3, 1)
            nm = np.stack(data["normal_mask"]) > 0
            pred = np.ascontiguousarray(np.where(nm[..., None], n, np.float32([0, 0, -1])).astype(np.float32))
            self.pipeline.engine.pred = pred
            return {"pred_depths": torch.zeros(pred.shape[:3]), "pred_normals": torch.from_numpy(pred)}

    cfg = {"dataset": "sevenScenesDataset", "root": roots["7scenes"], "scenes": [fx.SCENE["7scenes"]], "h": 12, "w": 16, "clip_length": 3,
           "clip_overlap": 0, "split": "test", "model_name": "DepthCrafter", "model_params": {}, "normals": "depth",
           "eval_normal": {"metric_names": NORMAL_KEYS}}
    host, _ = evaluate(cfg, model=Model(), save_dir=str(tmp_path / "h"), verbose=False)
    dev, _ = evaluate(cfg, model=Model(), save_dir=str(tmp_path / "d"), verbose=False, device_metrics=True)
    assert len(host) == len(dev) == 1
    print("host", host[0], "\ndevice", dev[0])
    for k in NORMAL_KEYS:
        if k.startswith("angle"):
            assert dev[0][k] == host[0][k], k              # a count over the same pixels: the same percentage
        else:
            assert dev[0][k] == pytest.approx(host[0][k], rel=2e-4, abs=1e-3), k
    assert host[0]["normal mean"] < 0.1 and host[0]["angle < 5"] == 100.0
