"""GPU: ug_pointmap_focal / ug_pointmap_poses (kernels/pointmap.hip) against the numpy mirror harness/pointmap.py - focal and
poses within max(1e-10, 4 x d_order), the same inlier sets and iteration counts, depth bit for bit, the same bytes twice, error paths, and the
harness loop with ``engine=``."""
import ctypes as C

import numpy as np
import pytest

from camera_fixtures import PointMapModel, moving_camera_dataset, pointmap_scene, pose_errors

pytestmark = pytest.mark.gpu


def _P():
    from unigeo_amd.harness import pointmap
    return pointmap


def _case(name):
    if name == "3x24x32":
        pts, ext = pointmap_scene(3, 24, 32, 30.0, seed=1)
        return pts, ext, None, 30.0
    # 2 x 17 x 23 = 391 pixels a frame: a block tail, an odd width, NaN pixels, a mask and a few displaced points for the trim
    pts, ext = pointmap_scene(2, 17, 23, 25.0, seed=5)
    rng = np.random.default_rng(6)
    holes = rng.uniform(size=pts.shape[:3]) < 0.1
    pts[holes, rng.integers(0, 3, int(holes.sum()))] = np.nan
    mask = rng.uniform(size=pts.shape[:3]) < 0.8
    wild = rng.uniform(size=pts.shape[:3]) < 0.04
    pts[wild] += rng.normal(0, 0.8, (int(wild.sum()), 3)).astype(np.float32)
    return pts, ext, mask, 25.0


@pytest.fixture(scope="module", params=["3x24x32", "2x17x23"])
def case(request):
    """Inputs, the mirror's result, and d_order: how far the mirror's own numbers move when every sum takes the pixels in reversed order.
    Computed once for the tests that share it."""
    P = _P()
    pts, ext, mask, f = _case(request.param)
    ref = P.pointmap_poses(pts, focal=f, mask=mask)
    rev = P.pointmap_poses(pts, focal=f, mask=mask, _reverse=True)
    assert np.array_equal(rev["iterations"], ref["iterations"]) and np.array_equal(rev["inliers"], ref["inliers"])
    d_order = float(np.abs(rev["extrinsics"] - ref["extrinsics"]).max())
    f_ref, f_rev = P.pointmap_focal(pts[0]), P.pointmap_focal(pts[0], _reverse=True)
    return pts, ext, mask, f, ref, d_order, f_ref, abs(f_rev - f_ref)


def test_focal_matches_the_mirror(engine, case):
    pts, _, _, _, _, _, f_ref, d_order = case
    f = engine.pointmap_focal(pts[0])
    print(f"focal: device {f!r} mirror {f_ref!r} |diff| {abs(f - f_ref):.3g} d_order {d_order:.3g}")
    assert abs(f - f_ref) <= max(1e-10, 4 * d_order)
    assert engine.pointmap_focal(pts[0]) == f
    assert engine.pointmap_focal(pts[0], pp=(10.0, 9.5)) == pytest.approx(_P().pointmap_focal(pts[0], pp=(10.0, 9.5)), abs=1e-10)


def test_poses_match_the_mirror(engine, case):
    pts, ext, mask, f, ref, d_order, _, _ = case
    res = engine.pointmap_poses(pts, f, mask=mask)
    d = float(np.abs(res["extrinsics"] - ref["extrinsics"]).max())
    print(f"poses: |device - mirror| {d:.3g} d_order {d_order:.3g} iterations {res['iterations'].tolist()} inliers {res['n_inliers'].tolist()} "
          f"of {pts.shape[1] * pts.shape[2]}, errors against the truth {pose_errors(res['extrinsics'], ext)}")
    assert np.array_equal(res["iterations"], ref["iterations"])
    assert np.array_equal(res["inliers"], ref["inliers"]) and np.array_equal(res["n_inliers"], ref["n_inliers"])
    assert d <= max(1e-10, 4 * d_order)
    assert res["depth"].dtype == np.float32 and res["depth"].tobytes() == ref["depth"].tobytes()
    assert np.abs(res["reproj_rms"] - ref["reproj_rms"]).max() <= 1e-9
    if mask is not None:
        assert (res["n_inliers"] < (np.isfinite(pts).all(-1) & mask).reshape(len(pts), -1).sum(1)).any()      # the trim did something
        assert not res["depth"][~mask].any()


def test_poses_return_the_same_bytes_twice(engine, case):
    pts, _, mask, f, _, _, _, _ = case
    a, b = engine.pointmap_poses(pts, f, mask=mask), engine.pointmap_poses(pts, f, mask=mask)
    for k in ("extrinsics", "depth", "n_inliers", "iterations", "reproj_rms", "inliers"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_errors_are_reported_and_the_context_stays_usable(engine):
    from unigeo_amd._lib import PointmapOptsC, _ptr
    pts, _ = pointmap_scene(2, 8, 8, 12.0, seed=7)
    T, H, W = pts.shape[:3]
    o = PointmapOptsC()
    engine.lib.ug_pointmap_opts_default(C.byref(o))
    assert (o.reproj_px, o.max_iter, o.max_rounds) == (8.0, 300, 5)
    ext, depth, stats = np.zeros((T, 16)), np.zeros((T, H, W), np.float32), np.zeros((T, 3))
    err = lambda: engine.lib.ug_last_error(engine.ctx).decode()

    def call(p=pts, m=None, t=T, h=H, w=W, f=12.0, oo=None, e=ext, d=depth, s=stats):
        return engine.lib.ug_pointmap_poses(engine.ctx, _ptr(p), _ptr(m), t, h, w, f, W / 2.0, H / 2.0, C.byref(o) if oo is None else oo, _ptr(e),
                                            _ptr(d), _ptr(s), None)
    assert call(e=None) != 0 and "NULL" in err()
    assert call(d=None) != 0 and "NULL" in err()
    assert call(s=None) != 0 and "NULL" in err()
    assert call(p=None) != 0 and "NULL" in err()
    assert call(oo=C.POINTER(PointmapOptsC)()) != 0 and "NULL" in err()
    for kw in ({"t": 0}, {"h": 0}, {"w": -1}):
        assert call(**kw) != 0 and "positive" in err()
    assert call(f=0.0) != 0 and "focal" in err()
    assert call(f=float("nan")) != 0 and "focal" in err()
    few = np.zeros((T, H, W), np.uint8)
    few[0] = 1
    few[1, 0, :3] = 1
    assert call(m=few) != 0 and "frame 1 has 3 valid pixels" in err()
    out = np.zeros(1)
    assert engine.lib.ug_pointmap_focal(engine.ctx, None, H, W, 4.0, 4.0, _ptr(out)) != 0 and "NULL" in err()
    assert engine.lib.ug_pointmap_focal(engine.ctx, _ptr(pts), H, W, 4.0, 4.0, None) != 0 and "NULL" in err()
    assert engine.lib.ug_pointmap_focal(engine.ctx, _ptr(pts), 0, W, 4.0, 4.0, _ptr(out)) != 0 and "positive" in err()
    assert call() == 0 and np.isfinite(ext).all() and (stats[:, 0] == H * W).all()          # the context still works


def test_harness_device_rows_equal_the_host_rows(engine, tmp_path):
    """A model without an engine of its own: under device_metrics=True the point-map step runs through ``engine=``; the rows agree with the host
    path within 1e-9."""
    from unigeo_amd.harness import evaluate
    cfg = {"root": "x", "h": 32, "w": 48, "clip_length": 4, "clip_overlap": 1,
           "eval_camera": {"metric_names": ["ATE", "RPE trans", "RPE rot"]}}
    ds = moving_camera_dataset(clip_length=4, clip_overlap=1, input_size=(32, 48), num_frames=6)
    host, _ = evaluate(cfg, dataset=ds, model=PointMapModel(), save_dir=str(tmp_path / "h"), verbose=False)
    calls = []
    real = engine.pointmap_poses
    engine.pointmap_poses = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        dev, _ = evaluate(cfg, dataset=ds, model=PointMapModel(), save_dir=str(tmp_path / "d"), verbose=False, device_metrics=True, engine=engine)
    finally:
        del engine.pointmap_poses
    assert len(calls) == len(host) == len(dev) == 2
    for h_, d_ in zip(host, dev):
        for k in ("ATE", "RPE trans", "RPE rot"):
            print(f"harness {h_['seq_name']} {k}: device {d_[k]:.17g} host {h_[k]:.17g}")
            assert np.isfinite(d_[k]) and abs(d_[k] - h_[k]) <= 1e-9, k
