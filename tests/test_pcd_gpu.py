"""GPU: point-cloud evaluation on the device (ug_pcd_world_points, ug_eval_pcd and the ug_op_pcd_* entry points; kernels/pcd.hip, DESIGN.md
section 18) against the numpy mirror of harness/metrics.py: nearest neighbours, exact selection and KNN lists bit for bit, normals against
numpy.linalg.eigh, world points against world_points_from_depth, the whole call against pcd_evaluation, error paths, and the harness loop.

Measured on MI355X (printed by the tests; DESIGN.md section 18 keeps the figures): ug_eval_pcd against the mirror at most 5.4e-15 on the
metrics and 1.95e-14 on the transformation (d_order 5.7e-15 / 2.0e-14), the same ICP update counts (4 and 14), KNN normals within 6.7e-16
of numpy.linalg.eigh in |dot|, world points equal to the mirror's in every coordinate, harness rows within 1.5e-15."""
import ctypes as C
import time

import numpy as np
import pytest

from pcd_fixtures import depth_scene, wavy_grid, wavy_pair

pytestmark = pytest.mark.gpu

KEYS = ("acc", "comp", "nc1", "nc2", "acc_med", "comp_med", "nc1_med", "nc2_med")
SCALARS = ("pred_scale", "gt_scale", "pred_shift_z", "gt_shift_z")


def _M():
    from unigeo_amd.harness import metrics
    return metrics


# ------------------------------------------------------------------------------------------------------------------ op level
@pytest.mark.parametrize("nq,nt", [(1, 1), (257, 1000), (1000, 257)])
@pytest.mark.parametrize("moved", [False, True])
def test_nearest_neighbour_equals_the_brute_force_bit_for_bit(engine, nq, nt, moved):
    """Queries and targets that are no multiple of the block (256) or the tile (256), several blockIdx.y slices, a partial last tile."""
    M = _M()
    rng = np.random.default_rng(nq * 7 + nt)
    q, t = rng.normal(size=(nq, 3)), rng.normal(size=(nt, 3))
    T = None
    if moved:
        T = np.eye(4)
        T[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        T[:3, 3] = rng.normal(size=3) * 0.1
    dist, idx = engine.op_pcd_nn(q, t, T)
    rd, ri = M.nn_brute(q if T is None else M._move(T, q), t)
    assert np.array_equal(idx, ri)
    assert dist.tobytes() == rd.tobytes()


def test_nearest_neighbour_ties_go_to_the_lowest_index(engine):
    rng = np.random.default_rng(3)
    base = rng.normal(size=(300, 3))
    t = np.concatenate([base, base[::-1], base])           # every target three times, in two different slices
    q = base + rng.normal(size=base.shape) * 1e-3
    dist, idx = engine.op_pcd_nn(q, t)
    rd, ri = _M().nn_brute(q, t)
    assert np.array_equal(idx, ri) and idx.max() < 300 and dist.tobytes() == rd.tobytes()
    dist, idx = engine.op_pcd_nn(base, t)                   # exact hits: distance 0 at the first copy
    assert np.array_equal(idx, np.arange(300)) and not dist.any()


@pytest.mark.parametrize("n", [1, 2, 255, 70001])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_select_equals_the_sorted_element(engine, n, dtype):
    """Negative values, both zeros and repeated values; one block, a partial block, and 274 blocks whose histograms are merged.  np.sort
    leaves -0.0 and +0.0 in the order it found them; the key order puts -0.0 first, so the expected array orders its zeros that way."""
    rng = np.random.default_rng(n)
    v = rng.normal(size=n).astype(dtype)
    v[rng.uniform(size=n) < 0.2] = dtype(0.0)
    v[rng.uniform(size=n) < 0.1] = dtype(-0.0)
    if n > 2:
        v[rng.integers(0, n, n // 3)] = v[rng.integers(0, n, n // 3)]      # repeated values
    s = np.sort(v)
    z = s == 0
    s[z] = np.where(np.sort(np.signbit(s[z]))[::-1], dtype(-0.0), dtype(0.0))
    for k in sorted({0, n - 1, (n - 1) // 2, n // 2, n // 3, min(n - 1, 7)}):
        got = engine.op_pcd_select(v, k)
        assert got.dtype == dtype and got.tobytes() == s[k].tobytes(), (n, k, got, s[k])


@pytest.mark.parametrize("n", [1, 2, 29, 30, 31, 700])
def test_knn_lists_and_normals(engine, n):
    """Measured: smallest eigenvalue ratio 35.9 (n = 31); |dot| with eigh >= 1 - 1e-12."""
    M = _M()
    pts = wavy_pair(n, seed=n)[0].astype(np.float64)
    nbr, nrm = engine.op_pcd_knn_normals(pts, 30)
    ref = M.knn_brute(pts, 30)
    assert nbr.shape == ref.shape == (n, min(n, 30))
    assert np.array_equal(nbr, ref)                        # the same neighbours in the same (distance, index) order
    if n < 3:
        assert np.array_equal(nrm, np.tile([0.0, 0.0, 1.0], (n, 1)))
        return
    nb = pts[ref]
    c = nb - nb.mean(1, keepdims=True)
    w, v = np.linalg.eigh(np.einsum("nki,nkj->nij", c, c) / nb.shape[1])
    ratio = float((w[:, 1] / w[:, 0]).min())
    dots = np.abs(np.sum(v[:, :, 0] * nrm, -1))
    print(f"knn normals n={n}: eigenvalue ratio >= {ratio:.3g}, min |dot| = 1 - {1 - dots.min():.3g}")
    assert ratio >= 10
    assert dots.min() >= 1 - 1e-12
    np.testing.assert_allclose(np.linalg.norm(nrm, axis=-1), 1.0, atol=1e-14)


def test_knn_ties_follow_the_index(engine):
    rng = np.random.default_rng(5)
    base = rng.normal(size=(40, 3))
    pts = np.concatenate([base, base, base])               # every point three times: ties inside every list and at its end
    nbr, _ = engine.op_pcd_knn_normals(pts, 7)
    assert np.array_equal(nbr, _M().knn_brute(pts, 7))


# ------------------------------------------------------------------------------------------------------------------ world points
@pytest.mark.parametrize("shape,rtol,atol", [((1, 3, 5), 1e-5, 1e-6), ((2, 384, 512), 2e-4, 0.0)])
def test_world_points_match_the_host_mirror(engine, shape, rtol, atol):
    """The bounds tests/test_depth_global_gpu.py puts on the radius of the same arithmetic.  A coordinate is a signed sum that can cancel to
    zero while its error scales with the whole point, so the relative bound is taken against the point's radius."""
    M = _M()
    pred, gt, poses, K = depth_scene(shape, 5)
    pts, fit = engine.pcd_world_points(gt, poses, K, pred=pred)
    ref, ref_fit = M.world_points_from_depth(pred, gt, poses, K)
    assert pts.shape == ref.shape == shape + (3,) and pts.dtype == np.float32
    assert fit == pytest.approx(ref_fit, rel=rtol, abs=atol)
    err = np.abs(pts.astype(np.float64) - ref).max(-1)
    bound = atol + rtol * np.linalg.norm(ref.astype(np.float64), axis=-1)
    print(f"world points {shape}: max error / bound = {(err / bound).max():.3g}, bit-equal coordinates {np.mean(pts == ref):.6f}")
    assert (err <= bound).all()
    clip = dict(pre_clip_min=0.5, pre_clip_max=5.0, post_clip_min=0.6, post_clip_max=4.0)
    pts_c, _ = engine.pcd_world_points(gt, poses, K, pred=pred, **clip)
    ref_c, _ = M.world_points_from_depth(pred, gt, poses, K, **clip)
    assert (np.abs(pts_c.astype(np.float64) - ref_c).max(-1) <= atol + rtol * np.linalg.norm(ref_c.astype(np.float64), axis=-1)).all()
    assert not np.array_equal(pts_c, pts)


@pytest.fixture(scope="module")
def tiny_plugin():
    from unigeo_amd import weights as W
    from unigeo_amd.model import DepthCrafter
    m = DepthCrafter(synthetic_weights=True, cfgs=W.tiny_cfgs(), num_inference_steps=2, workspace_bytes=3 << 30)
    yield m
    m.pipeline.engine.close()


def test_resident_depth_and_resident_points_give_the_same_bytes(tiny_plugin):
    from unigeo_amd.synthetic import synthetic_clip
    tiny_plugin.forward(synthetic_clip(3, 64, 64, seed=1))
    eng = tiny_plugin.pipeline.engine
    _, depth, _ = eng.get_outputs(frames=False, depth=True)
    _, gt, poses, K = depth_scene(depth.shape, 0)
    a, fa = eng.pcd_world_points(gt, poses, K)
    b, fb = eng.pcd_world_points(gt, poses, K, pred=depth)
    assert fa == fb and a.tobytes() == b.tobytes() and np.isfinite(a).all()
    _, gpts, mask, rgb = wavy_grid(*depth.shape, seed=2)
    r1 = eng.eval_pcd(None, gpts, mask, rgb, downsample_num=500)       # the points the last call left on the device
    r2 = eng.eval_pcd(b, gpts, mask, rgb, downsample_num=500)
    assert all(np.array_equal(r1[k], r2[k], equal_nan=True) for k in KEYS + SCALARS) and r1["pred_pcd"][0].tobytes() == r2["pred_pcd"][0].tobytes()
    with pytest.raises(RuntimeError, match="resident"):                 # another size than the resident points'
        eng.eval_pcd(None, gpts[:2], mask[:2])


# ------------------------------------------------------------------------------------------------------------------ the whole call
@pytest.fixture(scope="module", params=[((2, 24, 32), -1), ((2, 384, 512), 10000)], ids=["small", "frame-size"])
def icp_case(request):
    """Inputs, the mirror's result, and d_order: how far the mirror's own numbers move when the aligned clouds are fed in reversed order -
    the neighbours stay, only the summation order changes.  Computed once for the tests that share it."""
    M = _M()
    shape, down = request.param
    pred, gt, mask, rgb = wavy_grid(*shape, seed=1)
    ref = M.pcd_evaluation(pred, gt, mask, rgb, downsample_num=down, seed=3)
    rev = M.pcd_metrics_from_clouds(ref["pred_pcd"][0][::-1], ref["gt_pcd"][0][::-1])
    d_order = {k: abs(rev[k] - ref[k]) for k in KEYS}
    d_order["transformation"] = float(np.abs(rev["transformation"] - ref["transformation"]).max())
    assert rev["icp_iterations"] == ref["icp_iterations"]
    return shape, down, (pred, gt, mask, rgb), ref, d_order


def test_eval_pcd_matches_the_host_mirror(engine, icp_case):
    """(2, 24, 32) with about a quarter of the pixels masked out, and (2, 384, 512) sampled down to 10 000 points: 393 216 pixels cross the
    1024-block cap of the compaction.  Alignment scalars and clouds bit-equal, the same iteration count, metrics and transformation within
    max(1e-10, 4 x d_order) - the factor 4 covers the device's different reduction tree, the floor only guards d_order = 0."""
    shape, down, (pred, gt, mask, rgb), ref, d_order = icp_case
    res = engine.eval_pcd(pred, gt, mask, rgb, downsample_num=down, seed=3)
    assert res["n_points"] == ref["n_points"] == (int(mask.sum()) if down < 0 else down)
    for k in SCALARS:
        assert np.float32(res[k]).tobytes() == np.float32(ref[k]).tobytes(), k
    for k in ("pred_pcd", "gt_pcd"):
        assert res[k][0].tobytes() == ref[k][0].tobytes() and res[k][1].tobytes() == ref[k][1].tobytes(), k
    print(f"eval_pcd {shape} n={res['n_points']}: iterations device {res['icp_iterations']} host {ref['icp_iterations']}, "
          f"fitness {res['icp_fitness']:.6f} rmse {res['icp_rmse']:.6e}")
    steps = np.abs(np.diff(np.asarray(ref["icp_history"]), axis=0))
    print("  host |d fitness|, |d rmse| per update:", steps.tolist())
    assert res["icp_iterations"] == ref["icp_iterations"]
    for k in KEYS:
        print(f"  {k}: device {res[k]:.17g} host {ref[k]:.17g} |diff| {abs(res[k] - ref[k]):.3g} d_order {d_order[k]:.3g}")
    dT = float(np.abs(res["transformation"] - ref["transformation"]).max())
    print(f"  transformation |diff| {dT:.3g} d_order {d_order['transformation']:.3g}")
    for k in KEYS:
        assert abs(res[k] - ref[k]) <= max(1e-10, 4 * d_order[k]), k
    assert dT <= max(1e-10, 4 * d_order["transformation"])
    assert res["icp_fitness"] == pytest.approx(ref["icp_fitness"], abs=1e-10) and res["icp_rmse"] == pytest.approx(ref["icp_rmse"], abs=1e-10)


def test_eval_pcd_returns_the_same_bytes_twice(engine, icp_case):
    _, down, (pred, gt, mask, rgb), _, _ = icp_case
    a = engine.eval_pcd(pred, gt, mask, rgb, downsample_num=down, seed=3)
    b = engine.eval_pcd(pred, gt, mask, rgb, downsample_num=down, seed=3)
    for k in KEYS + SCALARS + ("icp_fitness", "icp_rmse", "icp_iterations"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k
    assert a["transformation"].tobytes() == b["transformation"].tobytes()
    c = engine.eval_pcd(pred, gt, mask, downsample_num=down, seed=3, return_clouds=False)      # the clouds are optional
    assert all(a[k] == c[k] for k in KEYS) and "pred_pcd" not in c


def test_no_correspondence_returns_the_identity_after_one_update(engine):
    pred, gt, mask, _ = wavy_grid(1, 8, 8, seed=4, keep=1.0)
    far = pred.copy()
    far[..., 0] = far[..., 0] * 50.0 + 400.0               # the x spread survives the median alignment: nothing within the threshold
    res = engine.eval_pcd(far, gt, mask)
    ref = _M().pcd_evaluation(far, gt, mask)
    assert res["icp_iterations"] == ref["icp_iterations"] == 1 and res["icp_fitness"] == ref["icp_fitness"] == 0.0 and res["icp_rmse"] == 0.0
    assert np.array_equal(res["transformation"], np.eye(4)) and np.array_equal(ref["transformation"], np.eye(4))
    for k in KEYS:
        assert res[k] == pytest.approx(ref[k], abs=1e-10), k


# ------------------------------------------------------------------------------------------------------------------ error paths
def test_errors_are_reported_and_the_context_stays_usable(engine):
    from unigeo_amd._lib import PcdOptsC, _ptr
    pred, gt, mask, _ = wavy_grid(1, 8, 8, seed=6)
    p, g = np.ascontiguousarray(pred.reshape(-1, 3)), np.ascontiguousarray(gt.reshape(-1, 3))
    m = np.ascontiguousarray(mask.reshape(-1).astype(np.uint8))
    out = np.zeros(32, np.float64)
    o = PcdOptsC()
    engine.lib.ug_pcd_opts_default(C.byref(o))
    assert (round(o.threshold, 6), o.max_iteration, o.knn) == (0.1, 30, 30)
    call = lambda pp, gg, mm, oo, oout, n=len(m): engine.lib.ug_eval_pcd(engine.ctx, _ptr(pp), _ptr(gg), _ptr(mm), n, None, 0, oo, _ptr(oout), None, None)
    err = lambda: engine.lib.ug_last_error(engine.ctx).decode()
    assert call(p, None, m, C.byref(o), out) != 0 and "NULL" in err()
    assert call(p, g, None, C.byref(o), out) != 0 and "NULL" in err()
    assert call(p, g, m, None, out) != 0 and "NULL" in err()
    assert call(p, g, m, C.byref(o), None) != 0 and "NULL" in err()
    assert call(p, g, m, C.byref(o), out, n=0) != 0 and "n_pixels" in err()
    o.knn = 33
    assert call(p, g, m, C.byref(o), out) != 0 and "knn" in err()
    o.knn = 30
    bad = np.array([0, len(m)], np.int64)
    assert engine.lib.ug_eval_pcd(engine.ctx, _ptr(p), _ptr(g), _ptr(m), len(m), _ptr(bad), 2, C.byref(o), _ptr(out), None, None) != 0 and "sample index" in err()
    n_big = (1 << 20) + 1                                   # (2^20 + 1)^2 pairs: just above the cap; rejected before any pair is formed
    big = np.zeros((n_big, 3), np.float32)
    with pytest.raises(RuntimeError, match="pcd_downsample_num"):
        engine.eval_pcd(big, big, np.ones(n_big, bool), return_clouds=False)
    with pytest.raises(RuntimeError, match="pcd_downsample_num"):
        engine.op_pcd_nn(np.zeros((n_big, 3)), np.zeros((n_big, 3)))
    assert call(p, g, m, C.byref(o), out) == 0 and out[8] == m.sum() and np.isfinite(out[:8]).all()      # the context still works


def test_empty_mask_gives_nan_metrics_on_both_paths(engine):
    pred, gt, mask, rgb = wavy_grid(1, 8, 8, seed=6)
    res = engine.eval_pcd(pred, gt, np.zeros_like(mask), rgb)
    ref = _M().pcd_evaluation(pred, gt, np.zeros_like(mask), rgb)
    for r in (res, ref):
        assert r["n_points"] == 0 and r["icp_iterations"] == 0 and all(np.isnan(r[k]) for k in KEYS + SCALARS)
        assert np.array_equal(r["transformation"], np.eye(4)) and r["pred_pcd"][0].shape == (0, 3)


# ------------------------------------------------------------------------------------------------------------------ harness
def test_harness_device_rows_equal_the_host_rows(tiny_plugin, tmp_path):
    """The device path makes its points from the resident depth, the host path from the downloaded one; with the same float32 fit both give
    the same points, so the rows agree within the floor of the bound above (d_order measured there stays below 1e-14)."""
    from unigeo_amd.harness import SyntheticGeometryDataset, evaluate, read_ply
    cfg = {"root": "x", "h": 64, "w": 64, "clip_length": 3, "clip_overlap": 1, "vis_pcd": True,
           "eval_depth": {"metric_names": ["Abs Rel"]},
           "eval_pcd": {"metric_names": ["acc", "comp", "nc1", "nc2"], "pcd_downsample_num": 1500, "seed": 7}}
    ds = SyntheticGeometryDataset(clip_length=3, clip_overlap=1, input_size=(64, 64), num_frames=5)
    host, _ = evaluate(cfg, dataset=ds, model=tiny_plugin, save_dir=str(tmp_path / "h"), verbose=False)
    dev, mm = evaluate(cfg, dataset=ds, model=tiny_plugin, save_dir=str(tmp_path / "d"), verbose=False, device_metrics=True)
    assert len(host) == len(dev) == 3
    for h_, d_ in zip(host, dev):
        for k in KEYS:
            print(f"harness {h_['seq_name']} {k}: device {d_[k]:.17g} host {h_[k]:.17g}")
        for k in KEYS:
            assert np.isfinite(d_[k]) and abs(d_[k] - h_[k]) <= 1e-10, k
        for sub in ("h", "d"):
            for name in ("pred.ply", "gt.ply"):
                pts, col = read_ply(str(tmp_path / sub / f"pcd_{h_['seq_name']}" / name))
                assert pts.shape == col.shape == (1500, 3) and np.isfinite(pts).all()
    assert not np.isnan(mm.calculate_averages()["acc"])


# ------------------------------------------------------------------------------------------------------------------ timing (not a gate)
@pytest.mark.parametrize("n", [10000, 262144])
def test_print_the_times(engine, n):
    """Not a gate: prints one nearest-neighbour pass and the whole call beside the mirror's times (DESIGN.md section 18 keeps the figures of the
    day).  At 262 144 points the mirror's brute-force KNN is out of reach of a test; only its k-d tree pass is timed there."""
    M = _M()
    pred, gt = wavy_pair(n, seed=9)
    p64, g64 = pred.astype(np.float64), gt.astype(np.float64)
    engine.op_pcd_nn(p64[:300], g64[:300])
    t0 = time.perf_counter(); dist, idx = engine.op_pcd_nn(p64, g64); t_nn = time.perf_counter() - t0
    t0 = time.perf_counter(); rd, _ = M._nn(p64, g64); t_nn_host = time.perf_counter() - t0
    assert np.abs(dist - rd).max() <= 1e-12
    mask = np.ones(n, bool)
    t0 = time.perf_counter(); res = engine.eval_pcd(pred, gt, mask, return_clouds=False); t_all = time.perf_counter() - t0
    t_host = "not run"
    if n <= 10000:
        t0 = time.perf_counter(); M.pcd_evaluation(pred, gt, mask); t_host = f"{time.perf_counter() - t0:.3f} s"
    print(f"timing n={n}: nearest-neighbour pass (with transfers) device {t_nn * 1e3:.1f} ms, host k-d tree {t_nn_host * 1e3:.1f} ms; "
          f"whole call device {t_all:.3f} s ({res['icp_iterations']} ICP updates), host mirror {t_host}")
    assert np.isfinite(res["acc"])
