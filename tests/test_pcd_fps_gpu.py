"""GPU: farthest-point sampling for eval_pcd (ug_op_pcd_fps, ug_eval_pcd_fps; k_pcd_fps in kernels/pcd.hip) against the
numpy mirror of harness/metrics.py.  The kernel alone: indices equal and selected distances bit-equal at the workgroup edges, with more points
than PCD_MAXB x 256, on integer lattices full of ties, with non-finite points, at the extremes and at both parities of k.  The whole call:
indices, clouds and alignment scalars bit-equal to pcd_evaluation(sampling="fps"), metrics within the bound of test_pcd_gpu.py, error
paths, the harness loop.  The last test prints times and is no gate (DESIGN.md section 19 keeps the figures)."""
import ctypes as C
import time

import numpy as np
import pytest

from pcd_fixtures import depth_scene, wavy_grid

pytestmark = pytest.mark.gpu

KEYS = ("acc", "comp", "nc1", "nc2", "acc_med", "comp_med", "nc1_med", "nc2_med")
SCALARS = ("pred_scale", "gt_scale", "pred_shift_z", "gt_shift_z")
f32 = np.float32


def _M():
    from unigeo_amd.harness import metrics
    return metrics


def _check(engine, pts, k):
    idx, sel = engine.op_pcd_fps(pts, k)
    ref_idx, ref_sel = _M().pcd_fps_indices(pts, k)
    assert idx.dtype == np.int64 and sel.dtype == f32 and idx.shape == sel.shape == (k,)
    assert np.array_equal(idx, ref_idx), (np.nonzero(idx != ref_idx)[0][:5], idx[:8], ref_idx[:8])
    assert sel.tobytes() == ref_sel.tobytes()
    return idx, sel


def _cloud(n, seed):
    return np.random.default_rng(seed).normal(size=(n, 3)).astype(f32)


# ------------------------------------------------------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_fps_at_the_workgroup_edges(engine, n):
    """k = n: one workgroup up to 256 points, two at 257; every point is picked once."""
    idx, sel = _check(engine, _cloud(n, n), n)
    assert sorted(idx.tolist()) == list(range(n)) and sel[0] == np.inf


@pytest.mark.parametrize("k", [1, 64, 65])
def test_fps_over_several_workgroups(engine, k):
    """n = 1000: four workgroups, one partial each; k = 1 and an even and an odd k leave the last pick in either partial buffer."""
    _check(engine, _cloud(1000, 7), k)


def test_fps_with_more_points_than_the_grid(engine):
    """300 001 > PCD_MAXB x 256 = 262 144 points: the grid-stride loop takes a second round and all 1024 partial slots are in use."""
    _check(engine, _cloud(300001, 8), 256)


def _lattice(nx, ny, nz):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(f32)
    return np.ascontiguousarray(g)


def test_fps_ties_go_to_the_lowest_index(engine):
    """17 x 17 x 3 integer lattice (867 points, four workgroups): exact distances and many equal ones, inside a workgroup and between the
    partials of different workgroups.  Then 67^3 = 300 763 points: ties between the two grid-stride rounds of one thread as well."""
    pts = _lattice(17, 17, 3)
    idx, sel = _check(engine, pts, 200)
    assert len(set(sel[1:].tolist())) < 20                                            # few distinct distances: the ties are there
    _check(engine, _lattice(67, 67, 67), 64)


def test_fps_skips_non_finite_points(engine):
    pts = _lattice(17, 17, 3)
    pts[0:40:3, 0], pts[1:40:3, 1], pts[2:40:3, 2] = np.nan, np.inf, -np.inf
    idx, _ = _check(engine, pts, 200)
    assert idx[0] == 40 and idx.min() == 40
    idx, sel = _check(engine, pts, len(pts))                                          # k above the finite count: distance-0 repeats, no marked point
    assert idx.min() == 40 and (sel[len(pts) - 40:] == 0).all()
    _check(engine, np.full((300, 3), np.nan, f32), 3)                                 # nothing finite: index 0 with the mark -1


@pytest.mark.parametrize("k", [200, 201])
def test_fps_returns_the_same_bytes_twice_at_either_parity(engine, k):
    pts = _cloud(5000, 9)
    a, b = engine.op_pcd_fps(pts, k), engine.op_pcd_fps(pts, k)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    full = engine.op_pcd_fps(pts, 201)
    assert np.array_equal(full[0][:k], a[0]) and full[1][:k].tobytes() == a[1].tobytes()      # the prefix property


def test_fps_errors_leave_the_context_usable(engine):
    pts = _cloud(10, 1)
    for k in (11, 0):
        with pytest.raises(RuntimeError, match="k must be"):
            engine.op_pcd_fps(pts, k)
    with pytest.raises(RuntimeError, match="n must be"):
        engine.op_pcd_fps(np.zeros((0, 3), f32), 0)
    _check(engine, pts, 10)


# ------------------------------------------------------------------------------------------------------------------ the whole call
def _world_inputs(engine, shape):
    """Prediction = the world points that ug_pcd_world_points makes of a noisy depth (they stay resident), ground truth = the world points of
    the ground-truth depth, mask = its valid pixels."""
    pred, gt, poses, K = depth_scene(shape, 5)
    noisy = (0.7 * gt + 0.3).astype(f32) + (pred - pred.mean()) * f32(0.02)
    gpts = _M().world_points_from_depth(gt, gt, poses, K)[0]
    pts, _ = engine.pcd_world_points(gt, poses, K, pred=noisy)
    rgb = np.random.default_rng(1).uniform(size=shape + (3,)).astype(f32)
    return pts, gpts, gt > 0, rgb


@pytest.fixture(scope="module", params=[((2, 24, 32), 300, False), ((2, 96, 128), 2000, False), ((2, 24, 32), 300, True), ((2, 96, 128), 2000, True)],
                ids=["small-host", "large-host", "small-resident", "large-resident"])
def fps_case(request, engine):
    """Inputs, the mirror's result and d_order (how far the mirror's own numbers move when the sampled clouds are fed in reversed order), computed
    once.  The resident cases run the device call here, while the points of ug_pcd_world_points are still resident."""
    M = _M()
    shape, down, resident = request.param
    if resident:
        pred, gt, mask, rgb = _world_inputs(engine, shape)
        res = engine.eval_pcd(None, gt, mask, rgb, downsample_num=down, sampling="fps")
    else:
        pred, gt, mask, rgb = wavy_grid(*shape, seed=1)
        res = None
    ref = M.pcd_evaluation(pred, gt, mask, rgb, downsample_num=down, sampling="fps")
    rev = M.pcd_metrics_from_clouds(ref["pred_pcd"][0][::-1], ref["gt_pcd"][0][::-1])
    d_order = {k: abs(rev[k] - ref[k]) for k in KEYS}
    d_order["transformation"] = float(np.abs(rev["transformation"] - ref["transformation"]).max())
    assert rev["icp_iterations"] == ref["icp_iterations"]
    return shape, down, (pred, gt, mask, rgb), ref, d_order, res


def test_eval_pcd_fps_matches_the_host_mirror(engine, fps_case):
    """Indices, clouds, colours and alignment scalars bit-equal; behind identical indices the code is ug_eval_pcd's, so metrics and transformation
    keep its bound max(1e-10, 4 x d_order)."""
    shape, down, (pred, gt, mask, rgb), ref, d_order, res = fps_case
    if res is None:
        res = engine.eval_pcd(pred, gt, mask, rgb, downsample_num=down, sampling="fps")
    assert res["n_points"] == ref["n_points"] == down < int(mask.sum())
    for k in ("pred_idx", "gt_idx"):
        assert res[k].dtype == np.int64 and np.array_equal(res[k], ref[k]), k
    assert not np.array_equal(res["pred_idx"], res["gt_idx"])
    for k in SCALARS:
        assert f32(res[k]).tobytes() == f32(ref[k]).tobytes(), k
    for k in ("pred_pcd", "gt_pcd"):
        assert res[k][0].tobytes() == ref[k][0].tobytes() and res[k][1].tobytes() == ref[k][1].tobytes(), k
    print(f"eval_pcd fps {shape} n={res['n_points']}: iterations device {res['icp_iterations']} host {ref['icp_iterations']}, "
          f"fitness {res['icp_fitness']:.6f} rmse {res['icp_rmse']:.6e}")
    for k in KEYS:
        print(f"  {k}: device {res[k]:.17g} host {ref[k]:.17g} |diff| {abs(res[k] - ref[k]):.3g} d_order {d_order[k]:.3g}")
    dT = float(np.abs(res["transformation"] - ref["transformation"]).max())
    print(f"  transformation |diff| {dT:.3g} d_order {d_order['transformation']:.3g}")
    assert res["icp_iterations"] == ref["icp_iterations"]
    for k in KEYS:
        assert abs(res[k] - ref[k]) <= max(1e-10, 4 * d_order[k]), k
    assert dT <= max(1e-10, 4 * d_order["transformation"])
    again = engine.eval_pcd(pred, gt, mask, rgb, downsample_num=down, sampling="fps")      # twice, or resident and uploaded points: the same bytes
    for k in KEYS + SCALARS:
        assert np.float64(res[k]).tobytes() == np.float64(again[k]).tobytes(), k
    assert np.array_equal(res["pred_idx"], again["pred_idx"]) and res["pred_pcd"][0].tobytes() == again["pred_pcd"][0].tobytes()
    assert res["transformation"].tobytes() == again["transformation"].tobytes()


def test_fps_with_every_point_is_eval_pcd_without_an_index_list(engine):
    pred, gt, mask, rgb = wavy_grid(2, 24, 32, seed=1)
    n = int(mask.sum())
    plain = engine.eval_pcd(pred, gt, mask, rgb)
    for down in (n, n + 1, -1, 0):
        res = engine.eval_pcd(pred, gt, mask, rgb, downsample_num=down, sampling="fps")
        assert np.array_equal(res["pred_idx"], np.arange(n)) and np.array_equal(res["gt_idx"], np.arange(n))
        for k in KEYS + SCALARS + ("n_points", "icp_iterations", "icp_fitness", "icp_rmse"):
            assert np.float64(res[k]).tobytes() == np.float64(plain[k]).tobytes(), k
        assert res["transformation"].tobytes() == plain["transformation"].tobytes()
        for k in ("pred_pcd", "gt_pcd"):
            assert res[k][0].tobytes() == plain[k][0].tobytes() and res[k][1].tobytes() == plain[k][1].tobytes(), k
    empty = engine.eval_pcd(pred, gt, np.zeros_like(mask), rgb, downsample_num=300, sampling="fps")
    assert empty["n_points"] == 0 and len(empty["pred_idx"]) == 0 and all(np.isnan(empty[k]) for k in KEYS)
    with pytest.raises(ValueError, match="sampling"):
        engine.eval_pcd(pred, gt, mask, rgb, sampling="grid")


def test_eval_pcd_fps_errors_are_reported_and_the_context_stays_usable(engine):
    from unigeo_amd._lib import PcdOptsC, _ptr
    pred, gt, mask, _ = wavy_grid(1, 8, 8, seed=6)
    p, g = np.ascontiguousarray(pred.reshape(-1, 3)), np.ascontiguousarray(gt.reshape(-1, 3))
    m = np.ascontiguousarray(mask.reshape(-1).astype(np.uint8))
    out = np.zeros(32, np.float64)
    o = PcdOptsC()
    engine.lib.ug_pcd_opts_default(C.byref(o))
    ip, ig = np.zeros(20, np.int64), np.zeros(20, np.int64)
    call = lambda pp, gg, mm, oo, oout, n=len(m): engine.lib.ug_eval_pcd_fps(engine.ctx, _ptr(pp), _ptr(gg), _ptr(mm), n, 20, oo, _ptr(oout), None,
                                                                             None, _ptr(ip), _ptr(ig))
    err = lambda: engine.lib.ug_last_error(engine.ctx).decode()
    assert call(p, None, m, C.byref(o), out) != 0 and "NULL" in err()
    assert call(p, g, None, C.byref(o), out) != 0 and "NULL" in err()
    assert call(p, g, m, C.byref(o), out, n=0) != 0 and "n_pixels" in err()
    o.knn = 0
    assert call(p, g, m, C.byref(o), out) != 0 and "knn" in err()
    o.knn = 30
    n_big = (1 << 20) + 1                                   # every point of (2^20 + 1): above the pair cap; sampled down it passes the cap
    big = np.zeros((n_big, 3), f32)
    with pytest.raises(RuntimeError, match="pcd_downsample_num"):
        engine.eval_pcd(big, big, np.ones(n_big, bool), return_clouds=False, sampling="fps")
    assert call(p, g, m, C.byref(o), out) == 0 and out[8] == 20 and np.isfinite(out[:8]).all()      # the context still works
    assert len(set(ip.tolist())) == 20 and ip.max() < m.sum()
    assert engine.lib.ug_eval_pcd_fps(engine.ctx, _ptr(p), _ptr(g), _ptr(m), len(m), 20, C.byref(o), _ptr(out), None, None, None, None) == 0      # optional


# ------------------------------------------------------------------------------------------------------------------ harness
@pytest.fixture(scope="module")
def tiny_plugin():
    from unigeo_amd import weights as W
    from unigeo_amd.model import DepthCrafter
    m = DepthCrafter(synthetic_weights=True, cfgs=W.tiny_cfgs(), num_inference_steps=2, workspace_bytes=3 << 30)
    yield m
    m.pipeline.engine.close()


def test_harness_device_rows_equal_the_host_rows_under_fps(tiny_plugin, tmp_path):
    """As test_harness_device_rows_equal_the_host_rows with `sampling: fps`: the device path samples the points it made from the resident
    depth, the host path the ones from the downloaded depth; the same points give the same picks, and the rows agree within 1e-10."""
    from unigeo_amd.harness import SyntheticGeometryDataset, evaluate, read_ply
    cfg = {"root": "x", "h": 64, "w": 64, "clip_length": 3, "clip_overlap": 1, "vis_pcd": True,
           "eval_depth": {"metric_names": ["Abs Rel"]},
           "eval_pcd": {"metric_names": ["acc", "comp", "nc1", "nc2"], "pcd_downsample_num": 1500, "sampling": "fps"}}
    ds = SyntheticGeometryDataset(clip_length=3, clip_overlap=1, input_size=(64, 64), num_frames=5)
    host, _ = evaluate(cfg, dataset=ds, model=tiny_plugin, save_dir=str(tmp_path / "h"), verbose=False)
    dev, _ = evaluate(cfg, dataset=ds, model=tiny_plugin, save_dir=str(tmp_path / "d"), verbose=False, device_metrics=True)
    assert len(host) == len(dev) == 3
    for h_, d_ in zip(host, dev):
        for k in KEYS:
            print(f"harness fps {h_['seq_name']} {k}: device {d_[k]:.17g} host {h_[k]:.17g}")
        for k in KEYS:
            assert np.isfinite(d_[k]) and abs(d_[k] - h_[k]) <= 1e-10, k
        for name in ("pred.ply", "gt.ply"):
            a, ca = read_ply(str(tmp_path / "h" / f"pcd_{h_['seq_name']}" / name))
            b, cb = read_ply(str(tmp_path / "d" / f"pcd_{h_['seq_name']}" / name))
            assert a.shape == (1500, 3) and a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes(), name


# ------------------------------------------------------------------------------------------------------------------ timing (not a gate)
def test_print_the_fps_times(engine):
    """Not a gate: the masked points of wavy_grid(2, 384, 512), k = 10 000, the second of two runs, beside the mirror at k = 512 (the prefix
    property makes its first 512 picks the check); and k = 10 000 at n = 10 000, the fewest points that admit that k (40 workgroups, one
    point per thread), where a launch does next to no work: the cost of a launch."""
    M = _M()
    pred, _, mask, _ = wavy_grid(2, 384, 512, seed=1)
    pts = np.ascontiguousarray(pred[mask])
    k = 10000
    engine.op_pcd_fps(pts, k)
    t0 = time.perf_counter(); idx, sel = engine.op_pcd_fps(pts, k); t_dev = time.perf_counter() - t0
    t0 = time.perf_counter(); ref_idx, ref_sel = M.pcd_fps_indices(pts, 512); t_host = time.perf_counter() - t0
    assert np.array_equal(idx[:512], ref_idx) and sel[:512].tobytes() == ref_sel.tobytes()
    assert len(np.unique(idx)) == k and (np.diff(sel[1:]) <= 0).all()
    small = _cloud(k, 3)
    engine.op_pcd_fps(small, k)
    t0 = time.perf_counter(); engine.op_pcd_fps(small, k); t_small = time.perf_counter() - t0
    print(f"fps timing n={len(pts)} k={k}: device {t_dev:.3f} s = {t_dev / k * 1e6:.1f} us per step (with transfers); "
          f"host mirror k=512 {t_host:.3f} s = {t_host / 512 * 1e6:.0f} us per step; "
          f"n={k} k={k}: device {t_small:.3f} s = {t_small / k * 1e6:.1f} us per launch")
