"""GPU: the exact search through a uniform grid (ug_op_pcd_nn_grid, ug_op_pcd_knn_normals_grid, ug_eval_pcd_ex with UG_PCD_SEARCH_GRID;
kernels/pcd.hip) against the brute-force kernels on the same arrays.  A different search changes no arithmetic: every
comparison is on bytes, there is no tolerance anywhere.  Where the share of queries that the grid leaves to the brute-force kernels is
bounded (at most 5 % on the in-distribution clouds) the bound is a condition on the rule for the cell edge and on the ring cap, so that the
grid kernels are what these tests exercise."""
import ctypes as C

import numpy as np
import pytest

from pcd_fixtures import depth_scene, wavy_grid, wavy_pair
from pcd_grid_fixtures import cluster, lattice, planar

pytestmark = pytest.mark.gpu

f32 = np.float32


def _M():
    from unigeo_amd.harness import metrics
    return metrics


def _turn(angle, shift):
    c, s = np.cos(angle), np.sin(angle)
    T = np.eye(4)
    T[:3, :3] = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = shift
    return T


def _nn_case(name):
    """-> (query, target, T44 or None, compare with the numpy mirror, most leftovers allowed or None, fewest leftovers expected)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "one-target":
        return rng.normal(size=(100, 3)), np.array([[0.25, -1.0, 2.0]]), None, True, None, 0
    if name == "two-equal-targets":
        return rng.normal(size=(100, 3)), np.array([[0.25, -1.0, 2.0]] * 2), None, True, None, 0
    if name == "257x255":
        return rng.normal(size=(257, 3)), rng.normal(size=(255, 3)), None, True, None, 0
    if name == "unit-cube":
        return rng.uniform(0, 1, (5000, 3)), rng.uniform(0, 1, (5000, 3)), None, False, 250, 0
    if name == "wavy":
        p, g = wavy_pair(5000)
        return p.astype(np.float64), g.astype(np.float64), None, False, 250, 0
    if name == "lattice":
        q, t = lattice()
        return q, t, None, True, None, 0
    if name == "planar":
        return planar(700, seed=3) + np.array([0.0, 0.0, 0.1]), planar(), None, True, None, 0
    if name == "all-equal":
        return rng.normal(size=(300, 3)), np.tile(np.array([[1.0, 2.0, 3.0]]), (700, 1)), None, True, None, 0
    if name == "cluster":
        t = cluster()
        return np.concatenate([cluster(500, seed=4), t[:200]], 0), t, None, False, None, 0
    if name == "moved-half-outside":
        t = rng.uniform(0, 1, (3000, 3))
        return rng.uniform(0, 1, (2000, 3)), t, _turn(0.3, [0.5, 0.0, 0.0]), False, None, 0
    if name == "non-finite":
        q, t = rng.uniform(0, 1, (1000, 3)), rng.uniform(0, 1, (1000, 3))
        t[rng.choice(1000, 40, replace=False), rng.integers(0, 3, 40)] = np.array([np.nan, np.inf, -np.inf, np.nan] * 10)
        q[rng.choice(1000, 40, replace=False), rng.integers(0, 3, 40)] = np.array([np.inf, np.nan, -np.inf, np.nan] * 10)
        return q, t, None, False, None, 40
    if name == "far-queries":
        t = rng.uniform(0, 1, (5000, 3))
        far = rng.normal(size=(20, 3))
        far = 0.5 + far / np.linalg.norm(far, axis=1, keepdims=True) * rng.uniform(3.0, 50.0, (20, 1))      # the box's diagonal is sqrt(3)
        return np.concatenate([rng.uniform(0, 1, (480, 3)), far], 0), t, None, False, None, 1
    raise KeyError(name)


NN_CASES = ["one-target", "two-equal-targets", "257x255", "unit-cube", "wavy", "lattice", "planar", "all-equal", "cluster", "moved-half-outside",
            "non-finite", "far-queries"]


@pytest.mark.parametrize("name", NN_CASES)
def test_grid_nearest_neighbour_is_the_brute_force_kernel_bit_for_bit(engine, name):
    q, t, T, mirror, most, fewest = _nn_case(name)
    d0, i0 = engine.op_pcd_nn(q, t, T)
    d1, i1, st = engine.op_pcd_nn_grid(q, t, T)
    print(f"nn grid {name}: nq {len(q)} nt {len(t)} {st} leftover share {st['leftover'] / len(q):.4f}")
    assert np.array_equal(i0, i1)
    assert d0.tobytes() == d1.tobytes()
    assert st["settled"] + st["leftover"] == len(q) and 1 <= st["cells"] <= 1 << 24 and 0 <= st["max_cell"] <= len(t)
    if mirror:
        rd, ri = _M().nn_brute(q if T is None else _M()._move(T, q), t)
        assert np.array_equal(i1, ri) and d1.tobytes() == rd.tobytes()
    if most is not None:
        assert st["leftover"] <= most                  # 5 % of the queries: the grid kernel is what ran
    assert st["leftover"] >= fewest
    d2, i2, st2 = engine.op_pcd_nn_grid(q, t, T)      # the order inside a cell and of the leftover list may differ; the outputs may not
    assert i2.tobytes() == i1.tobytes() and d2.tobytes() == d1.tobytes() and st2 == st


def test_lattice_ties_go_to_the_lowest_original_index(engine):
    q, t = lattice()
    d, i, _ = engine.op_pcd_nn_grid(q, t)
    centres = 16 * 16 * 2
    assert np.all(d[:centres] == np.sqrt(0.75)) and not d[centres:].any()
    d2 = ((q[:centres, None, :] - t[None, :, :]) ** 2).sum(-1)                   # exact: halves and integers
    assert np.array_equal(i[:centres], np.argmax(d2 == 0.75, axis=1))           # the first of the eight corners in STORED order
    assert (d2 == 0.75).sum(1).min() == 8


def _knn_cloud(name):
    if name == "lattice":
        return lattice()[1]
    if name == "planar":
        return planar()
    if name == "cluster":
        return cluster()
    if name == "wavy":
        return wavy_pair(5000)[1].astype(np.float64)
    return np.random.default_rng(int(name)).normal(size=(int(name), 3))


@pytest.mark.parametrize("name,knn", [(str(n), 30) for n in (1, 2, 3, 29, 30, 31, 1000, 5000)] + [("1000", 1), ("1000", 3), ("1000", 32), ("31", 32),
                                      ("lattice", 30), ("planar", 30), ("cluster", 30), ("wavy", 30), ("lattice", 3)])
def test_grid_knn_lists_and_normals_are_the_brute_force_kernel_bit_for_bit(engine, name, knn):
    pts = _knn_cloud(name)
    nbr0, nrm0 = engine.op_pcd_knn_normals(pts, knn)
    nbr1, nrm1, st = engine.op_pcd_knn_normals_grid(pts, knn)
    print(f"knn grid {name} k={knn}: n {len(pts)} {st} leftover share {st['leftover'] / len(pts):.4f}")
    assert nbr1.shape == (len(pts), min(knn, len(pts))) and np.array_equal(nbr0, nbr1)
    assert nrm0.tobytes() == nrm1.tobytes()
    assert st["settled"] + st["leftover"] == len(pts)
    if name == "wavy":
        assert st["leftover"] <= len(pts) // 20
    if len(pts) <= 1000:
        assert np.array_equal(nbr1, _M().knn_brute(pts, knn))
    nbr2, nrm2, st2 = engine.op_pcd_knn_normals_grid(pts, knn)
    assert nbr2.tobytes() == nbr1.tobytes() and nrm2.tobytes() == nrm1.tobytes() and st2 == st


def test_grid_knn_with_a_non_finite_point_is_the_brute_force_kernel(engine):
    pts = np.random.default_rng(9).normal(size=(400, 3))
    pts[[3, 250], [0, 2]] = [np.nan, np.inf]
    nbr0, nrm0 = engine.op_pcd_knn_normals(pts, 8)
    nbr1, nrm1, st = engine.op_pcd_knn_normals_grid(pts, 8)
    assert nbr0.tobytes() == nbr1.tobytes() and nrm0.tobytes() == nrm1.tobytes() and st["leftover"] == 400


# ------------------------------------------------------------------------------------------------------------------ the whole call
def _same_entry(a, b, key):
    if isinstance(a, tuple):
        assert len(a) == len(b), key
        for x, y in zip(a, b):
            _same_entry(x, y, key)
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key
    else:
        assert type(a) is type(b) and np.float64(a).tobytes() == np.float64(b).tobytes(), key


def _same_result(brute, grid):
    stats = grid["search_stats"]
    assert set(grid) == set(brute) | {"search_stats"}
    for k, v in brute.items():
        _same_entry(v, grid[k], k)
    return stats


@pytest.mark.parametrize("shape", [(2, 24, 32), (2, 96, 128)])
def test_unsampled_eval_pcd_with_the_grid_is_eval_pcd(engine, shape):
    pred, gt, mask, rgb = wavy_grid(*shape, seed=1)
    brute = engine.eval_pcd(pred, gt, mask, rgb)
    grid = engine.eval_pcd(pred, gt, mask, rgb, search="grid")
    st = _same_result(brute, grid)
    n = brute["n_points"]
    passes = brute["icp_iterations"] + 1 + 2 + 2                       # ICP evaluations, two score passes, two KNN passes
    print(f"eval_pcd grid {shape}: n {n} iterations {brute['icp_iterations']} {st} leftover share {st['leftover'] / (passes * n):.4f}")
    assert n == int(mask.sum()) and st["settled"] + st["leftover"] == passes * n
    assert st["leftover"] <= passes * n // 20
    _same_result(brute, engine.eval_pcd(pred, gt, mask, rgb, search="grid"))


@pytest.mark.parametrize("sampling", ["random", "fps"])
@pytest.mark.parametrize("resident", [False, True])
def test_sampled_eval_pcd_with_the_grid_is_eval_pcd(engine, sampling, resident):
    if resident:
        d_pred, d_gt, poses, K = depth_scene((2, 96, 128), 5)
        noisy = (0.7 * d_gt + 0.3).astype(f32) + (d_pred - d_pred.mean()) * f32(0.02)
        gt = _M().world_points_from_depth(d_gt, d_gt, poses, K)[0]
        engine.pcd_world_points(d_gt, poses, K, pred=noisy, return_points=False)
        pred, mask = None, d_gt > 0
        rgb = np.random.default_rng(1).uniform(size=d_gt.shape + (3,)).astype(f32)
    else:
        pred, gt, mask, rgb = wavy_grid(2, 96, 128, seed=1)
    brute = engine.eval_pcd(pred, gt, mask, rgb, downsample_num=2000, seed=3, sampling=sampling)
    grid = engine.eval_pcd(pred, gt, mask, rgb, downsample_num=2000, seed=3, sampling=sampling, search="grid")
    st = _same_result(brute, grid)
    print(f"eval_pcd grid sampled {sampling} resident={resident}: iterations {brute['icp_iterations']} {st}")
    assert brute["n_points"] == 2000 and ("pred_idx" in grid) == (sampling == "fps")


def test_an_unknown_flag_is_an_error_and_the_context_stays_usable(engine):
    from unigeo_amd._lib import PcdOptsC, _ptr
    pred, gt, mask, _ = wavy_grid(1, 8, 8, seed=6)
    p, g = np.ascontiguousarray(pred.reshape(-1, 3)), np.ascontiguousarray(gt.reshape(-1, 3))
    m = np.ascontiguousarray(mask.reshape(-1).astype(np.uint8))
    out, st = np.zeros(32, np.float64), np.zeros(8, np.int64)
    o = PcdOptsC()
    engine.lib.ug_pcd_opts_default(C.byref(o))
    idx = np.arange(20, dtype=np.int64)
    call = lambda flags, sidx: engine.lib.ug_eval_pcd_ex(engine.ctx, _ptr(p), _ptr(g), _ptr(m), len(m), _ptr(sidx), 20, C.byref(o), flags, _ptr(out),
                                                         None, None, None, None, _ptr(st))
    err = lambda: engine.lib.ug_last_error(engine.ctx).decode()
    assert call(4, None) != 0 and "unknown flag bits 0x4" in err()
    assert call(2 | 8, None) != 0 and "0x8" in err()
    assert call(1, idx) != 0 and "sample_idx" in err()
    assert call(2, idx) == 0 and out[8] == 20 and np.isfinite(out[:8]).all() and st[0] + st[1] > 0      # the context still works
    ref = np.zeros(32, np.float64)
    assert engine.lib.ug_eval_pcd(engine.ctx, _ptr(p), _ptr(g), _ptr(m), len(m), _ptr(idx), 20, C.byref(o), _ptr(ref), None, None) == 0
    assert out.tobytes() == ref.tobytes()
    assert call(0, idx) == 0 and out.tobytes() == ref.tobytes() and not st.any()
    with pytest.raises(ValueError, match="search"):
        engine.eval_pcd(pred, gt, mask, search="tree")


# ------------------------------------------------------------------------------------------------------------------ harness
@pytest.fixture(scope="module")
def tiny_plugin():
    from unigeo_amd import weights as W
    from unigeo_amd.model import DepthCrafter
    m = DepthCrafter(synthetic_weights=True, cfgs=W.tiny_cfgs(), num_inference_steps=2, workspace_bytes=3 << 30)
    yield m
    m.pipeline.engine.close()


def test_harness_device_rows_are_the_same_under_either_search(tiny_plugin, tmp_path):
    """`eval_pcd.search: grid` on the `device_metrics=True` path, unsampled, from the resident points: the rows and the CSV of `search: brute`."""
    from unigeo_amd.harness import SyntheticGeometryDataset, evaluate
    ds = SyntheticGeometryDataset(clip_length=3, clip_overlap=1, input_size=(64, 64), num_frames=5)
    rows = {}
    for search in ("brute", "grid"):
        cfg = {"root": "x", "h": 64, "w": 64, "clip_length": 3, "clip_overlap": 1, "eval_depth": {"metric_names": ["Abs Rel"]},
               "eval_pcd": {"metric_names": ["acc", "comp", "nc1", "nc2"], "pcd_downsample_num": -1, "search": search}}
        rows[search], _ = evaluate(cfg, dataset=ds, model=tiny_plugin, save_dir=str(tmp_path / search), verbose=False, device_metrics=True)
    assert len(rows["brute"]) == len(rows["grid"]) == 3
    for b, g in zip(rows["brute"], rows["grid"]):
        for k in ("acc", "comp", "nc1", "nc2", "acc_med", "comp_med", "nc1_med", "nc2_med"):
            assert np.isfinite(b[k]) and np.float64(b[k]).tobytes() == np.float64(g[k]).tobytes(), k
    assert (tmp_path / "brute" / "metrics.csv").read_text() == (tmp_path / "grid" / "metrics.csv").read_text()
