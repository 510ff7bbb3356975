"""GPU: ug_eval_pcd_scores and ug_op_voxel_set (kernels/pcd.hip k_pcd_count_below, kernels/voxel.hip) against the numpy
mirror and the independent oracle of tests/pcd_score_fixtures.py.  The device returns integer counts, so every comparison is on equality; the
fixture's margins (no distance within 1e-9 of a threshold, no coordinate within 1e-9 of a cell face) keep the last-place differences between the
device's and the mirror's ICP from moving a count.  Every case runs on a few thousand points."""
import ctypes as C
import math

import numpy as np
import pytest

from pcd_fixtures import depth_scene
from pcd_score_fixtures import THRESHOLDS, VOXEL_SIZES, assert_conditions, names, oracle_scores, py_voxel_hash, py_voxel_pack, score_scene

pytestmark = pytest.mark.gpu

f32 = np.float32
OLD_KEYS = ("acc", "comp", "nc1", "nc2", "acc_med", "comp_med", "nc1_med", "nc2_med", "n_points", "icp_iterations", "icp_fitness", "icp_rmse",
            "transformation", "pred_scale", "gt_scale", "pred_shift_z", "gt_shift_z", "pred_pcd", "gt_pcd")
NEW_KEYS = ["score_counts", "voxel_counts"] + [f"{w}@{t}" for w in ("prec", "recall", "fscore") for t in names(THRESHOLDS)] + \
    [f"iou@{v}" for v in names(VOXEL_SIZES)]
SAMPLE = {False: 700, True: 1500}      # points kept of the about 1200 masked (host prediction) / 5800 valid (resident) ones


def _M():
    from unigeo_amd.harness import metrics
    return metrics


_INPUTS, _MIRROR = {}, {}


def _inputs(engine, seed, resident):
    """(pred for the mirror, pred for the device, gt, mask, rgb); the resident case leaves the device's own world points on the device and hands
    the mirror the float32 points it made"""
    if resident:
        d_pred, d_gt, poses, K = depth_scene((2, 48, 64), 20 + seed)
        noisy = (0.7 * d_gt + 0.3).astype(f32) + (d_pred - d_pred.mean()) * f32(0.02)
        gt = _M().world_points_from_depth(d_gt, d_gt, poses, K)[0]
        pts, _ = engine.pcd_world_points(d_gt, poses, K, pred=noisy, return_points=True)
        if (seed, True) not in _INPUTS:
            _INPUTS[seed, True] = pts, gt, d_gt > 0, np.random.default_rng(seed).uniform(size=d_gt.shape + (3,)).astype(f32)
        pts, gt, mask, rgb = _INPUTS[seed, True]
        return pts, None, gt, mask, rgb
    pred, gt, mask, rgb = score_scene(seed)
    return pred, pred, gt, mask, rgb


def _mirror(seed, sampling, resident, inputs):
    """the host evaluation, once per (seed, sampling, resident): either search returns the same neighbours"""
    key = seed, sampling, resident
    if key not in _MIRROR:
        pred, _, gt, mask, rgb = inputs
        _MIRROR[key] = _M().pcd_evaluation(pred, gt, mask, rgb, downsample_num=SAMPLE[resident], seed=3, sampling=sampling,
                                           fscore_thresholds=THRESHOLDS, voxel_sizes=VOXEL_SIZES)
    return _MIRROR[key]


def _bytes_equal(a, b, key):
    if isinstance(a, dict):               # search_stats: the searches did the same work; the workspace peak includes the new tables
        assert {k: v for k, v in a.items() if k != "workspace_peak_bytes"} == {k: v for k, v in b.items() if k != "workspace_peak_bytes"}, key
    elif isinstance(a, tuple):
        for x, y in zip(a, b):
            _bytes_equal(x, y, key)
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key
    else:
        assert type(a) is type(b) and np.float64(a).tobytes() == np.float64(b).tobytes(), key


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("sampling", ["random", "fps"])
@pytest.mark.parametrize("search", ["brute", "grid"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_device_counts_what_the_mirror_counts(engine, seed, search, sampling, resident):
    inputs = _inputs(engine, seed, resident)
    _, dev_pred, gt, mask, rgb = inputs
    kw = dict(downsample_num=SAMPLE[resident], seed=3, sampling=sampling, search=search)
    plain = engine.eval_pcd(dev_pred, gt, mask, rgb, **kw)
    res = engine.eval_pcd(dev_pred, gt, mask, rgb, fscore_thresholds=THRESHOLDS, voxel_sizes=VOXEL_SIZES, **kw)
    ref = _mirror(seed, sampling, resident, inputs)
    o_dev, o_ref = oracle_scores(res), oracle_scores(ref)
    print(f"seed {seed} {search} {sampling} resident={resident}: n {res['n_points']} iterations {res['icp_iterations']} / {ref['icp_iterations']} "
          f"counts {res['score_counts'].tolist()} {res['voxel_counts'].tolist()} margins {o_dev['distance_margin']:.3g} {o_dev['face_margin']:.3g}")
    assert_conditions(o_dev, bands=not resident)
    assert_conditions(o_ref, bands=not resident)
    assert res["n_points"] == ref["n_points"] == SAMPLE[resident]
    assert set(res) == set(plain) | set(NEW_KEYS)
    for k in plain:                                   # the existing outputs do not move when the options are given
        _bytes_equal(plain[k], res[k], k)
    for k in ("score_counts", "voxel_counts"):
        assert res[k].dtype == np.int64 and res[k].shape == ref[k].shape
        assert np.array_equal(res[k], o_dev[k]), k     # the oracle on the device's own clouds and transformation
        assert np.array_equal(res[k], ref[k]), k       # the mirror
    for k in NEW_KEYS[2:]:
        assert isinstance(res[k], float) and np.float64(res[k]).tobytes() == np.float64(ref[k]).tobytes(), k
    assert np.float32(res["recall@0.05"]) == np.float32(o_dev["score_counts"][1, 1] / res["n_points"])


def test_two_calls_return_the_same_integers(engine):
    pred, gt, mask, rgb = score_scene(1)
    for search in ("brute", "grid"):
        a, b = (engine.eval_pcd(pred, gt, mask, rgb, search=search, fscore_thresholds=THRESHOLDS, voxel_sizes=VOXEL_SIZES) for _ in range(2))
        assert a["n_points"] == int(mask.sum())          # unsampled: every masked point
        for k in NEW_KEYS:
            _bytes_equal(a[k], b[k], k)
        assert np.array_equal(a["score_counts"], oracle_scores(a)["score_counts"]) and np.array_equal(a["voxel_counts"], oracle_scores(a)["voxel_counts"])


# ------------------------------------------------------------------------------------------------------------------ the raw entry point
def _raw(engine, seed=0):
    from unigeo_amd._lib import PcdOptsC, PcdScoreOptsC, _ptr
    pred, gt, mask, _ = score_scene(seed)
    a = {"p": np.ascontiguousarray(pred), "g": np.ascontiguousarray(gt), "m": np.ascontiguousarray(mask.astype(np.uint8)), "o": PcdOptsC(),
         "so": PcdScoreOptsC(), "idx": np.ascontiguousarray(np.random.default_rng(4).choice(int(mask.sum()), 500, replace=False).astype(np.int64))}
    engine.lib.ug_pcd_opts_default(C.byref(a["o"]))
    engine.lib.ug_pcd_score_opts_default(C.byref(a["so"]))

    def scores(so, sc, vc, flags=0, eng=engine, out=None):
        out = np.zeros(32, np.float64) if out is None else out
        rc = eng.lib.ug_eval_pcd_scores(eng.ctx, _ptr(a["p"]), _ptr(a["g"]), _ptr(a["m"]), len(a["m"]), _ptr(a["idx"]), len(a["idx"]), C.byref(a["o"]),
                                        flags, _ptr(out), None, None, None, None, None, None if so is None else C.byref(so), _ptr(sc), _ptr(vc))
        return rc, out, eng.lib.ug_last_error(eng.ctx).decode()
    return a, scores


def test_the_default_options_are_empty_and_then_the_call_is_eval_pcd_ex(engine):
    from unigeo_amd._lib import _ptr
    a, scores = _raw(engine)
    so = a["so"]
    assert so.n_thresholds == 0 and so.n_voxel_sizes == 0 and not any(so.thresholds) and not any(so.voxel_sizes)
    for flags in (0, 2):
        ref, st_ref = np.zeros(32, np.float64), np.zeros(8, np.int64)
        pc_ref, gc_ref = np.zeros((500, 3), f32), np.zeros((500, 3), f32)
        assert engine.lib.ug_eval_pcd_ex(engine.ctx, _ptr(a["p"]), _ptr(a["g"]), _ptr(a["m"]), len(a["m"]), _ptr(a["idx"]), 500, C.byref(a["o"]), flags,
                                         _ptr(ref), _ptr(pc_ref), _ptr(gc_ref), None, None, _ptr(st_ref)) == 0
        for opts in (so, None):
            out, st = np.zeros(32, np.float64), np.zeros(8, np.int64)
            pc, gc = np.zeros((500, 3), f32), np.zeros((500, 3), f32)
            sc, vc = np.full(16, -7, np.int64), np.full(24, -7, np.int64)
            assert engine.lib.ug_eval_pcd_scores(engine.ctx, _ptr(a["p"]), _ptr(a["g"]), _ptr(a["m"]), len(a["m"]), _ptr(a["idx"]), 500,
                                                 C.byref(a["o"]), flags, _ptr(out), _ptr(pc), _ptr(gc), None, None, _ptr(st),
                                                 None if opts is None else C.byref(opts), _ptr(sc), _ptr(vc)) == 0
            assert out.tobytes() == ref.tobytes() and pc.tobytes() == pc_ref.tobytes() and gc.tobytes() == gc_ref.tobytes()
            assert st[:6].tobytes() == st_ref[:6].tobytes() and (sc == -7).all() and (vc == -7).all()      # nothing written for nothing asked
        assert np.isfinite(ref[:8]).all() and ref[8] == 500


def test_errors_are_returned_and_the_context_stays_usable(engine):
    from unigeo_amd._lib import Engine, PcdScoreOptsC
    a, scores = _raw(engine)
    sc, vc = np.zeros(16, np.int64), np.zeros(24, np.int64)

    def opts(taus=(), sizes=(), nt=None, nv=None):
        so = PcdScoreOptsC()
        for k, t in enumerate(taus):
            so.thresholds[k] = t
        for k, v in enumerate(sizes):
            so.voxel_sizes[k] = v
        so.n_thresholds, so.n_voxel_sizes = len(taus) if nt is None else nt, len(sizes) if nv is None else nv
        return so
    cases = [(opts([0.05]), None, vc, "score_counts"), (opts(sizes=[0.1]), sc, None, "voxel_counts"), (opts([0.05] * 8, nt=9), sc, vc, "n_thresholds"),
             (opts(nt=-1), sc, vc, "n_thresholds"), (opts(sizes=[0.1] * 4, nv=5), sc, vc, "n_voxel_sizes"), (opts([0.05, 0.0]), sc, vc, "threshold"),
             (opts([math.inf]), sc, vc, "threshold"), (opts(sizes=[math.nan]), sc, vc, "voxel size"), (opts(sizes=[-0.1]), sc, vc, "voxel size")]
    for so, s, v, word in cases:
        rc, _, err = scores(so, s, v)
        assert rc != 0 and word in err, (word, err)
    rc, _, err = scores(opts([0.05]), sc, vc, flags=4)
    assert rc != 0 and "0x4" in err
    rc, out, _ = scores(opts([0.05], [0.1]), sc, vc)                  # the context still works
    assert rc == 0 and out[8] == 500 and 0 < sc[0] < 500 and 0 < sc[1] < 500 and vc[2] > 0 and vc[3] == vc[0] + vc[1] - vc[2] and not sc[2:].any()
    good = sc.copy(), vc.copy()
    small = Engine(0, workspace_bytes=256 << 10, persist_bytes=1 << 20)      # a workspace too small: named with the bytes the call needs
    try:
        rc, _, err = scores(opts([0.05], [0.1]), sc, vc, eng=small)
        assert rc != 0 and "workspace is too small" in err and "needs" in err and "bytes" in err, err
        need = int(err.split("needs ")[1].split(" bytes")[0])
        assert 256 << 10 < need < 64 << 20
        assert small.op_voxel_set(np.zeros((3, 3)), np.ones((2, 3)), 0.5).tolist() == [1, 1, 0, 2, 0, 0]
        roomy = Engine(0, workspace_bytes=need, persist_bytes=1 << 20)       # and exactly that many bytes are enough (brute-force search)
        try:
            rc, _, err = scores(opts([0.05], [0.1]), sc, vc, eng=roomy)
            assert rc == 0, err
            assert sc.tobytes() == good[0].tobytes() and vc.tobytes() == good[1].tobytes()
        finally:
            roomy.close()
    finally:
        small.close()


def test_an_empty_mask_gives_zero_counts(engine):
    pred, gt, mask, rgb = score_scene(0)
    res = engine.eval_pcd(pred, gt, np.zeros_like(mask), rgb, fscore_thresholds=[0.05], voxel_sizes=[0.1])
    ref = _M().pcd_evaluation(pred, gt, np.zeros_like(mask), rgb, fscore_thresholds=[0.05], voxel_sizes=[0.1])
    assert res["n_points"] == 0 and not res["score_counts"].any() and not res["voxel_counts"].any()
    assert res["score_counts"].shape == ref["score_counts"].shape and res["voxel_counts"].shape == ref["voxel_counts"].shape
    assert all(math.isnan(res[k]) and math.isnan(ref[k]) for k in ("prec@0.05", "recall@0.05", "fscore@0.05", "iou@0.1"))
    with pytest.raises(ValueError, match="fscore_thresholds"):
        engine.eval_pcd(pred, gt, mask, rgb, fscore_thresholds=[0.05, 0.05])


# ------------------------------------------------------------------------------------------------------------------ the voxel table alone
def _set_counts(a, b, v):
    cell = lambda pts: {tuple(math.floor(c / v) for c in p) for p in np.asarray(pts, np.float64).reshape(-1, 3).tolist()}
    A, B = cell(a), cell(b)
    return [len(A), len(B), len(A & B), len(A | B), 0, 0]


def test_every_lane_on_one_slot(engine):
    one = np.tile(np.array([[0.31, -2.2, 7.7]]), (4096, 1))
    assert engine.op_voxel_set(one, one, 0.1).tolist() == [1, 1, 1, 1, 0, 0]
    assert engine.op_voxel_set(one, np.zeros((0, 3)), 0.1, capacity_log2=1).tolist() == [1, 0, 0, 1, 0, 0]
    assert engine.op_voxel_set(np.zeros((0, 3)), np.zeros((0, 3)), 0.1).tolist() == [0] * 6
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0.25 * (1 << 20), 0, 0], [0.05, 0.05, 0.05]])      # exact at a quarter: cell 2^20 is outside
    assert engine.op_voxel_set(bad, bad[:2], 0.25).tolist() == [1, 0, 0, 1, 3, 2]


def _wrapping_cells():
    rng = np.random.default_rng(9)
    cells = np.unique(rng.integers(-100, 101, (4000, 3)), axis=0)
    return cells[rng.permutation(len(cells))[:3000]]


def test_probing_wraps_past_the_end_of_the_table(engine):
    """3000 distinct cells in a forced table of 4096 slots (load 0.73).  More than w keys have their home in the last w slots, so linear probing
    must carry at least one of them past the end to slot 0: asserted from a restatement of the hash, as a condition on the seed."""
    cells = _wrapping_cells()
    assert len(cells) == 3000
    homes = np.array([py_voxel_hash(py_voxel_pack(*map(int, c))) & 4095 for c in cells])
    wraps = [w for w in range(1, 64) if int((homes >= 4096 - w).sum()) > w]
    assert wraps, "the seed no longer makes the occupied run wrap"
    v = 0.25
    pts = (cells + 0.5) * v
    order = np.random.default_rng(1).permutation(3000)
    a, b = pts[order[:2000]], np.concatenate([pts[order[1000:]], pts[order[1500:2500]]], 0)      # 1000 cells in both, some points twice
    want = _set_counts(a, b, v)
    assert want[:4] == [2000, 2000, 1000, 3000]
    got = engine.op_voxel_set(a, b, v, capacity_log2=12)
    assert got.tolist() == want
    assert engine.op_voxel_set(a, b, v, capacity_log2=12).tolist() == want          # whatever order the threads arrive in
    assert engine.op_voxel_set(a, b, v).tolist() == want                            # the production table
    pa, pb = np.unique(np.floor(a / v), axis=0), np.unique(np.floor(b / v), axis=0)
    assert (len(pa), len(pb)) == (got[0], got[1])


def test_a_full_table_is_an_error_return_and_the_context_stays_usable(engine):
    """The same 3000 cells in 2048 slots cannot fit.  The probe is a counted loop of `capacity` steps (read in the compiled kernel, DESIGN.md
    section 32): a thread that exhausts it flags the overflow and goes on, so the call ends and reports it."""
    cells = _wrapping_cells()
    v = 0.25
    pts = (cells + 0.5) * v
    with pytest.raises(RuntimeError, match="overflow"):
        engine.op_voxel_set(pts[:2000], pts[1000:], v, capacity_log2=11)
    assert engine.op_voxel_set(pts[:2000], pts[1000:], v, capacity_log2=12).tolist() == [2000, 2000, 1000, 3000, 0, 0]
    with pytest.raises(RuntimeError, match="capacity_log2"):
        engine.op_voxel_set(pts[:10], pts[:10], v, capacity_log2=31)
    with pytest.raises(RuntimeError, match="voxel_size"):
        engine.op_voxel_set(pts[:10], pts[:10], 0.0)
