"""Shared by tests/test_pcd_scores_cpu.py and tests/test_pcd_scores_gpu.py: a seeded scene for the threshold scores and
the voxel IoU, and an oracle for both that shares no code with what it checks - it imports neither the new functions of harness/metrics.py nor
the hash.  Distances come from a scipy k-d tree over the pre-ICP cloud moved with the transformation the call returned; voxels are a Python
set of math.floor tuples."""
import functools
import math

import numpy as np

THRESHOLDS = (0.02, 0.05, 0.1)
VOXEL_SIZES = (0.05, 0.1)
MARGIN = 1e-9


@functools.lru_cache(maxsize=None)
def score_scene(seed, n=1500):
    """-> (pred float32 [n,3], gt float32 [n,3], mask bool [n], rgb float32 [n,3]).  The ground truth lies on two perpendicular planes of a
    2 m box (a back wall z = 2.97 and a side wall x = 0.93: neither on a face of the voxel grids used here); the prediction is the ground
    truth plus N(0, 0.03) noise per coordinate, a tenth of its points thrown up to 0.5 m away; the mask drops about a fifth of the pixels."""
    rng = np.random.default_rng(1000 + seed)
    h = n // 2
    back = np.stack([rng.uniform(-1.0, 0.93, h), rng.uniform(-1.0, 1.0, h), np.full(h, 2.97)], 1)
    side = np.stack([np.full(n - h, 0.93), rng.uniform(-1.0, 1.0, n - h), rng.uniform(1.0, 2.97, n - h)], 1)
    gt = np.concatenate([back, side], 0)[rng.permutation(n)]
    pred = gt + rng.normal(0.0, 0.03, gt.shape)
    far = rng.choice(n, n // 10, replace=False)
    way = rng.normal(size=(len(far), 3))
    pred[far] += way / np.linalg.norm(way, axis=1, keepdims=True) * rng.uniform(0.0, 0.5, (len(far), 1))
    mask = rng.uniform(size=n) < 0.8
    rgb = rng.uniform(size=(n, 3)).astype(np.float32)
    out = pred.astype(np.float32), gt.astype(np.float32), mask, rgb
    for a in out:
        a.setflags(write=False)      # computed once, shared, left unchanged
    return out


def oracle_clouds(res):
    """The two float64 clouds the scores are taken on: the pre-ICP prediction of the result moved by its transformation, and the ground truth."""
    p, g = res["pred_pcd"][0].astype(np.float64), res["gt_pcd"][0].astype(np.float64)
    T = np.asarray(res["transformation"], np.float64)
    return p @ T[:3, :3].T + T[:3, 3], g


def oracle_scores(res, thresholds=THRESHOLDS, voxel_sizes=VOXEL_SIZES):
    """-> dict: ``score_counts`` [len(thresholds), 2], ``voxel_counts`` [len(voxel_sizes), 6], the derived ``prec`` / ``recall`` / ``iou`` lists,
    and the two margins: how close any distance comes to a threshold, and any coordinate to a cell face."""
    from scipy.spatial import cKDTree
    moved, g = oracle_clouds(res)
    n = len(moved)
    if n == 0:
        nan = [math.nan] * len(thresholds)
        return {"score_counts": np.zeros((len(thresholds), 2), np.int64), "voxel_counts": np.zeros((len(voxel_sizes), 6), np.int64), "prec": nan,
                "recall": nan, "iou": [math.nan] * len(voxel_sizes), "distance_margin": math.inf, "face_margin": math.inf}
    d_acc, d_comp = cKDTree(g).query(moved)[0], cKDTree(moved).query(g)[0]
    sc = np.array([[int(sum(1 for d in d_acc.tolist() if d < t)), int(sum(1 for d in d_comp.tolist() if d < t))] for t in thresholds], np.int64)
    dm = min(float(np.abs(d - t).min()) for d in (d_acc, d_comp) for t in thresholds) if len(thresholds) else math.inf
    vc, fm = [], math.inf
    for v in voxel_sizes:
        sets = []
        for cloud in (moved, g):
            cells, skipped = set(), 0
            for x, y, z in cloud.tolist():
                if not (math.isfinite(x / v) and math.isfinite(y / v) and math.isfinite(z / v)):
                    skipped += 1
                    continue
                c = (math.floor(x / v), math.floor(y / v), math.floor(z / v))
                if max(abs(i) for i in c) >= 1 << 20:
                    skipped += 1
                    continue
                cells.add(c)
            sets.append((cells, skipped))
            q = cloud / v
            fm = min(fm, float(np.abs(q - np.rint(q)).min()) * v)
        (a, sa), (b, sb) = sets
        vc.append([len(a), len(b), len(a & b), len(a | b), sa, sb])
    vc = np.array(vc, np.int64).reshape(len(voxel_sizes), 6)
    return {"score_counts": sc, "voxel_counts": vc, "prec": [c / n for c in sc[:, 0].tolist()], "recall": [c / n for c in sc[:, 1].tolist()],
            "iou": [(c[2] / c[3] if c[3] else math.nan) for c in vc.tolist()], "distance_margin": dm, "face_margin": fm}


def assert_conditions(o, bands=True):
    """What the fixture promises, on the oracle alone: no distance within 1e-9 of a threshold and no coordinate within 1e-9 of a cell face (so
    that roundings of the last place cannot move a count), and with ``bands`` a scene that is neither all right nor all wrong."""
    assert o["distance_margin"] > MARGIN and o["face_margin"] > MARGIN, (o["distance_margin"], o["face_margin"])
    if bands:
        k, j = THRESHOLDS.index(0.05), VOXEL_SIZES.index(0.1)
        assert 0.3 < o["prec"][k] < 0.95 and 0.3 < o["recall"][k] < 0.95, (o["prec"][k], o["recall"][k])
        assert 0.1 < o["iou"][j] < 0.7, o["iou"][j]


def names(values):
    return [format(float(v), "g") for v in values]


# ---- the voxel key and the hash, restated (tests of kernels/voxkey.h and of the table's probing)
M64 = (1 << 64) - 1


def py_voxel_index(x, v):
    """-> the cell or None, with Python floats (IEEE float64)"""
    try:
        q = x / v
    except ZeroDivisionError:
        return None
    if not math.isfinite(q):
        return None
    f = math.floor(q)
    return f if -(1 << 20) < f < (1 << 20) else None


def py_voxel_pack(ix, iy, iz):
    return ((ix + (1 << 20)) << 42) | ((iy + (1 << 20)) << 21) | (iz + (1 << 20))


def py_voxel_hash(x):
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & M64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & M64
    x ^= x >> 31
    return x
