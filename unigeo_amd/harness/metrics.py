"""Evaluation metrics and the CSV sink, restated from the reference:

* ``depth_evaluation``  <- ``/root/reference/metrics/eval_depth.py:6-246`` restricted to the call the harness makes
  (``eval.py:49``: ``align_with_lstsq=True`` + ``custom_mask``): mask 0 < gt < 80, least-squares scale/shift
  (``metrics/alignment.py:150-167``), then AbsRel / SqRel / RMSE / LogRMSE / delta thresholds on the custom mask;
  plus its median / L1-scale / metric alignment modes and the pre- and post-alignment clamps.
* ``depth_evaluation_in_global_coord`` <- ``/root/reference/metrics/eval_depth.py:250-441``: the aligned depth back-projected,
  moved into the world frame, and evaluated as the distance from the world origin.
* ``world_points_from_depth`` / ``pcd_evaluation`` <- ``/root/reference/metrics/eval_pcd.py:10-168`` with ``pcd_alignment.py``,
  ``metrics/utils.py:14-42`` and the Open3D calls it makes (point-to-point ICP, KNN normals) restated in numpy.
* ``normal_evaluation`` <- ``/root/reference/metrics/eval_normal.py:4-72``: angular error in degrees, mean / median /
  rmse / % under 5, 7.5, 11.25, 22.5, 30 degrees.
* ``MetricsManager``    <- ``/root/reference/metrics/save_utils.py:5-90``: one row per sequence, NaN for missing
  metrics, trailing ``Average`` row (NaN-skipping mean), ``%.5f``.
The lad / lad2 / disp_input modes of the reference function raise here (see ``depth_evaluation``); ``align_with_l1`` is the exact
minimiser of the objective lad / lad2 approach (``l1_fit``); ``align_space="disparity"`` is what ``disp_input``
means, with the function the reference never defines supplied (``disparity_to_depth``).
"""
import math
import os

import numpy as np


def _np(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


DEPTH_ALIGNMENTS = ("lstsq", "median", "scale", "metric", "l1")

L1_BITS, L1_MAX_STEPS, L1_MAX_TIES = 36, 64, 4096      # fixed-point bits of the prediction, and the two caps of the descent


def _l1_quantise(p):
    """``(q, E)``: ``E`` the smallest integer with ``max |p| < 2^E`` (0 for an all-zero ``p``), ``q = rint(p * 2^(36 - E))`` as int64.  The
    product is exact, so a value within 12 binades of the largest keeps every bit."""
    p = np.asarray(p, np.float32).reshape(-1)
    m = float(np.max(np.abs(p))) if p.size else 0.0
    E = math.frexp(m)[1] if m > 0 else 0
    return np.rint(p.astype(np.float64) * math.ldexp(1.0, L1_BITS - E)).astype(np.int64), E


def _l1_slopes(q, g64, j, down):
    """Every ``i`` with ``q_i != q_j`` -> (indices, integer weights ``|q_i - q_j|``, float64 slopes through point ``j``)."""
    dq = q - q[j]
    idx = np.nonzero(dq)[0]
    d = dq[idx]
    r = (g64[idx] - g64[j]) / (d.astype(np.float64) * down)
    return idx, np.abs(d), r + 0.0          # -0.0 + 0.0 = +0.0


def _l1_step(q, g64, j, down):
    """One pivot step: the lower weighted median ``S`` of the slopes through ``j`` and the indices whose slope equals it (index order);
    ``None`` when every ``q`` equals ``q_j``."""
    idx, w, r = _l1_slopes(q, g64, j, down)
    if idx.size == 0:
        return None
    o = np.argsort(r, kind="stable")
    cw = np.cumsum(w[o])
    S = r[o[int(np.argmax(cw >= cw[-1] - cw))]]
    return float(S), idx[r == S]


def _l1_vertex_holds(q, g64, z, S, down):
    """Is ``S`` optimal along the line of fits through ``z``: neither side of ``S`` holds more than half of the weight."""
    _, w, r = _l1_slopes(q, g64, z, down)
    B, A, W = int(w[r < S].sum()), int(w[r > S].sum()), int(w.sum())
    return B <= W - B and A <= W - A


def l1_fit(p, g):
    """The exact least-absolute-deviations fit ``min sum |s p_i + t - g_i|`` of float32 ``p`` against float32 ``g``
    -> ``(s, t, info)``, ``info = {j, k, steps, certified}``: the optimal line passes through points ``j`` and ``k`` (``k`` the lowest-index
    partner of the last step).  ``p`` is held as the integers ``q = rint(p * 2^(36 - E))``, so that every weight ``|q_i - q_j|`` and every
    sum of weights is an exact integer; a step from pivot ``j`` takes the lower weighted median of the slopes through ``j``, which minimises
    the objective along the line of fits through that point.  The descent starts at the lowest index holding the lower median of ``p``;
    at each vertex ``(j, S)`` every point ``z`` on the line (one per distinct ``q``, in index order) is asked whether ``S`` is also optimal
    along ITS line, and the first that says no becomes the pivot.  When all agree the vertex is the minimiser.  ``certified = 0``: one of
    the caps (64 steps, 4096 tied points) was met and the current vertex is returned.  No point: ``(0, 0)``; every ``q`` equal: ``s = 0``,
    ``t`` the lower median of ``g``."""
    p, g = np.asarray(p, np.float32).reshape(-1), np.asarray(g, np.float32).reshape(-1)
    n = p.size
    if n == 0:
        return 0.0, 0.0, {"j": -1, "k": -1, "steps": 0, "certified": 1}
    if n >= 1 << 26:
        raise ValueError("l1_fit: 2^26 points or more (the integer weights must sum below 2^63)")
    q, E = _l1_quantise(p)
    down, g64 = math.ldexp(1.0, E - L1_BITS), g.astype(np.float64)
    pivot = int(np.argmax(p == np.sort(p)[(n - 1) // 2]))
    step = _l1_step(q, g64, pivot, down)
    if step is None:
        return 0.0, float(np.sort(g)[(n - 1) // 2]), {"j": pivot, "k": -1, "steps": 0, "certified": 1}
    steps, certified = 1, 1
    while True:
        j, (S, tied) = pivot, step
        if tied.size > L1_MAX_TIES:
            certified = 0
            break
        _, first = np.unique(q[tied], return_index=True)          # the first occurrence of each distinct q; tied is in index order
        nxt = next((int(z) for z in tied[np.sort(first)] if not _l1_vertex_holds(q, g64, int(z), S, down)), None)
        if nxt is None:
            break
        if steps == L1_MAX_STEPS:
            certified = 0
            break
        pivot, step, steps = nxt, _l1_step(q, g64, nxt, down), steps + 1
    t = float(g64[j]) - S * (float(q[j]) * down)
    return S, t, {"j": j, "k": int(tied[0]), "steps": steps, "certified": certified}


def l1_objective(p, g, s, t):
    """``sum |s p_i + t - g_i|`` in float64 and plain index order, on the de-quantised prediction ``q * 2^(E - 36)`` that ``l1_fit`` fits."""
    g = np.asarray(g, np.float32).reshape(-1).astype(np.float64)
    if g.size == 0:
        return 0.0
    q, E = _l1_quantise(p)
    return float(np.cumsum(np.abs(float(s) * (q.astype(np.float64) * math.ldexp(1.0, E - L1_BITS)) + float(t) - g))[-1])


def _scale_l1(p, g):
    """The reference's ``align_with_scale_torch`` (``metrics/alignment.py:170-195``) in float64, sums in plain index order
    (``np.cumsum`` adds sequentially; ``np.sum`` would add pairwise).  The 1 / |residual| weights make the result move with
    the summation order alone at clip size, hence the fixed order."""
    p, g = p.astype(np.float64), g.astype(np.float64)
    s = (np.cumsum(g)[-1] / g.size) / (np.cumsum(p)[-1] / p.size)
    for _ in range(10):
        w = 1.0 / (np.abs(s * p - g) + 1e-8)
        s = np.cumsum(w * p * g)[-1] / np.cumsum(w * p * p)[-1]
    return float(s)


def _lstsq_f32(p, g, solve_dtype=np.float32):
    """The reference's ``align_with_lstsq_torch`` (``metrics/alignment.py:150-167``): numpy's least squares on the columns ``[p, 1]``
    -> float32 ``(s, t)``; ``(0, 0)`` for no pixel.  ``solve_dtype=np.float32`` solves in the precision of the values, as the reference
    does; ``np.float64`` solves the same system in double and rounds the answer once."""
    p, g = p.astype(solve_dtype), g.astype(solve_dtype)
    A = np.stack([p, np.ones_like(p)], 1)
    sol = np.linalg.lstsq(A, g[:, None], rcond=None)[0]
    return np.float32(sol[0, 0]), np.float32(sol[1, 0])


def _metric_values(p, g):
    """The eight metrics of the reference (``metrics/eval_depth.py:138-164``, again ``:384-408``) on the selected float32 values, plus
    ``valid_pixels``; no selected pixel gives zeros."""
    f32 = np.float32
    n = int(p.size)
    if n == 0:
        vals = [0, 0, 0, 0, 0, 0, 0, 0]
    else:
        abs_rel = float(np.mean(np.abs(p - g) / g, dtype=f32))
        sq_rel = float(np.mean((p - g) ** 2 / g, dtype=f32))
        rmse = float(np.sqrt(np.mean((p - g) ** 2, dtype=f32)))
        pc = np.maximum(p, f32(1e-5))
        log_rmse = float(np.sqrt(np.mean((np.log(pc) - np.log(g)) ** 2, dtype=f32)))
        ratio = np.maximum(pc / g, g / pc)
        th = [float(np.mean((ratio < k).astype(f32))) for k in (1.0, 1.25, 1.25 ** 2, 1.25 ** 3)]
        vals = [abs_rel, sq_rel, rmse, log_rmse] + th
    keys = ["Abs Rel", "Sq Rel", "RMSE", "Log RMSE", "delta < 1.", "delta < 1.25", "delta < 1.25^2", "delta < 1.25^3"]
    res = dict(zip(keys, vals))
    res["valid_pixels"] = n
    return res


DEPTH_ALIGN_SPACES = ("depth", "disparity")


def check_disp_clip_min(align_space, disp_clip_min, who="depth_evaluation"):
    """The two option checks every layer shares: a known ``align_space``; ``disp_clip_min`` finite and positive, and only in disparity space."""
    if align_space not in DEPTH_ALIGN_SPACES:
        raise ValueError(f"{who}: the alignment space must be one of {DEPTH_ALIGN_SPACES}, not {align_space!r}")
    if disp_clip_min is None:
        return
    try:
        c = float(disp_clip_min)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: disp_clip_min must be a finite positive number, not {disp_clip_min!r}") from None
    if isinstance(disp_clip_min, bool) or not (math.isfinite(c) and c > 0):
        raise ValueError(f"{who}: disp_clip_min must be a finite positive number, not {disp_clip_min!r}")
    if align_space != "disparity":
        raise ValueError(f"{who}: disp_clip_min floors the aligned disparity and needs the alignment space 'disparity'")


def disparity_to_depth(a, disp_clip_min=None):
    """Aligned float32 disparity -> float32 depth: with ``disp_clip_min = c``, ``a = c`` where ``a < c`` (a NaN stays
    NaN); then ``1 / a`` where ``a > 0``, else 0.  Without the floor this is the three-line ``depth2disparity`` the reference's
    ``disp_input`` branch calls and never defines."""
    a = np.asarray(a, np.float32)
    if disp_clip_min is not None:
        a = np.where(a < np.float32(disp_clip_min), np.float32(disp_clip_min), a)
    out = np.zeros(a.shape, np.float32)
    pos = a > 0
    out[pos] = np.float32(1) / a[pos]
    return out


def depth_evaluation(predicted_depth_original, ground_truth_depth_original, max_depth=80, custom_mask=None,
                     post_clip_min=None, post_clip_max=None, pre_clip_min=None, pre_clip_max=None,
                     align_with_lstsq=False, align_with_lad=False, align_with_lad2=False, metric_scale=False,
                     align_with_scale=False, disp_input=False, lr=1e-4, max_iters=1000, use_gpu=False, return_error_map=False,
                     align_with_l1=False, align_space="depth", disp_clip_min=None, **unsupported):
    """``depth_evaluation`` of the reference (``metrics/eval_depth.py:59-204``) -> ``(res, (s, t))``, with
    ``return_error_map=True`` ``(res, (s, t), error_map)``.

    On mask1 = ``gt > 0`` (and ``gt < max_depth`` unless that is ``None``): clamp the prediction to the pre-clip bounds,
    align, clamp to the post-clip bounds, apply the custom mask, compute the metrics.  The alignment keeps the
    reference's precedence: ``metric_scale`` (s = 1), then ``align_with_lstsq`` (scale and shift), then ``align_with_l1`` (the exact
    least-absolute-deviations scale and shift of ``l1_fit``, rounded once to float32; in the place the reference gives lad), then
    ``align_with_scale`` (Weiszfeld L1 scale, here in float64 and plain index order; clamped to >= 1e-3), then the
    default: ``s = median(gt) / median(pred)`` with ``torch.median``'s LOWER median, element ``(n - 1) // 2`` of the
    sorted values.  The error map is ``|s * pred + t - gt| / gt`` on mask1 and 0 elsewhere, from the ORIGINAL prediction
    (neither clamp applied), as the reference computes it.  No valid pixel: zero metrics and ``(s, t) = (1, 0)`` under
    ``metric_scale``, ``(0, 0)`` otherwise.

    Still rejected with ``NotImplementedError``: ``align_with_lad`` / ``align_with_lad2`` run a scipy BFGS and a
    1000-step Adam on a non-smooth objective, which gives no reproducible answer; ``disp_input`` calls ``depth2disparity``,
    which the reference defines nowhere, so its own call raises ``NameError``.  The objective lad / lad2 approach has an exact
    minimiser: ``align_with_l1`` returns it.  ``lr`` / ``max_iters`` (lad2 only) and
    ``use_gpu`` (tensor placement) are accepted and have no effect.  The flag ``disp_input`` keeps raising; what it means, with the
    missing function supplied, is ``align_space="disparity"``:

    ``align_space="disparity"``: the prediction is a DISPARITY.  On mask1 (from the original gt), with every
    operation one float32 rounding: ``p = clamp(pred, pre_clip)``, ``gd = 1 / (gt + 1e-8)``, ``(s, t)`` = the chosen alignment of ``p``
    against ``gd`` (each mode as above, same precedence), ``a = s * p + t``, with ``disp_clip_min = c`` ``a = max(a, c)``,
    ``d = 1 / a`` where ``a > 0`` else 0 (``disparity_to_depth``), ``d = clamp(d, post_clip)``, then the custom mask and the metrics
    against the REAL gt.  The error map is ``|d0 - gt| / gt`` on mask1, ``d0`` made the same way from ``a0 = pred * s + t`` of the
    original prediction (the floor applies, the clips do not).  ``align_space="depth"`` (the default) is everything above, unchanged;
    ``disp_clip_min`` with it, a ``disp_clip_min`` that is not finite and positive, or an unknown ``align_space`` is a ``ValueError``.
    """
    if align_with_lad or align_with_lad2 or disp_input or any(v for v in unsupported.values()):
        raise NotImplementedError("align_with_lad / align_with_lad2 (no reproducible optimum) and disp_input (undefined in the "
                                  "reference) are not restated")
    check_disp_clip_min(align_space, disp_clip_min)
    disparity = align_space == "disparity"
    f32 = np.float32
    pred = _np(predicted_depth_original).astype(np.float32).reshape(-1)
    gt = _np(ground_truth_depth_original).astype(np.float32).reshape(-1)
    cm = None if custom_mask is None else _np(custom_mask).astype(bool).reshape(-1)
    mask = (gt > 0) & (gt < max_depth) if max_depth is not None else gt > 0
    p, g = pred[mask], gt[mask]
    if pre_clip_min is not None:
        p = np.maximum(p, f32(pre_clip_min))
    if pre_clip_max is not None:
        p = np.minimum(p, f32(pre_clip_max))
    if disparity:
        real_g, g = g, f32(1) / (g + f32(1e-8))
    if metric_scale:
        s, t = f32(1), f32(0)
    elif align_with_lstsq:
        s, t = _lstsq_f32(p, g)
    elif align_with_l1:
        s, t = (f32(v) for v in l1_fit(p, g)[:2])
    elif p.size == 0:
        s, t = f32(0), f32(0)
    elif align_with_scale:
        s, t = max(_scale_l1(p, g), 1e-3), f32(0)
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            s, t = np.sort(g)[(g.size - 1) // 2] / np.sort(p)[(p.size - 1) // 2], f32(0)
    s_ret = float(s)
    s = f32(s)
    p = s * p + t
    if disparity:
        p, g = disparity_to_depth(p, disp_clip_min), real_g
    if post_clip_min is not None:
        p = np.maximum(p, f32(post_clip_min))
    if post_clip_max is not None:
        p = np.minimum(p, f32(post_clip_max))
    if cm is not None:
        sel = cm[mask]
        p, g = p[sel], g[sel]
    res = _metric_values(p, g)
    if not return_error_map:
        return res, (s_ret, float(t))
    emap = np.zeros(gt.shape, f32)
    p0 = pred[mask] * s + t
    emap[mask] = np.abs((disparity_to_depth(p0, disp_clip_min) if disparity else p0) - gt[mask]) / gt[mask]
    return res, (s_ret, float(t)), emap.reshape(np.shape(_np(ground_truth_depth_original)))


def _world_from_depth(pred_depth, gt_depth, cam2world, intrinsics, max_depth, pre_clip_min, pre_clip_max, post_clip_min, post_clip_max):
    """The first half of ``depth_evaluation_in_global_coord``, shared with ``world_points_from_depth``: mask1, fit 1 on the pre-clipped
    prediction, ``d = s_d * pred + t_d`` in float32 from the ORIGINAL prediction, the post clips, then the float64 back-projection with integer
    pixel indices and the world transform -> ``(world float64 [Nf,H,W,3], mask1 [Nf,H,W], (s_d, t_d) float32)``."""
    f32, f64 = np.float32, np.float64
    pred = _np(pred_depth).astype(f32)
    if pred.ndim == 2:
        pred = pred[None]
    nf, h, w = pred.shape
    gt = _np(gt_depth).astype(f32).reshape(pred.shape)
    poses, K = _np(cam2world).reshape(nf, 4, 4), _np(intrinsics).reshape(nf, 3, 3)
    mask = (gt > 0) & (gt < max_depth) if max_depth is not None else gt > 0
    p = pred[mask]
    if pre_clip_min is not None:
        p = np.maximum(p, f32(pre_clip_min))
    if pre_clip_max is not None:
        p = np.minimum(p, f32(pre_clip_max))
    s_d, t_d = _lstsq_f32(p, gt[mask], np.float64)
    d = s_d * pred + t_d
    if post_clip_min is not None:
        d = np.maximum(d, f32(post_clip_min))
    if post_clip_max is not None:
        d = np.minimum(d, f32(post_clip_max))
    col, row = np.meshgrid(np.arange(w), np.arange(h), indexing="xy")
    world = np.empty((nf, h, w, 3), f64)
    for i in range(nf):
        z = d[i].astype(f64)
        x = (col - f64(K[i, 0, 2])) * z / f64(K[i, 0, 0])
        y = (row - f64(K[i, 1, 2])) * z / f64(K[i, 1, 1])
        cam = np.stack((x, y, z), axis=-1).reshape(-1, 3)
        world[i] = (cam @ poses[i][:3, :3].T + poses[i][:3, 3][:, None].T).reshape(h, w, 3)
    return world, mask, (s_d, t_d)


def world_points_from_depth(pred_depth, gt_depth, cam2world, intrinsics, max_depth=80, pre_clip_min=None, pre_clip_max=None,
                            post_clip_min=None, post_clip_max=None):
    """World points of a predicted depth -> ``(pts float32 [T,H,W,3], (s_d, t_d))``: the first half of
    ``depth_evaluation_in_global_coord`` - least-squares fit on mask1, aligned and post-clipped float32 depth of every pixel, float64
    back-projection and world transform - with each coordinate rounded once to float32."""
    world, _, (s_d, t_d) = _world_from_depth(pred_depth, gt_depth, cam2world, intrinsics, max_depth, pre_clip_min, pre_clip_max,
                                             post_clip_min, post_clip_max)
    return world.astype(np.float32), (float(s_d), float(t_d))


# ---------------------------------------------------------------------------------------------------------------------------------
# Point-cloud evaluation: /root/reference/metrics/eval_pcd.py:10-168 with pcd_alignment.py, metrics/utils.py:14-42
# and the Open3D calls (registration_icp, estimate_normals) restated in numpy.
PCD_KEYS = ("acc", "comp", "nc1", "nc2", "acc_med", "comp_med", "nc1_med", "nc2_med")


def _lower_median(a):
    """``torch.nanmedian`` of finite values: element ``(n - 1) // 2`` of the sorted array."""
    k = (a.shape[0] - 1) // 2
    return np.partition(a, k, axis=0)[k]


def pcd_align(p, g):
    """``Regr3D_t_ScaleShiftInv(norm_mode=False, gt_scale=True)`` plus ``eval_pcd.py:67-69`` on the masked float32 points ``p`` (prediction)
    and ``g`` (ground truth), ``[n,3]`` -> ``(p', g', (pred_scale, gt_scale, pred_shift_z, gt_shift_z))``, everything float32.  The norms
    behind the two scales are taken in float64 from the float32 differences and rounded once."""
    f32 = np.float32
    p, g = np.array(p, f32), np.array(g, f32)
    pz, gz = _lower_median(p[:, 2]), _lower_median(g[:, 2])
    p[:, 2] -= pz
    g[:, 2] -= gz

    def scale(x):
        diff = (x - _lower_median(x)).astype(np.float64)
        return _lower_median(np.sqrt((diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]).astype(f32))
    gs, ps = scale(g), np.clip(scale(p), f32(1e-3), f32(1e3))
    p *= f32(gs) / f32(ps)
    p[:, 2] += gz
    g[:, 2] += gz
    return p, g, (ps, gs, pz, gz)


def _d2(q, t):
    dx, dy, dz = q[:, None, 0] - t[None, :, 0], q[:, None, 1] - t[None, :, 1], q[:, None, 2] - t[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def nn_brute(q, t, chunk=1 << 22):
    """Nearest target of every query, float64 ``[n,3]`` each -> ``(distance float64, index)``: the smallest
    ``(dx*dx + dy*dy) + dz*dz``, ties to the lowest index; the distance is its square root."""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    idx, dist = np.empty(len(q), np.int64), np.empty(len(q), np.float64)
    step = max(1, chunk // max(1, len(t)))
    for a in range(0, len(q), step):
        d2 = _d2(q[a:a + step], t)
        i = np.argmin(d2, axis=1)
        idx[a:a + step], dist[a:a + step] = i, np.sqrt(d2[np.arange(len(i)), i])
    return dist, idx


def _nn(q, t):
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return nn_brute(q, t)
    return cKDTree(t).query(q)


def knn_brute(pts, k, chunk=1 << 22):
    """The ``min(k, n)`` nearest points of every point in its own cloud, itself included, ordered by (squared distance, index) ->
    ``[n, min(k, n)]`` indices."""
    pts = np.asarray(pts, np.float64)
    n = len(pts)
    k = min(k, n)
    out = np.empty((n, k), np.int64)
    step = max(1, chunk // max(1, n))
    for a in range(0, n, step):
        d2 = _d2(pts[a:a + step], pts)
        if k < n:          # keep only what can be among the k nearest, then sort that stably; a tie at the k-th distance sorts the whole row
            kth = np.partition(d2, k - 1, axis=1)[:, k - 1]
            keep = d2 <= kth[:, None]
            if (keep.sum(1) == k).all():
                cols = np.nonzero(keep)[1].reshape(-1, k)
                o = np.argsort(np.take_along_axis(d2, cols, 1), axis=1, kind="stable")
                out[a:a + step] = np.take_along_axis(cols, o, 1)
                continue
        out[a:a + step] = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return out


def _tree():
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return None
    return cKDTree


_TREE_SLACK = 1.0 - 1e-9      # the tree's own distances carry a few float64 roundings; a row must clear its radius by far more than that


def nn_grid(q, t, extra=16):
    """``nn_brute(q, t)`` exactly, from a host-side index: ``extra`` candidates per query from a k-d tree over the
    targets, re-ranked by ``(dx*dx + dy*dy) + dz*dz`` and the index as ``nn_brute`` ranks them.  A row is accepted when its winner
    lies inside the tree's radius (the distance of the farthest candidate, less a slack), so that no target outside the candidates can
    beat or tie it; every other row (a tie that fills the candidates, a non-finite query) is redone by ``nn_brute``.  Without scipy, or
    with a non-finite target, this is ``nn_brute``."""
    q, t = np.asarray(q, np.float64).reshape(-1, 3), np.asarray(t, np.float64).reshape(-1, 3)
    tree = _tree()
    if tree is None or len(q) == 0 or len(t) == 0 or not np.isfinite(t).all():      # numpy's argmin stops at a NaN distance: leave such a target to it
        return nn_brute(q, t)
    fin = np.arange(len(t))
    idx, dist = np.zeros(len(q), np.int64), np.full(len(q), np.inf)
    ok = np.zeros(len(q), bool)
    rows = np.nonzero(np.isfinite(q).all(1))[0]
    if len(rows):
        kk = min(extra, len(fin))
        dt, it = tree(t[fin]).query(q[rows], k=kk)
        dt, it = dt.reshape(len(rows), kk), fin[it.reshape(len(rows), kk)]
        d = q[rows][:, None, :] - t[it]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        o = np.lexsort((it, d2), axis=1)[:, 0]
        ar = np.arange(len(rows))
        best, bi = d2[ar, o], it[ar, o]
        radius = dt[:, -1] * _TREE_SLACK
        good = np.isfinite(best) & ((kk == len(fin)) | (best < radius * radius))
        idx[rows[good]], dist[rows[good]] = bi[good], np.sqrt(best[good])
        ok[rows[good]] = True
    if not ok.all():
        dist[~ok], idx[~ok] = nn_brute(q[~ok], t)
    return dist, idx


def knn_grid(pts, k, extra=16):
    """``knn_brute(pts, k)`` exactly, from the same index: ``min(k, n) + extra`` candidates per point, re-ranked by (squared distance,
    index); a row is accepted when its last kept neighbour lies inside the tree's radius, else it is redone by brute force.  A cloud with
    a non-finite point, and a host without scipy, go to ``knn_brute``."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    n = len(pts)
    k = min(k, n)
    tree = _tree()
    if tree is None or n == 0 or not np.isfinite(pts).all():
        return knn_brute(pts, k)
    kk = min(k + extra, n)
    dt, it = tree(pts).query(pts, k=kk)
    dt, it = dt.reshape(n, kk), it.reshape(n, kk)
    d = pts[:, None, :] - pts[it]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    o = np.lexsort((it, d2), axis=1)[:, :k]
    out = np.take_along_axis(it, o, 1).astype(np.int64)
    radius = dt[:, -1] * _TREE_SLACK
    last = np.take_along_axis(d2, o[:, -1:], 1)[:, 0]
    good = (kk == n) | (last < radius * radius)
    for r in np.nonzero(~good)[0]:
        out[r] = np.argsort(_d2(pts[r:r + 1], pts)[0], kind="stable")[:k]
    return out


def knn_normals(pts, knn=30, knn_fn=None):
    """Open3D's ``estimate_normals()`` with its default KNN search: the unit eigenvector of the smallest eigenvalue of the float64 covariance
    of the ``min(knn, n)`` nearest points about their mean; ``(0, 0, 1)`` with fewer than 3 points.  The sign is free.  ``knn_fn`` finds the
    lists (default ``knn_brute``)."""
    pts = np.asarray(pts, np.float64)
    n = len(pts)
    if min(n, knn) < 3:
        return np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))
    nb = pts[(knn_fn or knn_brute)(pts, knn)]
    c = nb - nb.mean(1, keepdims=True)
    cov = np.einsum("nki,nkj->nij", c, c) / nb.shape[1]
    return np.linalg.eigh(cov)[1][:, :, 0]


def _move(T, p):
    """``((r0 x + r1 y) + r2 z) + t`` per coordinate, float64."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)


def umeyama_rigid(src, dst):
    """Least-squares rigid ``dst ~ R src + t`` (Umeyama without scaling) -> 4x4; the identity for no point."""
    U4 = np.eye(4)
    if len(src) == 0:
        return U4
    ms, md = src.mean(0), dst.mean(0)
    H = (dst - md).T @ (src - ms) / len(src)
    U, _, Vt = np.linalg.svd(H)
    S = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0])
    R = U @ S @ Vt
    U4[:3, :3], U4[:3, 3] = R, md - R @ ms
    return U4


def icp_point_to_point(src, dst, threshold, max_iteration=30, nn=_nn):
    """Open3D's ``registration_icp`` with ``TransformationEstimationPointToPoint``, identity start, relative fitness / rmse 1e-6 ->
    ``(T, iterations, fitness, inlier_rmse, history)``; ``history`` lists ``(fitness, rmse)`` of every evaluation."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)

    def evaluate(T):
        moved = _move(T, src)
        if len(src) == 0 or len(dst) == 0:
            return 0.0, 0.0, moved[:0], dst[:0]
        d, i = nn(moved, dst)
        ok = d < threshold
        nc = int(ok.sum())
        return nc / len(src), (math.sqrt(float((d[ok] * d[ok]).sum()) / nc) if nc else 0.0), moved[ok], dst[i[ok]]
    T = np.eye(4)
    fit, rmse, s, d = evaluate(T)
    hist, it = [(fit, rmse)], 0
    for it in range(1, max_iteration + 1):
        T = umeyama_rigid(s, d) @ T
        prev = (fit, rmse)
        fit, rmse, s, d = evaluate(T)
        hist.append((fit, rmse))
        if abs(prev[0] - fit) < 1e-6 and abs(prev[1] - rmse) < 1e-6:
            break
    return T, it, fit, rmse, hist


# ---- precision / recall / F-score at distance thresholds and the voxel IoU
PCD_MAX_THRESHOLDS, PCD_MAX_VOXEL_SIZES = 8, 4      # the arrays of ug_pcd_score_opts
VOXEL_HALF = 1 << 20                                # a cell index lies in (-2^20, 2^20): kernels/voxkey.h


def pcd_score_names(values, what, limit):
    """The configured thresholds or voxel sizes -> ``(float values, their names)``; a name is ``format(x, "g")``.  At most ``limit``
    real numbers, each positive and finite, no two with the same name: anything else is a ``ValueError``."""
    if isinstance(values, (str, bytes)) or not hasattr(values, "__iter__"):
        raise ValueError(f"{what} must be a list of positive finite numbers, not {values!r}")
    vals = []
    for v in values:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{what}: {v!r} is not a number")
        v = float(v)
        if not (v > 0.0 and math.isfinite(v)):
            raise ValueError(f"{what}: {v!r} is not positive and finite")
        vals.append(v)
    if len(vals) > limit:
        raise ValueError(f"{what}: at most {limit} values, not {len(vals)}")
    names = [format(v, "g") for v in vals]
    if len(set(names)) != len(names):
        raise ValueError(f"{what}: two values are written the same way: {names}")
    return vals, names


def pcd_threshold_values(names, counts, n):
    """``prec@t = n_prec / n``, ``recall@t = n_rec / n`` and ``fscore@t = 2 P R / (P + R)`` (0 when ``P + R == 0``) in float64 from the integer
    counts ``[len(names), 2]``; NaN for ``n == 0``.  The device path forms its values here too."""
    res = {}
    for name, (n_prec, n_rec) in zip(names, np.asarray(counts, np.int64).reshape(-1, 2).tolist()):
        if n == 0:
            P = R = F = math.nan
        else:
            P, R = float(n_prec) / float(n), float(n_rec) / float(n)
            F = 0.0 if P + R == 0.0 else 2.0 * P * R / (P + R)
        res.update({f"prec@{name}": P, f"recall@{name}": R, f"fscore@{name}": F})
    return res


def pcd_threshold_scores(d_acc, d_comp, thresholds):
    """Precision, recall and F-score at distance thresholds (Tanks and Temples) -> ``prec@t``, ``recall@t``, ``fscore@t`` per threshold and
    ``score_counts`` int64 ``[len(thresholds), 2]``.  ``d_acc[i]`` is the distance of prediction ``i`` to its nearest ground-truth point,
    ``d_comp[j]`` that of ground-truth point ``j`` to its nearest prediction: the arrays ``acc`` and ``comp`` are the means of.
    ``n_prec = #{d_acc < t}``, ``n_rec = #{d_comp < t}``, both strict; a NaN distance is not below.

    ``np.float32(recall@0.05)`` is the reference's ``completion_ratio(gt, rec)`` with its default ``dist_th=0.05``
    (``metrics/utils.py:7-11``, called nowhere there): the float32 mean of a 0 / 1 array is that quotient rounded once, as long as the
    count stays below 2^24."""
    taus, names = pcd_score_names(thresholds, "fscore_thresholds", PCD_MAX_THRESHOLDS)
    d1, d2 = np.asarray(d_acc, np.float64).reshape(-1), np.asarray(d_comp, np.float64).reshape(-1)
    counts = np.zeros((len(taus), 2), np.int64)
    with np.errstate(invalid="ignore"):
        for k, t in enumerate(taus):
            counts[k] = int(np.count_nonzero(d1 < t)), int(np.count_nonzero(d2 < t))
    res = pcd_threshold_values(names, counts, len(d1))
    res["score_counts"] = counts
    return res


def voxel_keys(pts, voxel_size):
    """The sorted distinct packed cells of a cloud ``[n,3]`` and how many points were skipped.  The cell is ``floor(x / v)`` per axis, each
    step one float64 operation, from the world origin; a point with a non-finite coordinate or a cell outside ``(-2^20, 2^20)`` is
    skipped.  Packed as ``kernels/voxkey.h`` packs it: ``((ix + 2^20) << 42) | ((iy + 2^20) << 21) | (iz + 2^20)``."""
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        f = np.floor(p / np.float64(voxel_size))
        keep = ((f > -float(VOXEL_HALF)) & (f < float(VOXEL_HALF))).all(1)      # a NaN fails both
    i = (f[keep].astype(np.int64) + VOXEL_HALF).astype(np.uint64)
    keys = (i[:, 0] << np.uint64(42)) | (i[:, 1] << np.uint64(21)) | i[:, 2]
    return np.unique(keys), int(len(p) - np.count_nonzero(keep))


def voxel_iou(pred, gt, voxel_size):
    """Occupancy IoU of two clouds on one voxel grid of edge ``voxel_size`` anchored at the world origin -> ``(iou, counts)``:
    ``counts`` int64 ``[6]`` = cells of the prediction, of the ground truth, of both, of either, skipped predictions, skipped ground-truth
    points; ``iou = both / either`` in float64, NaN when neither cloud has a cell.

    UNPINNED: the reference's ``compute_iou`` (``metrics/utils.py:45-60``) is called nowhere and takes Open3D voxel grids, each with its own
    origin (the cloud's minimum bound), so their index sets are not comparable; open3d is not installed.  One common origin is a
    deliberate difference."""
    v = float(voxel_size)
    if not (v > 0.0 and math.isfinite(v)):
        raise ValueError(f"voxel_iou: voxel_size must be positive and finite, not {voxel_size!r}")
    kp, sp = voxel_keys(pred, v)
    kg, sg = voxel_keys(gt, v)
    both = int(len(np.intersect1d(kp, kg, assume_unique=True)))
    either = len(kp) + len(kg) - both
    counts = np.array([len(kp), len(kg), both, either, sp, sg], np.int64)
    return (float(both) / float(either) if either else math.nan), counts


def pcd_voxel_values(names, counts):
    """``iou@v = both / either`` in float64 from the integer counts ``[len(names), 6]``, NaN for an empty union."""
    return {f"iou@{name}": (float(c[2]) / float(c[3]) if c[3] else math.nan)
            for name, c in zip(names, np.asarray(counts, np.int64).reshape(-1, 6).tolist())}


def _pcd_extra_scores(d_acc, d_comp, pred_pts, gt_pts, fscore_thresholds, voxel_sizes):
    res = {}
    if len(fscore_thresholds):
        res.update(pcd_threshold_scores(d_acc, d_comp, fscore_thresholds))
    if len(voxel_sizes):
        vs, names = pcd_score_names(voxel_sizes, "voxel_sizes", PCD_MAX_VOXEL_SIZES)
        counts = np.stack([voxel_iou(pred_pts, gt_pts, v)[1] for v in vs], 0)
        res.update(pcd_voxel_values(names, counts))
        res["voxel_counts"] = counts
    return res


def pcd_scores(gt_pts, pred_pts, gt_normals, pred_normals, nn=_nn, fscore_thresholds=(), voxel_sizes=()):
    """``accuracy`` and ``completion`` of ``metrics/utils.py:14-42`` -> the eight reference keys; with ``fscore_thresholds`` / ``voxel_sizes``
    also the keys of ``pcd_threshold_scores`` over the same two distance arrays and ``iou@v`` / ``voxel_counts``."""
    d1, i1 = nn(pred_pts, gt_pts)
    d2, i2 = nn(gt_pts, pred_pts)
    n1 = np.abs(np.sum(gt_normals[i1] * pred_normals, axis=-1))
    n2 = np.abs(np.sum(gt_normals * pred_normals[i2], axis=-1))
    res = {"acc": float(np.mean(d1)), "comp": float(np.mean(d2)), "nc1": float(np.mean(n1)), "nc2": float(np.mean(n2)),
           "acc_med": float(np.median(d1)), "comp_med": float(np.median(d2)), "nc1_med": float(np.median(n1)), "nc2_med": float(np.median(n2))}
    res.update(_pcd_extra_scores(d1, d2, pred_pts, gt_pts, fscore_thresholds, voxel_sizes))
    return res


def pcd_metrics_from_clouds(p, g, threshold=0.1, knn=30, max_iteration=30, nn=_nn, knn_fn=None, fscore_thresholds=(), voxel_sizes=()):
    """ICP, normals and scores of two aligned float32 clouds ``[n,3]`` -> the eight keys plus the ICP record; NaN scores for no point.
    ``nn`` / ``knn_fn`` do the searches (defaults: the k-d tree or ``nn_brute``, and ``knn_brute``).  ``fscore_thresholds`` / ``voxel_sizes``
    as in ``pcd_scores``: scored on the moved prediction against the ground truth."""
    p64, g64 = np.asarray(p, np.float32).astype(np.float64), np.asarray(g, np.float32).astype(np.float64)
    if len(p64) == 0:
        res = {k: math.nan for k in PCD_KEYS}
        res.update(_pcd_extra_scores(p64[:, 0], p64[:, 0], p64, g64, fscore_thresholds, voxel_sizes))
        res.update(icp_iterations=0, icp_fitness=0.0, icp_rmse=0.0, transformation=np.eye(4))
        return res
    T, it, fit, rmse, hist = icp_point_to_point(p64, g64, threshold, max_iteration, nn)
    moved = _move(T, p64)
    res = pcd_scores(g64, moved, knn_normals(g64, knn, knn_fn), knn_normals(moved, knn, knn_fn), nn, fscore_thresholds, voxel_sizes)
    res.update(icp_iterations=it, icp_fitness=fit, icp_rmse=rmse, transformation=T, icp_history=hist)
    return res


def pcd_sample_indices(n, downsample_num, seed):
    """The sampled positions among the ``n`` masked points: ``default_rng(seed).choice`` without replacement when
    ``0 < downsample_num < n``, else ``None`` (every point)."""
    if 0 < downsample_num < n:
        return np.random.default_rng(seed).choice(n, downsample_num, replace=False)
    return None


def pcd_fps_indices(pts, k):
    """Farthest-point sampling of a float32 cloud ``[n,3]`` -> ``(idx int64 [k], sel_dist float32 [k])``, the statement
    that ``k_pcd_fps`` follows operation by operation.  ``m[j]`` starts at ``+inf`` for a point with three finite coordinates, else ``-1``.
    Step ``i``: ``s = argmax m`` (ties to the lowest index), ``idx[i] = s``, ``sel_dist[i] = m[s]``, then ``m[j] = d if d < m[j]`` with
    ``d = (dx*dx + dy*dy) + dz*dz``, every operation one float32 rounding, never fused; a NaN ``d`` leaves ``m[j]`` alone, so a non-finite
    point is never picked while a finite one remains.  Step 0 picks the first finite point.

    UNPINNED: this restates ``pytorch3d.ops.sample_farthest_points`` (``random_start_point=False``: start at index 0; each next point the
    argmax of the running minimum squared distance, first maximum on ties) from its documented behaviour; pytorch3d is not installed here, so
    neither the start index nor the tie rule has been compared against it."""
    f32 = np.float32
    p = np.ascontiguousarray(np.asarray(pts, f32).reshape(-1, 3))
    n, k = len(p), int(k)
    if not 0 < k <= n:
        raise ValueError(f"pcd_fps_indices: k must be 1 .. n ({k} of {n})")
    x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    m = np.where(np.isfinite(x) & np.isfinite(y) & np.isfinite(z), f32(np.inf), f32(-1)).astype(f32)
    idx, sel = np.empty(k, np.int64), np.empty(k, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(k):
            s = int(np.argmax(m))          # the first of equal maxima
            idx[i], sel[i] = s, m[s]
            dx, dy, dz = x - x[s], y - y[s], z - z[s]
            d = (dx * dx + dy * dy) + dz * dz
            np.copyto(m, d, where=d < m)
    return idx, sel


def pcd_sample_indices_fps(p, g, downsample_num):
    """Farthest-point sampling of each aligned cloud on its own, as the reference's disabled branch (``metrics/eval_pcd.py:92-93``) ->
    ``(idx_pred, idx_gt)`` when ``0 < downsample_num < n``, else ``None`` (every point)."""
    if 0 < downsample_num < len(p):
        return pcd_fps_indices(p, downsample_num)[0], pcd_fps_indices(g, downsample_num)[0]
    return None


def pcd_evaluation(pred_pts, gt_pts, masks, rgbs=None, threshold=0.1, downsample_num=-1, seed=0, knn=30, max_iteration=30, sampling="random",
                   search="brute", fscore_thresholds=(), voxel_sizes=()):
    """``pcd_evaluation`` of the reference (``metrics/eval_pcd.py:10-168``) -> dict: masked selection in pixel order,
    ``pcd_align``, seeded downsampling (the reference draws from the unseeded global generator and raises when ``downsample_num`` exceeds the
    point count; here that uses every point), point-to-point ICP from the identity, KNN normals, ``accuracy`` / ``completion``.
    ``pred_pcd`` / ``gt_pcd`` are ``(points float32 [n,3], colours float32 [n,3])`` taken before ICP (zeros without ``rgbs``).
    ``sampling="fps"`` ignores ``seed``, samples each aligned cloud with ``pcd_fps_indices`` and adds ``pred_idx`` /
    ``gt_idx``, the picked positions among the masked points; each cloud then carries the colours of its own points.
    ``search="grid"`` does every search with ``nn_grid`` / ``knn_grid``, which return what ``nn_brute`` / ``knn_brute``
    return; ``search="brute"`` keeps the default searches.
    ``fscore_thresholds`` (at most 8) and ``voxel_sizes`` (at most 4), both empty by default, add ``prec@t`` / ``recall@t`` / ``fscore@t`` with
    ``score_counts`` and ``iou@v`` with ``voxel_counts`` (the number in a key is ``format(x, "g")``); without them the
    dict is what it was."""
    pcd_score_names(fscore_thresholds, "fscore_thresholds", PCD_MAX_THRESHOLDS)
    pcd_score_names(voxel_sizes, "voxel_sizes", PCD_MAX_VOXEL_SIZES)
    if sampling not in ("random", "fps"):
        raise ValueError(f"pcd_evaluation: sampling must be 'random' or 'fps', not {sampling!r}")
    if search not in ("brute", "grid"):
        raise ValueError(f"pcd_evaluation: search must be 'brute' or 'grid', not {search!r}")
    how = {"nn": nn_grid, "knn_fn": knn_grid} if search == "grid" else {}
    how.update(fscore_thresholds=fscore_thresholds, voxel_sizes=voxel_sizes)
    m = _np(masks).reshape(-1) > 0
    p = _np(pred_pts).astype(np.float32).reshape(-1, 3)[m]
    g = _np(gt_pts).astype(np.float32).reshape(-1, 3)[m]
    col = np.zeros((len(p), 3), np.float32) if rgbs is None else _np(rgbs).astype(np.float32).reshape(-1, 3)[m]
    scal = (math.nan,) * 4
    if len(p):
        p, g, scal = pcd_align(p, g)
    if sampling == "fps":
        pair = pcd_sample_indices_fps(p, g, downsample_num)
        ip, ig = pair if pair is not None else (np.arange(len(p), dtype=np.int64),) * 2
        p, g, cp, cg = (p, g, col, col.copy()) if pair is None else (p[ip], g[ig], col[ip], col[ig])
        res = pcd_metrics_from_clouds(p, g, threshold, knn, max_iteration, **how)
        res.update(n_points=len(p), pred_scale=float(scal[0]), gt_scale=float(scal[1]), pred_shift_z=float(scal[2]), gt_shift_z=float(scal[3]),
                   pred_pcd=(p, cp), gt_pcd=(g, cg), pred_idx=ip, gt_idx=ig)
        return res
    idx = pcd_sample_indices(len(p), downsample_num, seed)
    if idx is not None:
        p, g, col = p[idx], g[idx], col[idx]
    res = pcd_metrics_from_clouds(p, g, threshold, knn, max_iteration, **how)
    res.update(n_points=len(p), pred_scale=float(scal[0]), gt_scale=float(scal[1]), pred_shift_z=float(scal[2]), gt_shift_z=float(scal[3]),
               pred_pcd=(p, col), gt_pcd=(g, col.copy()))
    return res


def depth_evaluation_in_global_coord(predicted_depth_original, ground_truth_depth_original, ground_truth_radius, cam2world, intrinsics,
                                     max_depth=80, custom_mask=None, post_clip_min=None, post_clip_max=None, pre_clip_min=None,
                                     pre_clip_max=None, align_with_lstsq=False, align_with_lad=False, align_with_lad2=False,
                                     metric_scale=False, lr=1e-4, max_iters=1000, use_gpu=False, align_with_scale=False,
                                     disp_input=False, return_fits=False):
    """``depth_evaluation_in_global_coord`` of the reference (``metrics/eval_depth.py:250-441``) -> ``(res, radius_map)``, float32
    ``[Nf,H,W]``; with ``return_fits=True`` ``(res, radius_map, (s_r, t_r), (s_d, t_d))``.

    mask1 = ``gt_depth > 0`` (and ``< max_depth`` unless that is ``None``) - from the ground-truth DEPTH, never from the radius.
    Fit 1: least squares ``(s_d, t_d)`` of the pre-clipped prediction against the ground-truth depth on mask1.  Every pixel's aligned
    depth ``d = s_d * pred + t_d`` comes from the ORIGINAL prediction (float32, product and sum rounded separately), then the
    post-clip clamps.  In float64 from that float32 ``d``: ``x = (col - cx) * d / fx``, ``y = (row - cy) * d / fy``, ``z = d``
    (integer pixel indices, ``utils/geometry_utils.py:246-253``), ``world = R p + t`` with the frame's ``cam2world[:3]``,
    ``r = |world|`` rounded once to float32.  Fit 2: least squares ``(s_r, t_r)`` of ``r`` against ``ground_truth_radius`` on mask1;
    ``radius_map = s_r * r + t_r`` on every pixel; the eight metrics of ``depth_evaluation`` on ``radius_map`` against the
    ground-truth radius over mask1 and the custom mask, no clamp at that stage.  No valid pixel: zero metrics, both fits
    ``(0, 0)`` and a zero map.  Both fits are solved in float64 and rounded once to float32 - the value the reference's float32
    LAPACK solve approximates, and on the fixture the same float32 bits - because the second fit sees the first one's last bit
    through the geometry, and a float32 solve's last bit is not pinned across LAPACK builds.

    The reference asserts ``align_with_lstsq``: anything else is a ``ValueError`` (``metric_scale`` / ``align_with_scale`` are never
    read once it is set).  ``align_with_lad`` / ``align_with_lad2`` / ``disp_input`` raise ``NotImplementedError`` as in
    ``depth_evaluation``; ``lr`` / ``max_iters`` / ``use_gpu`` have no effect.
    """
    if align_with_lad or align_with_lad2 or disp_input:
        raise NotImplementedError("align_with_lad / align_with_lad2 (no reproducible optimum) and disp_input (undefined in the "
                                  "reference) are not restated")
    if not align_with_lstsq:
        raise ValueError("depth_evaluation_in_global_coord needs align_with_lstsq=True (the reference asserts it)")
    f32 = np.float32
    world, mask, (s_d, t_d) = _world_from_depth(predicted_depth_original, ground_truth_depth_original, cam2world, intrinsics, max_depth,
                                                pre_clip_min, pre_clip_max, post_clip_min, post_clip_max)
    nf, h, w = mask.shape
    gr = _np(ground_truth_radius).astype(f32).reshape(mask.shape)
    r = np.empty(mask.shape, f32)
    for i in range(nf):
        r[i] = np.linalg.norm(world[i].reshape(-1, 3), axis=-1).reshape(h, w)
    s_r, t_r = _lstsq_f32(r[mask], gr[mask], np.float64)
    radius_map = s_r * r + t_r
    sel = mask if custom_mask is None else mask & _np(custom_mask).astype(bool).reshape(mask.shape)
    res = _metric_values(radius_map[sel], gr[sel])
    if return_fits:
        return res, radius_map, (float(s_r), float(t_r)), (float(s_d), float(t_d))
    return res, radius_map


def normal_evaluation(predicted_normal_original, ground_truth_normal_original, custom_mask=None):
    pn = _np(predicted_normal_original).astype(np.float32)
    gn = _np(ground_truth_normal_original).astype(np.float32)
    dot = (pn * gn).sum(-1)
    cosang = dot / (np.linalg.norm(pn, axis=-1) * np.linalg.norm(gn, axis=-1) + np.float32(1e-6))
    err = np.degrees(np.arccos(np.clip(cosang, -1.0, 1.0))).astype(np.float32)
    e = err[_np(custom_mask).astype(bool)] if custom_mask is not None else err.reshape(-1)
    n = e.size
    if n == 0:   # empty mask: NaN metrics (the reference's mean over an empty selection); MetricsManager skips NaN rows
        return {k: float("nan") for k in ("normal mean", "normal median", "normal rmse", "angle < 5", "angle < 7.5",
                                          "angle < 11.25", "angle < 22.5", "angle < 30")}
    out = {"normal mean": float(e.mean(dtype=np.float32)), "normal median": float(np.sort(e)[(n - 1) // 2]),
           "normal rmse": float(np.sqrt((e * e).sum(dtype=np.float32) / n))}
    for k in (5, 7.5, 11.25, 22.5, 30):
        out[f"angle < {k:g}"] = float(100.0 * np.float32((e < k).sum()) / n)
    return out


class MetricsManager:
    def __init__(self, metric_names, sequence_names=None):
        self.metric_names = list(metric_names)
        self.sequence_names = [] if sequence_names is None else list(sequence_names)
        self.rows = {}

    def update_metrics(self, metrics_dict):
        seq = metrics_dict.get("seq_name")
        if seq is None:
            print("error: 'seq_name' missing from the metrics dict")
            return
        if seq not in self.rows:
            if seq not in self.sequence_names:
                self.sequence_names.append(seq)
            self.rows[seq] = {m: math.nan for m in self.metric_names}
        for m in self.metric_names:
            if m in metrics_dict:
                self.rows[seq][m] = float(metrics_dict[m])

    def calculate_averages(self):
        out = {}
        for m in self.metric_names:
            v = [r[m] for r in self.rows.values() if not math.isnan(r[m])]
            out[m] = sum(v) / len(v) if v else math.nan
        return out

    def export_to_csv(self, filepath):
        if not self.rows:
            print("warning: nothing to export")
            return
        d = os.path.dirname(filepath)
        if d:
            os.makedirs(d, exist_ok=True)
        fmt = lambda x: "" if math.isnan(x) else "%.5f" % x
        lines = ["," + ",".join(self.metric_names)]
        for seq in self.sequence_names:
            if seq in self.rows:
                lines.append(seq + "," + ",".join(fmt(self.rows[seq][m]) for m in self.metric_names))
        avg = self.calculate_averages()
        lines.append("Average," + ",".join(fmt(avg[m]) for m in self.metric_names))
        with open(filepath, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(f"metrics export {filepath}")
