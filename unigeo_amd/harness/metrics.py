"""Evaluation metrics and the CSV sink, restated from the reference:

* ``depth_evaluation``  <- ``/root/reference/metrics/eval_depth.py:6-246`` restricted to the call the harness makes
  (``eval.py:49``: ``align_with_lstsq=True`` + ``custom_mask``): mask 0 < gt < 80, least-squares scale/shift
  (``metrics/alignment.py:150-167``), then AbsRel / SqRel / RMSE / LogRMSE / delta thresholds on the custom mask;
  plus its median / L1-scale / metric alignment modes and the pre- and post-alignment clamps.
* ``depth_evaluation_in_global_coord`` <- ``/root/reference/metrics/eval_depth.py:250-441``: the aligned depth back-projected,
  moved into the world frame, and evaluated as the distance from the world origin.
* ``normal_evaluation`` <- ``/root/reference/metrics/eval_normal.py:4-72``: angular error in degrees, mean / median /
  rmse / % under 5, 7.5, 11.25, 22.5, 30 degrees.
* ``MetricsManager``    <- ``/root/reference/metrics/save_utils.py:5-90``: one row per sequence, NaN for missing
  metrics, trailing ``Average`` row (NaN-skipping mean), ``%.5f``.
The lad / lad2 / disp_input modes of the reference function raise here (see ``depth_evaluation``).
"""
import math
import os

import numpy as np


def _np(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


DEPTH_ALIGNMENTS = ("lstsq", "median", "scale", "metric")


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


def depth_evaluation(predicted_depth_original, ground_truth_depth_original, max_depth=80, custom_mask=None,
                     post_clip_min=None, post_clip_max=None, pre_clip_min=None, pre_clip_max=None,
                     align_with_lstsq=False, align_with_lad=False, align_with_lad2=False, metric_scale=False,
                     align_with_scale=False, disp_input=False, lr=1e-4, max_iters=1000, use_gpu=False, return_error_map=False,
                     **unsupported):
    """``depth_evaluation`` of the reference (``metrics/eval_depth.py:59-204``) -> ``(res, (s, t))``, with
    ``return_error_map=True`` ``(res, (s, t), error_map)``.

    On mask1 = ``gt > 0`` (and ``gt < max_depth`` unless that is ``None``): clamp the prediction to the pre-clip bounds,
    align, clamp to the post-clip bounds, apply the custom mask, compute the metrics.  The alignment keeps the
    reference's precedence: ``metric_scale`` (s = 1), then ``align_with_lstsq`` (scale and shift), then
    ``align_with_scale`` (Weiszfeld L1 scale, here in float64 and plain index order; clamped to >= 1e-3), then the
    default: ``s = median(gt) / median(pred)`` with ``torch.median``'s LOWER median, element ``(n - 1) // 2`` of the
    sorted values.  The error map is ``|s * pred + t - gt| / gt`` on mask1 and 0 elsewhere, from the ORIGINAL prediction
    (neither clamp applied), as the reference computes it.  No valid pixel: zero metrics and ``(s, t) = (1, 0)`` under
    ``metric_scale``, ``(0, 0)`` otherwise.

    Still rejected with ``NotImplementedError``: ``align_with_lad`` / ``align_with_lad2`` run a scipy BFGS and a
    1000-step Adam on a non-smooth objective, which gives no reproducible answer; ``disp_input`` calls ``depth2disparity``,
    which the reference defines nowhere, so its own call raises ``NameError``.  ``lr`` / ``max_iters`` (lad2 only) and
    ``use_gpu`` (tensor placement) are accepted and have no effect.
    """
    if align_with_lad or align_with_lad2 or disp_input or any(v for v in unsupported.values()):
        raise NotImplementedError("align_with_lad / align_with_lad2 (no reproducible optimum) and disp_input (undefined in the "
                                  "reference) are not restated")
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
    if metric_scale:
        s, t = f32(1), f32(0)
    elif align_with_lstsq:
        s, t = _lstsq_f32(p, g)
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
    emap[mask] = np.abs((pred[mask] * s + t) - gt[mask]) / gt[mask]
    return res, (s_ret, float(t)), emap.reshape(np.shape(_np(ground_truth_depth_original)))


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
    f32, f64 = np.float32, np.float64
    pred = _np(predicted_depth_original).astype(f32)
    if pred.ndim == 2:
        pred = pred[None]
    nf, h, w = pred.shape
    gt = _np(ground_truth_depth_original).astype(f32).reshape(pred.shape)
    gr = _np(ground_truth_radius).astype(f32).reshape(pred.shape)
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
    r = np.empty(pred.shape, f32)
    for i in range(nf):
        z = d[i].astype(f64)
        x = (col - f64(K[i, 0, 2])) * z / f64(K[i, 0, 0])
        y = (row - f64(K[i, 1, 2])) * z / f64(K[i, 1, 1])
        cam = np.stack((x, y, z), axis=-1).reshape(-1, 3)
        world = cam @ poses[i][:3, :3].T + poses[i][:3, 3][:, None].T
        r[i] = np.linalg.norm(world, axis=-1).reshape(h, w)
    s_r, t_r = _lstsq_f32(r[mask], gr[mask], np.float64)
    radius_map = s_r * r + t_r
    sel = mask if custom_mask is None else mask & _np(custom_mask).astype(bool).reshape(pred.shape)
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
