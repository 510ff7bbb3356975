"""Evaluation metrics and the CSV sink, restated from the reference:

* ``depth_evaluation``  <- ``/root/reference/metrics/eval_depth.py:6-246`` restricted to the call the harness makes
  (``eval.py:49``: ``align_with_lstsq=True`` + ``custom_mask``): mask 0 < gt < 80, least-squares scale/shift
  (``metrics/alignment.py:150-167``), then AbsRel / SqRel / RMSE / LogRMSE / delta thresholds on the custom mask;
  plus its median / L1-scale / metric alignment modes and the pre- and post-alignment clamps.
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
        A = np.stack([p, np.ones_like(p)], 1)
        sol = np.linalg.lstsq(A, g[:, None], rcond=None)[0]
        s, t = f32(sol[0, 0]), f32(sol[1, 0])
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
    if not return_error_map:
        return res, (s_ret, float(t))
    emap = np.zeros(gt.shape, f32)
    emap[mask] = np.abs((pred[mask] * s + t) - gt[mask]) / gt[mask]
    return res, (s_ret, float(t)), emap.reshape(np.shape(_np(ground_truth_depth_original)))


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
