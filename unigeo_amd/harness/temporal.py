"""Temporal alignment error (TAE) of a video depth prediction: the numpy mirror of ``kernels/temporal.hip``.

UNPINNED: the reference has no such metric.  It is restated from the published definition (ChronoDepth, Video Depth Anything): every frame's
aligned depth is carried into its neighbour's camera with the ground-truth poses and intrinsics and compared there with the neighbour's own
aligned depth as an absolute relative error, averaged over both directions of every consecutive pair.  Two things differ from the published
code: the forward splat keeps the NEAREST depth that reaches a target pixel (an order-independent z-buffer, not the last writer), and a pair
in which no pixel can be scored is left out of the mean and counted as unscored instead of being scored as 0.

The definition, which the kernel implements operation for operation:

* aligned depth ``d`` of every pixel, float32, from the ORIGINAL prediction and the clip's ``(s, t)``: ``a = fl(fl(s * pred) + t)``; in
  disparity space ``a = c`` where ``a < c`` (the optional floor), ``d = 1 / a`` where ``a > 0`` else 0; then ``d`` clamped to the post-clip bounds.
* directed pairs ``P = 2 * (T - stride)``: pair ``2i`` carries frame ``a = i`` into ``b = i + stride``, pair ``2i + 1`` the other way;
  ``M_p = (inv(C_b) @ C_a)[:3]`` in float64 (``relative_poses``; one host function for both paths).
* splat: a source pixel ``(row, col)`` with ``d > 0`` and finite, in float64, one IEEE operation per step:
  ``X = ((col - cx_a) * D) / fx_a``, ``Y = ((row - cy_a) * D) / fy_a``, ``x3 = ((m0 * X + m1 * Y) + m2 * D) + m3`` (likewise ``y3, z3``),
  ``u = rint(((x3 / z3) * fx_b) + cx_b)`` (``v`` likewise), ``z = float32(z3)``; kept when ``z3 > 0``, ``z > 0``, ``z`` finite and
  ``0 <= u < W``, ``0 <= v < H``; the target keeps the smallest ``z``.
* score: a reached target pixel with ``d_b > 0``, ``0 < gt_b < max_depth`` and the custom mask contributes ``e = fl(|z - d_b|) / d_b``
  (float32); the pair's value is ``sum(float64(e)) / count``; ``TAE`` is the mean over the pairs with ``count > 0``, NaN when there is none.
"""
import numpy as np

from .metrics import _np, check_disp_clip_min, disparity_to_depth

TAE_KEYS = ("TAE", "TAE pairs", "TAE pairs total", "TAE pixels")
_UNREACHED = np.uint32(0xFFFFFFFF)      # above the bits of every finite positive float32


def pair_frames(T, stride):
    """``[(a, b)]`` of the ``2 * (T - stride)`` directed pairs, in pair order; empty when ``T <= stride``."""
    stride = int(stride)
    if stride < 1:
        raise ValueError(f"stride must be a positive integer, not {stride!r}")
    out = []
    for i in range(max(int(T) - stride, 0)):
        out += [(i, i + stride), (i + stride, i)]
    return out


def relative_poses(cam2world, stride=1):
    """``[P, 3, 4]`` float64: ``(inv(C_b) @ C_a)[:3]`` of every directed pair, from the float32 camera-to-world matrices widened exactly.
    A pose that cannot be inverted gives a NaN table for its pairs, which then reach no pixel."""
    C = _np(cam2world).astype(np.float32).reshape(-1, 4, 4).astype(np.float64)
    pairs = pair_frames(C.shape[0], stride)
    rel = np.empty((len(pairs), 3, 4), np.float64)
    with np.errstate(all="ignore"):
        for p, (a, b) in enumerate(pairs):
            try:
                rel[p] = (np.linalg.inv(C[b]) @ C[a])[:3]
            except np.linalg.LinAlgError:
                rel[p] = np.nan
    return rel


def aligned_depth(pred, fit, space="depth", disp_clip_min=None, post_clip_min=None, post_clip_max=None):
    """The aligned float32 depth of every pixel from the ORIGINAL prediction and ``fit = (s, t)``, as ``ug_eval_depth_global`` makes it
    (depth space) and as ``depth_evaluation(align_space="disparity")`` makes it (disparity space); the pre-clips enter through ``(s, t)`` only."""
    check_disp_clip_min(space, disp_clip_min, "aligned_depth")
    f32 = np.float32
    p = _np(pred).astype(f32)
    s, t = f32(fit[0]), f32(fit[1])
    with np.errstate(all="ignore"):
        d = p * s + t
        if space == "disparity":
            d = disparity_to_depth(d, disp_clip_min)
        if post_clip_min is not None:
            d = np.where(d < f32(post_clip_min), f32(post_clip_min), d)      # a NaN stays NaN and is dropped later
        if post_clip_max is not None:
            d = np.where(d > f32(post_clip_max), f32(post_clip_max), d)
    return d.astype(f32)


def warp_depth(depth, intrinsics, rel, stride=1):
    """Forward-splat every frame of ``depth`` ``[T,H,W]`` into its pair's target camera -> ``[P,H,W]`` float32, 0 where unreached."""
    f64 = np.float64
    d = _np(depth).astype(np.float32)
    T, H, W = d.shape
    K = _np(intrinsics).astype(np.float32).reshape(T, 3, 3).astype(f64)
    pairs = pair_frames(T, stride)
    rel = np.asarray(rel, f64).reshape(len(pairs), 3, 4)
    row, col = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing="ij")
    out = np.zeros((len(pairs), H, W), np.float32)
    with np.errstate(all="ignore"):
        for p, (a, b) in enumerate(pairs):
            D = d[a].astype(f64)
            X = ((col - K[a, 0, 2]) * D) / K[a, 0, 0]
            Y = ((row - K[a, 1, 2]) * D) / K[a, 1, 1]
            m = rel[p]
            x3 = ((m[0, 0] * X + m[0, 1] * Y) + m[0, 2] * D) + m[0, 3]
            y3 = ((m[1, 0] * X + m[1, 1] * Y) + m[1, 2] * D) + m[1, 3]
            z3 = ((m[2, 0] * X + m[2, 1] * Y) + m[2, 2] * D) + m[2, 3]
            u = np.rint(((x3 / z3) * K[b, 0, 0]) + K[b, 0, 2])
            v = np.rint(((y3 / z3) * K[b, 1, 1]) + K[b, 1, 2])
            z = z3.astype(np.float32)
            keep = (d[a] > 0) & np.isfinite(d[a]) & (z3 > 0) & (z > 0) & np.isfinite(z) & (u >= 0) & (v >= 0) & (v < H) & (u < W)
            idx = v[keep].astype(np.int64) * W + u[keep].astype(np.int64)
            zbuf = np.full(H * W, _UNREACHED, np.uint32)
            np.minimum.at(zbuf, idx, z[keep].view(np.uint32))      # positive floats order as their bits do
            zbuf[zbuf == _UNREACHED] = 0
            out[p] = zbuf.view(np.float32).reshape(H, W)
    return out


def temporal_alignment_error(pred, gt_depth, cam2world, intrinsics, fit, custom_mask=None, max_depth=80, stride=1, space="depth",
                             disp_clip_min=None, post_clip_min=None, post_clip_max=None, return_maps=False):
    """TAE of ``pred`` ``[T,H,W]`` (a depth, or a disparity with ``space="disparity"``) under the clip's ``fit = (s, t)`` ->
    ``{"TAE", "TAE pairs", "TAE pairs total", "TAE pixels"}``; ``return_maps=True`` adds ``pair_values`` ``[P,2]`` float64 (value, count; the
    value of a pair without a scored pixel is NaN), ``warp`` and ``err`` ``[P,H,W]`` float32 (0 where unreached / unscored).
    ``max_depth=None`` keeps every ``gt > 0``.  ``TAE`` is a fraction, like ``Abs Rel``; NaN when no pair is scored (``T <= stride`` included)."""
    f32 = np.float32
    d = aligned_depth(pred, fit, space, disp_clip_min, post_clip_min, post_clip_max)
    if d.ndim != 3:
        raise ValueError("temporal_alignment_error: pred must be [T,H,W]")
    T, H, W = d.shape
    gt = _np(gt_depth).astype(f32).reshape(T, H, W)
    cm = None if custom_mask is None else _np(custom_mask).astype(bool).reshape(T, H, W)
    pairs = pair_frames(T, stride)
    rel = relative_poses(cam2world, stride)
    warp = warp_depth(d, intrinsics, rel, stride)
    vals = np.full((len(pairs), 2), np.nan, np.float64)
    err = np.zeros_like(warp) if return_maps else None
    with np.errstate(all="ignore"):
        for p, (_, b) in enumerate(pairs):
            ok = (warp[p] > 0) & (d[b] > 0) & (gt[b] > 0)
            if max_depth is not None:
                ok &= gt[b] < f32(max_depth)
            if cm is not None:
                ok &= cm[b]
            e = np.abs(warp[p][ok] - d[b][ok]) / d[b][ok]
            vals[p, 1] = e.size
            if e.size:
                vals[p, 0] = e.astype(np.float64).sum() / e.size
            if return_maps:
                err[p][ok] = e
    scored = vals[:, 1] > 0
    res = {"TAE": float(vals[scored, 0].mean()) if scored.any() else float("nan"), "TAE pairs": int(scored.sum()),
           "TAE pairs total": len(pairs), "TAE pixels": int(vals[:, 1].sum())}
    if return_maps:
        res.update({"pair_values": vals, "warp": warp, "err": err})
    return res
