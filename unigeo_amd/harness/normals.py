"""Ground-truth normals fitted from the depth, for the loaders that have none (``harness/rgbd.py`` with ``normals="depth"``).

The reference gives the five RGB-D datasets no normals (its loaders comment them out) and, where its authors want to look at some, fits a
plane to the back-projected depth: ``get_surface_normal_np`` (``utils/geometry_utils.py:73-134``, used by ``test_vis_dataset.py`` on
7-Scenes).  ``fit_normals`` is that fit - the mean outer product of the window's points plus ``1e-6 I``, solved against their mean,
``n / (|n| + 1e-6)``, flipped to face the camera - made usable as ground truth on sensor depth: the window leaves out masked pixels (the
reference sums a hole as a point at the origin) and pixels across a depth discontinuity, and a pixel whose window keeps too few points is
marked invalid, which the reference cannot express.

It is the host mirror of ``ug_prep_gt_normals``: ``include/unigeo_hip.h`` documents the arithmetic operation by operation, and both evaluate
it in float64 on the float32 points, one IEEE operation at a time, every sum left to right - the kernel gives the same bits.

Pinned by ``tests/golden/gt_normals_golden.npz``: with ``edge=None`` and a full mask the interior pixels are the reference's system (weights
1/25, ``eps_identity = 1e-6``) and agree with ``get_surface_normal_np`` within its own float32 noise.  UNPINNED: the masked variant - the
reference has no such mode.  ``edge = 0.05`` (a neighbour takes part while its depth is within 5 % of the centre's) and the majority
``min_count`` are design choices, not measurements; ``radius = 2`` is the reference's ``patch_size = 5``.
"""
import numpy as np

NORMALS_MODES = (None, "depth")
RADIUS_RANGE = (1, 8)
DEFAULT_RADIUS = 2
DEFAULT_EDGE = 0.05


def default_min_count(radius):
    """The majority of the full window: ``(2r+1)^2 // 2 + 1``."""
    return (2 * radius + 1) ** 2 // 2 + 1


def check_fit_options(radius=DEFAULT_RADIUS, edge=DEFAULT_EDGE, min_count=None, who="fit_normals"):
    """-> ``(radius, edge or None, min_count)`` as the fit uses them; ``ValueError`` on a radius outside 1..8, an edge that is negative or
    NaN, or a min_count below 1."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not RADIUS_RANGE[0] <= radius <= RADIUS_RANGE[1]:
        raise ValueError(f"{who}: radius must be an integer in {RADIUS_RANGE[0]}..{RADIUS_RANGE[1]}, not {radius!r}")
    radius = int(radius)
    if edge is not None:
        edge = float(edge)
        if not edge >= 0:
            raise ValueError(f"{who}: edge must be a non-negative number or None (the edge test off), not {edge!r}")
    if min_count is None:
        min_count = default_min_count(radius)
    elif isinstance(min_count, bool) or not isinstance(min_count, (int, np.integer)) or min_count < 1:
        raise ValueError(f"{who}: min_count must be a positive integer or None (the majority of the window), not {min_count!r}")
    return radius, edge, int(min_count)


def fit_normals_counts(cam_coord, mask, radius=DEFAULT_RADIUS, edge=DEFAULT_EDGE, min_count=None):
    """``fit_normals`` with the window count of every pixel: -> ``(cam_normal, normal_mask, count)``, ``count`` int32 ``[H,W]`` = the number of
    neighbours that took part (0 where the centre is masked)."""
    radius, edge, min_count = check_fit_options(radius, edge, min_count)
    p = np.asarray(cam_coord)
    m = np.asarray(mask)
    if p.ndim != 3 or p.shape[0] != 3 or p.dtype != np.float32:
        raise ValueError("fit_normals: cam_coord must be float32 [3,H,W]")
    if m.shape != p.shape[1:]:
        raise ValueError("fit_normals: mask must be [H,W], the size of cam_coord")
    H, W = m.shape
    r = radius
    ok = m.astype(bool)
    # the frame padded by r: an absent neighbour is a masked one
    pad = np.zeros((3, H + 2 * r, W + 2 * r), np.float64)
    pad[:, r:r + H, r:r + W] = np.where(ok[None], p.astype(np.float64), 0.0)      # a masked pixel may hold anything (NaN): it never enters a sum
    okp = np.zeros((H + 2 * r, W + 2 * r), bool)
    okp[r:r + H, r:r + W] = ok
    cx, cy, cz = pad[:, r:r + H, r:r + W]
    dc = -cz
    lim = None if edge is None else edge * dc
    S = [np.zeros((H, W), np.float64) for _ in range(9)]      # Sxx Sxy Sxz Syy Syz Szz sx sy sz, each from +0
    cnt = np.zeros((H, W), np.int32)
    for dy in range(-r, r + 1):                               # row-major over the window: the order of the sums
        for dx in range(-r, r + 1):
            sl = (slice(r + dy, r + dy + H), slice(r + dx, r + dx + W))
            x, y, z = pad[0][sl], pad[1][sl], pad[2][sl]
            part = ok & okp[sl]
            if lim is not None:
                part &= np.abs(-z - dc) <= lim
            for acc, v in zip(S, (x * x, x * y, x * z, y * y, y * z, z * z, x, y, z)):
                acc += np.where(part, v, 0.0)                 # + (+0) leaves a sum that started at +0 unchanged, bit for bit
            cnt += part
    enough = ok & (cnt >= min_count)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c = np.where(enough, cnt, 1).astype(np.float64)
        axx, axy, axz, ayy, ayz, azz = S[0] / c + 1e-6, S[1] / c, S[2] / c, S[3] / c + 1e-6, S[4] / c, S[5] / c + 1e-6
        bx, by, bz = S[6] / c, S[7] / c, S[8] / c
        c00, c01, c02 = ayy * azz - ayz * ayz, axz * ayz - axy * azz, axy * ayz - axz * ayy
        c11, c12, c22 = axx * azz - axz * axz, axy * axz - axx * ayz, axx * ayy - axy * axy
        det = (axx * c00 + axy * c01) + axz * c02
        n0 = ((c00 * bx + c01 * by) + c02 * bz) / det
        n1 = ((c01 * bx + c11 * by) + c12 * bz) / det
        n2 = ((c02 * bx + c12 * by) + c22 * bz) / det
        den = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2) + 1e-6
        n0, n1, n2 = n0 / den, n1 / den, n2 / den
        flip = (n0 * cx + n1 * cy) + n2 * cz > 0
        n = np.stack([np.where(flip, -v, v) for v in (n0, n1, n2)])
        valid = enough & np.isfinite(n).all(axis=0)
        out = np.where(valid[None], n, 0.0).astype(np.float32)
    return out, valid.astype(np.float32), np.where(ok, cnt, 0).astype(np.int32)


def fit_normals(cam_coord, mask, radius=DEFAULT_RADIUS, edge=DEFAULT_EDGE, min_count=None):
    """Normals of one native-size frame from its points: ``cam_coord`` float32 ``[3,H,W]`` in the loader's OpenGL camera frame, ``mask``
    ``[H,W]`` (non-zero = valid) -> ``(cam_normal float32 [3,H,W], normal_mask float32 [H,W])``.  Per valid pixel the points of its
    ``(2 radius + 1)^2`` window that are valid and, with ``edge``, whose depth lies within ``edge * depth`` of the centre's are fitted with a
    plane (the reference's ``get_surface_normal_np`` system on that subset); the unit normal faces the camera.  A pixel is valid iff its
    centre is, at least ``min_count`` neighbours took part (default: the majority of the window) and the normal is finite; invalid pixels
    give 0 in both arrays.  ``edge=None`` switches the edge test off.  ``edge=0.05`` and the majority count are design choices, not
    measurements; the masked variant is UNPINNED (the module docstring).  Vectorised: one shifted-array accumulation per window offset.
    ``ValueError``: ``radius`` outside 1..8, a negative ``edge``, ``min_count`` below 1, arrays of another shape or dtype."""
    n, valid, _ = fit_normals_counts(cam_coord, mask, radius, edge, min_count)
    return n, valid


def world_normals(cam_normal, M):
    """``fl32(M33 n)`` per pixel: ``cam_normal`` float32 ``[3,H,W]``, ``M`` the source-camera-to-key-view matrix the loader applies to
    ``cam_coord``.  The three-term sums run in float64, left to right, and are rounded once - the arithmetic of ``ug_prep_gt_normals``."""
    g = np.asarray(cam_normal, np.float32).astype(np.float64)
    m = np.asarray(M, np.float32).astype(np.float64)
    return np.stack([(m[j, 0] * g[0] + m[j, 1] * g[1]) + m[j, 2] * g[2] for j in range(3)]).astype(np.float32)
