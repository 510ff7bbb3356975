"""Focal, camera poses and depth from world point maps - what the reference's point-map plugins (Spann3R, CUT3R) take from
``solve_depth_and_camera_from_3d_points`` (``metrics/utils.py:68-160``, called from ``model/spann3r.py:43``).  This numpy mirror states the
arithmetic once, in float64; ``kernels/pointmap.hip`` follows it operation by operation (``ug_pointmap_focal`` / ``ug_pointmap_poses``).

* ``pointmap_focal`` restates ``estimate_focal_knowing_depth(pts[0:1], pp, 'weiszfeld')`` (``metrics/utils.py:93-115``).  The reference runs in
  float32; ``tests/golden/camera_golden.npz`` holds its values and how far this float64 restatement lies from them.
* ``pointmap_poses`` is UNPINNED and a different algorithm: the reference calls ``cv2.solvePnPRansac``, which draws random samples (and is not
  installed).  Here every frame is solved by the orthogonal (object-space) iteration of Lu, Hager and Mjolsness (PAMI 2000), deterministic,
  followed by a trim at ``reproj_px`` (cv2's default reprojection threshold, 8 pixels) and a refit until the inlier set stops changing.

Sums run over all pixels of a frame in the order of the device kernels (``_ordered_sum``): 256 pixels per block, a binary tree inside the block,
the blocks in index order.  A pixel outside the current set contributes zero.
"""
import numpy as np

PB, MAXB = 256, 1024          # threads per block and the block cap of kernels/pointmap.hip
MAX_ITER = 300                # orthogonal iterations per fit
MAX_ROUNDS = 5                # trims after the first fit
REL_TOL = 1e-12               # relative change of the object-space error that ends a fit
FLOOR_SCALE = 1e-6 * 2.0 ** -48   # absolute floor of that error and of its change: a millionth of sum (2^-24 |X|)^2, the float32 rounding of the input
MIN_POINTS = 4


def _blocks(n):
    return min(max((n + PB - 1) // PB, 1), MAXB)


def _ordered_sum(v, reverse=False):
    """Sum of ``v [n]`` or ``[n,k]`` over axis 0 in the order of the device: block ``b`` of ``nb = min(ceil(n / 256), 1024)``, thread ``t`` adds
    the pixels ``b * 256 + t + j * nb * 256`` for ascending ``j``; the 256 threads are folded by halves (``t += t + o`` for ``o = 128 .. 1``); the
    block results are added in block order.  ``reverse`` feeds the pixels backwards: the same numbers in another order (what the tests call
    d_order)."""
    v = np.asarray(v, np.float64)
    flat = v.ndim == 1
    if flat:
        v = v[:, None]
    if reverse:
        v = v[::-1]
    n, k = v.shape
    nb = _blocks(n)
    stride = nb * PB
    J = -(-n // stride)
    buf = np.zeros((J * stride, k))
    buf[:n] = v
    buf = buf.reshape(J, nb, PB, k)
    a = buf[0].copy()
    for j in range(1, J):
        a += buf[j]
    o = PB // 2
    while o:
        a[:, :o] += a[:, o:2 * o]
        o //= 2
    out = np.cumsum(a[:, 0], axis=0)[-1]          # cumsum adds strictly in order
    return float(out[0]) if flat else out


def _pixel_grid(H, W):
    row, col = np.divmod(np.arange(H * W), W)
    return col.astype(np.float64), row.astype(np.float64)


def _f32_points(pts, ndim):
    if hasattr(pts, "detach"):
        pts = pts.detach().cpu().numpy()
    pts = np.asarray(pts)
    if pts.ndim != ndim or pts.shape[-1] != 3:
        raise ValueError(f"point map must be {'[T,H,W,3]' if ndim == 4 else '[H,W,3]'}, not {list(pts.shape)}")
    return np.ascontiguousarray(pts, dtype=np.float32)


def pointmap_focal(pts0, pp=None, _reverse=False):
    """Focal length in pixels from the point map ``[H,W,3]`` of the frame whose camera is the world frame.  ``pp`` defaults to ``(W/2, H/2)``.
    Pixel grid ``0 .. W-1``, ``0 .. H-1`` minus ``pp``; ``xy / z`` with NaN and +-inf set to 0; the closed-form start
    ``mean(xy.px) / mean(xy.xy)``; ten reweighting steps with ``w = 1 / max(|px - f xy|, 1e-8)``; means over all pixels; clipped below at 0 as
    the reference's ``clip(min_focal = 0)``."""
    pts0 = _f32_points(pts0, 3)
    H, W = pts0.shape[:2]
    cx, cy = (W / 2.0, H / 2.0) if pp is None else (float(pp[0]), float(pp[1]))
    col, row = _pixel_grid(H, W)
    u, v = col - cx, row - cy
    X = pts0.reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        a, b = X[:, 0] / X[:, 2], X[:, 1] / X[:, 2]
    a = np.where(np.isfinite(a), a, 0.0)
    b = np.where(np.isfinite(b), b, 0.0)
    dpx = a * u + b * v
    dxx = a * a + b * b
    n = float(H * W)
    s = _ordered_sum(np.stack([dpx, dxx], 1), _reverse)
    f = (s[0] / n) / (s[1] / n)
    for _ in range(10):
        du, dv = u - f * a, v - f * b
        dis = np.sqrt(du * du + dv * dv)
        w = 1.0 / np.maximum(dis, 1e-8)
        s = _ordered_sum(np.stack([w * dpx, w * dxx], 1), _reverse)
        f = (s[0] / n) / (s[1] / n)
    return float(f) if f > 0.0 else 0.0


def _inv3(m):
    """Inverse of a 3x3 by the adjugate (the host code of the device path does the same)."""
    c00 = m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]
    c01 = m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]
    c02 = m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]
    det = (m[0, 0] * c00 + m[0, 1] * c01) + m[0, 2] * c02
    adj = np.array([[c00, m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2], m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]],
                    [c01, m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0], m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]],
                    [c02, m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1], m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]]])
    return adj / det


def _rot(R, X):
    """``(r0 x + r1 y) + r2 z`` per coordinate."""
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    return np.stack([(R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z for r in range(3)], 1)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _rotation_from_sums(s):
    """The Kabsch rotation of the centred ``X`` onto the centred ``q`` from ``s = n, sum X (3), sum q (3), sum q X^T (9, row = q)``, with the
    determinant fix of ``umeyama_rigid`` (harness/metrics.py)."""
    n = s[0]
    mx, mq = s[1:4] / n, s[4:7] / n
    Hm = s[7:16].reshape(3, 3) / n - np.outer(mq, mx)
    U, _, Vt = np.linalg.svd(Hm)
    S = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0])
    return U @ S @ Vt


class _Frame:
    """One frame's pixels: points ``X`` (float64 copies of the float32 input, NaN allowed), unit rays ``b``, the pixel coordinates."""

    def __init__(self, pts, f, cx, cy, reverse):
        H, W = pts.shape[:2]
        self.col, self.row = _pixel_grid(H, W)
        self.f, self.cx, self.cy, self.reverse = f, cx, cy, reverse
        self.X = pts.reshape(-1, 3).astype(np.float64)
        dx, dy = (self.col - cx) / f, (self.row - cy) / f
        nrm = np.sqrt((dx * dx + dy * dy) + 1.0)
        self.b = np.stack([dx / nrm, dy / nrm, 1.0 / nrm], 1)

    def sum(self, keep, cols):
        with np.errstate(all="ignore"):
            v = np.stack(cols, 1)
        return _ordered_sum(np.where(keep[:, None], v, 0.0), self.reverse)

    def fit(self, keep, R, max_iter):
        """Orthogonal iteration over the pixels of ``keep`` from the rotation ``R`` -> ``(R, t, iterations, object-space error)``."""
        X, b = self.X, self.b
        with np.errstate(all="ignore"):
            s0 = self.sum(keep, [np.ones(len(X)), b[:, 0] * b[:, 0], b[:, 0] * b[:, 1], b[:, 0] * b[:, 2], b[:, 1] * b[:, 1], b[:, 1] * b[:, 2],
                                 b[:, 2] * b[:, 2], _dot(X, X)])
        n = s0[0]
        SV = np.array([[s0[1], s0[2], s0[3]], [s0[2], s0[4], s0[5]], [s0[3], s0[5], s0[6]]])
        Minv = _inv3(np.eye(3) - SV / n)
        floor = FLOOR_SCALE * s0[7]
        prev = None
        for it in range(1, max_iter + 1):
            with np.errstate(all="ignore"):
                p = _rot(R, X)
                bp = _dot(b, p)
                g = b * bp[:, None] - p
                sg = self.sum(keep, [g[:, 0], g[:, 1], g[:, 2]])
                t = np.array([((Minv[r, 0] * sg[0] + Minv[r, 1] * sg[1]) + Minv[r, 2] * sg[2]) / n for r in range(3)])
                c = p + t
                q = b * _dot(b, c)[:, None]
                d = c - q
                e = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                s = self.sum(keep, [np.ones(len(X)), X[:, 0], X[:, 1], X[:, 2], q[:, 0], q[:, 1], q[:, 2]] +
                             [q[:, r] * X[:, k] for r in range(3) for k in range(3)] + [e])
            err = s[16]
            if err <= floor or (prev is not None and abs(prev - err) <= max(REL_TOL * prev, floor)) or it == max_iter:
                break
            R = _rotation_from_sums(s)
            prev = err
        return R, t, it, err

    def camera_points(self, R, t):
        with np.errstate(all="ignore"):
            return _rot(R, self.X) + t

    def inliers(self, valid, keep, R, t, reproj_px):
        """The valid pixels in front of the camera whose reprojection under ``(R, t)`` lies within ``reproj_px`` of their own pixel ->
        ``(set, count, how many memberships changed against keep, sum of squared reprojection errors over the set)``."""
        with np.errstate(all="ignore"):
            c = self.camera_points(R, t)
            du = (self.f * (c[:, 0] / c[:, 2]) + self.cx) - self.col
            dv = (self.f * (c[:, 1] / c[:, 2]) + self.cy) - self.row
            e2 = du * du + dv * dv
            new = valid & (c[:, 2] > 0.0) & (e2 <= reproj_px * reproj_px)
        s = _ordered_sum(np.stack([new.astype(np.float64), (new != keep).astype(np.float64), np.where(new, e2, 0.0)], 1), self.reverse)
        return new, int(s[0]), int(s[1]), float(s[2])


def pointmap_poses(pts, focal=None, pp=None, mask=None, reproj_px=8.0, max_iter=MAX_ITER, max_rounds=MAX_ROUNDS, _reverse=False):
    """World point maps ``[T,H,W,3]`` (float32; frame 0 in its own camera frame when the focal is to be recovered) -> dict with
    ``extrinsics [T,4,4]`` float64 world to camera, ``depth [T,H,W]`` float32 (``z`` of ``R X + t`` rounded once, 0 at invalid pixels),
    ``focal``, and per frame ``n_inliers``, ``iterations``, ``reproj_rms`` (pixels) and the inlier set ``inliers [T,H,W]`` bool.
    ``pred_poses = inv(extrinsics)``.

    A pixel is valid when its three coordinates are finite and ``mask`` (``[T,H,W]``, > 0 keeps) keeps it; fewer than 4 valid pixels in a frame
    is a ``ValueError``.  Unit rays ``b = normalize(K^-1 (col, row, 1))`` with ``K`` from ``focal`` (``None``: ``pointmap_focal`` of frame 0) and
    ``pp`` (default ``(W/2, H/2)``).  With ``V = b b^T`` one iteration is ``t = (1/n) (I - mean V)^-1 sum (V - I) R X``, ``q = V (R X + t)``, next
    ``R`` = Kabsch of the centred ``X`` onto the centred ``q``.  Frame 0 starts from the identity, every other frame from the frame before.  A fit
    ends when the object-space error ``E = sum |(I - V)(R X + t)|^2`` changes by less than a relative ``1e-12``, or when ``E`` or its change is at
    most the floor ``1e-6 sum (2^-24 |X|)^2`` - a millionth of the float32 rounding of the input - or after ``max_iter`` iterations.  The floor is
    what ends a fit of data that are exact up to their float32 rounding: there ``E`` settles at about 0.07 of the rounding sum and is itself only
    known to a relative 1e-10 (``c - V c`` cancels), so a relative 1e-12 never holds; stopping as soon as ``E`` is below the whole rounding sum
    instead leaves the pose up to 2.6e-5 degrees from the optimum (measured).  Then pixels with a
    reprojection error above ``reproj_px`` or ``z <= 0`` are dropped and the fit continues from the current pose, until no membership changes or
    ``max_rounds`` trims were made; a trim that would leave fewer than 4 pixels is not made."""
    pts = _f32_points(pts, 4)
    T, H, W = pts.shape[:3]
    if min(T, H, W) <= 0:
        raise ValueError("pointmap_poses: T, H and W must be positive")
    if not reproj_px > 0:
        raise ValueError("pointmap_poses: reproj_px must be positive")
    cx, cy = (W / 2.0, H / 2.0) if pp is None else (float(pp[0]), float(pp[1]))
    f = pointmap_focal(pts[0], (cx, cy), _reverse) if focal is None else float(focal)
    if not (f > 0 and np.isfinite(f)):
        raise ValueError(f"pointmap_poses: the focal must be positive and finite, not {f}")
    if mask is not None:
        mask = np.asarray(mask).reshape(T, H * W) > 0
    out = {"extrinsics": np.tile(np.eye(4), (T, 1, 1)), "depth": np.zeros((T, H, W), np.float32), "focal": f,
           "n_inliers": np.zeros(T, np.int64), "iterations": np.zeros(T, np.int64), "reproj_rms": np.zeros(T),
           "inliers": np.zeros((T, H, W), bool)}
    R = np.eye(3)
    for k in range(T):
        fr = _Frame(pts[k], f, cx, cy, _reverse)
        valid = np.isfinite(fr.X).all(1)
        if mask is not None:
            valid &= mask[k]
        if int(valid.sum()) < MIN_POINTS:
            raise ValueError(f"pointmap_poses: frame {k} has {int(valid.sum())} valid pixels; a pose needs at least {MIN_POINTS}")
        keep, iters = valid, 0
        for rnd in range(max_rounds + 1):
            R, t, it, _ = fr.fit(keep, R, max_iter)
            iters += it
            new, cnt, changed, se = fr.inliers(valid, keep, R, t, float(reproj_px))
            if changed == 0 or rnd == max_rounds or cnt < MIN_POINTS:
                break
            keep = new
        out["extrinsics"][k, :3, :3], out["extrinsics"][k, :3, 3] = R, t
        z = fr.camera_points(R, t)[:, 2]
        out["depth"][k] = np.where(valid, z, 0.0).astype(np.float32).reshape(H, W)
        out["n_inliers"][k], out["iterations"][k] = cnt, iters
        out["reproj_rms"][k] = np.sqrt(se / cnt) if cnt else np.nan
        out["inliers"][k] = new.reshape(H, W)
    return out


def poses_from_pointmap(pts, focal=None, mask=None, reproj_px=8.0, engine=None):
    """``pred_poses [T,4,4]`` (camera to world, ``inv(extrinsics)`` as ``model/spann3r.py:46`` forms them) of a model's world points, through
    ``engine.pointmap_poses`` when an engine is given and through the mirror otherwise."""
    if engine is not None:
        pts = _f32_points(pts, 4)
        f = engine.pointmap_focal(pts[0]) if focal is None else float(focal)
        res = engine.pointmap_poses(pts, f, mask=mask, reproj_px=reproj_px)
    else:
        res = pointmap_poses(pts, focal=focal, mask=mask, reproj_px=reproj_px)
    return np.linalg.inv(res["extrinsics"]), res
