"""ScanNet++ mesh renderer on the host: depth, normals and the triangle index of a triangle mesh seen from pinhole
cameras - the numpy mirror of ``ug_prep_render_mesh`` (kernels/render.hip) and the oracle for it.

Restates what the reference makes offline through pyrender, OpenGL and two GLSL shaders
(``dataset/scannetpp/preprocess_scannetpp_imu.py:470-497``, ``shaders/mesh.vert``, ``mesh.frag``) as 2-D homogeneous rasterisation in
float64.  The arithmetic is documented operation by operation in ``include/unigeo_hip.h``; every line below is those operations in that
order (numpy evaluates one IEEE operation per operator and never fuses two), so host and device agree byte for byte.  UNPINNED against
pyrender: no GL stack is installed where this project is built (DESIGN.md section 29 states how far the two can differ).

Plain numpy, one triangle at a time over its conservative screen box; the per-triangle set-up is evaluated for all triangles of a frame at once.
"""
import math

import numpy as np

ZNEAR, ZFAR = 0.05, 20.0           # preprocess_scannetpp_imu.py:340-341
ZFAR_MAX = 65.535                  # depth_mm is 16 bits of millimetres


def _cross(a, b):
    """(a x b) per component as ``a*b - c*d``: swapping the operands negates the result exactly."""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _corner(v, m):
    """p = R v + T, rows summed as ((a + b) + c) + T; v [n,3] float64, m the 3x4 world-to-camera matrix."""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([((m[j, 0] * x + m[j, 1] * y) + m[j, 2] * z) + m[j, 3] for j in range(3)], axis=-1)


def _box(p, k, H, W):
    """The screen box [r0, r1) x [c0, c1) of one triangle with camera-space corners ``p`` [3,3]: with all three corners in front of the camera
    the pixel centres between the smallest and the largest projected coordinate and one more pixel each way, the whole frame otherwise."""
    r0, r1, c0, c1 = 0, H, 0, W
    if p[:, 2].min() > 0.0:
        fx, fy, cx, cy = k
        u = (p[:, 0] / p[:, 2]) * fx + cx
        v = (p[:, 1] / p[:, 2]) * fy + cy
        ulo, uhi, vlo, vhi = u.min(), u.max(), v.min(), v.max()
        if ulo > -1e9 and uhi < 1e9 and vlo > -1e9 and vhi < 1e9:
            c0 = int(max(0.0, math.floor(ulo - 0.5) - 1.0)); c1 = int(min(float(W), math.floor(uhi - 0.5) + 2.0))
            r0 = int(max(0.0, math.floor(vlo - 0.5) - 1.0)); r1 = int(min(float(H), math.floor(vhi - 0.5) + 2.0))
    return r0, r1, c0, c1


def _key(z32):
    """float32 -> uint32 whose unsigned order is the float order (``reg_key`` of kernels/zkey.h)."""
    u = z32.view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def _render_frame(v64, faces, keep, m, k, H, W, znear, zfar):
    """One frame: (the z-buffer of 64-bit words, D per triangle); ``keep``: the triangles that are not skipped."""
    fx, fy, cx, cy = k
    p0, p1, p2 = (_corner(v64[faces[:, i]], m) for i in range(3))
    c = np.stack([_cross(p1, p2), _cross(p2, p0), _cross(p0, p1)], axis=1)              # [NF,3,3]
    D = (p0[:, 0] * c[:, 0, 0] + p0[:, 1] * c[:, 0, 1]) + p0[:, 2] * c[:, 0, 2]
    pz = np.stack([p0[:, 2], p1[:, 2], p2[:, 2]], axis=1)
    with np.errstate(invalid="ignore"):
        todo = keep & (pz.max(1) >= znear * 0.999999) & (pz.min(1) <= zfar * 1.000001)
    best = np.full((H, W), np.uint64(0xffffffffffffffff), np.uint64)                     # (key of fl32(z) << 32) | index, as the device keeps it
    rx_all = ((np.arange(W, dtype=np.float64) + 0.5) - cx) / fx
    ry_all = ((np.arange(H, dtype=np.float64) + 0.5) - cy) / fy
    for t in np.nonzero(todo)[0]:
        r0, r1, c0, c1 = _box(np.stack([p0[t], p1[t], p2[t]]), k, H, W)
        if r1 <= r0 or c1 <= c0:
            continue
        rx, ry = rx_all[None, c0:c1], ry_all[r0:r1, None]
        ct = c[t]
        with np.errstate(all="ignore"):
            e0 = (rx * ct[0, 0] + ry * ct[0, 1]) + ct[0, 2]
            e1 = (rx * ct[1, 0] + ry * ct[1, 1]) + ct[1, 2]
            e2 = (rx * ct[2, 0] + ry * ct[2, 1]) + ct[2, 2]
            den = (e0 + e1) + e2
            z = D[t] / den
            hit = (den != 0.0) & (((e0 >= 0.0) & (e1 >= 0.0) & (e2 >= 0.0)) | ((e0 <= 0.0) & (e1 <= 0.0) & (e2 <= 0.0))) & (z >= znear) & (z <= zfar)
        if not hit.any():
            continue
        z32 = np.where(hit, z, 1.0).astype(np.float32)
        key = (_key(z32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
        sub = best[r0:r1, c0:c1]
        np.minimum(sub, np.where(hit, key, np.uint64(0xffffffffffffffff)), out=sub)
    return best, D


def _decode_key(best):
    empty = best == np.uint64(0xffffffffffffffff)
    tri = np.where(empty, -1, (best & np.uint64(0xffffffff)).astype(np.int64)).astype(np.int32)
    kz = (best >> np.uint64(32)).astype(np.uint32)
    u = np.where(kz & np.uint32(0x80000000), kz & np.uint32(0x7fffffff), ~kz)
    z32 = np.where(empty, np.float32(0), u.view(np.float32))
    return z32, tri, empty


def _encode_normals(n_world, l2, D, tri, empty, m):
    """The script's two-step encoding of the winner's face normal: world normal facing the camera -> unorm8 -> decoded -> rotated into the
    OpenGL camera -> unorm8 by truncation; 0 where no triangle covers the pixel."""
    t = np.where(empty, 0, tri)
    with np.errstate(all="ignore"):
        u = n_world[t] / np.sqrt(l2[t])[..., None]
        u = np.where((D[t] > 0.0)[..., None], -u, u)
        q = np.floor(255.0 * (0.5 * u + 0.5) + 0.5)
        d = (q / 255.0) * 2.0 - 1.0
        w = [(m[j, 0] * d[..., 0] + m[j, 1] * d[..., 1]) + m[j, 2] * d[..., 2] for j in range(3)]
        g = np.stack([w[0], -w[1], -w[2]], axis=-1)
        e = np.trunc(((g + 1.0) / 2.0) * 255.0)
    e = np.where(e >= 255.0, 255.0, np.where(e >= 0.0, e, 0.0))                          # a NaN gives 0
    out = e.astype(np.uint8)
    out[empty] = 0
    return out


def check_render_args(verts, faces, world2cam, K, H, W, znear, zfar, who="render_mesh"):
    """The argument checks of ``ug_prep_render_mesh`` (the same conditions, as ``ValueError``) -> (verts f32 [NV,3], faces i32 [NF,3],
    world2cam f64 [T,3,4], K f64 [T,4])."""
    v = np.ascontiguousarray(verts, dtype=np.float32)
    f = np.asarray(faces)
    if v.ndim != 2 or v.shape[1] != 3 or len(v) == 0:
        raise ValueError(f"{who}: verts must be [NV,3] with NV > 0")
    if f.ndim != 2 or f.shape[1] != 3 or len(f) == 0 or f.dtype.kind not in "iu":
        raise ValueError(f"{who}: faces must be integers [NF,3] with NF > 0")
    if f.min() < 0 or f.max() >= len(v):
        raise ValueError(f"{who}: a face index lies outside 0..NV-1")
    f = np.ascontiguousarray(f, dtype=np.int32)
    m = np.ascontiguousarray(world2cam, dtype=np.float64).reshape(-1, 3, 4)
    k = np.ascontiguousarray(K, dtype=np.float64).reshape(-1, 4)
    if len(m) != len(k) or len(m) == 0:
        raise ValueError(f"{who}: one world-to-camera matrix and one (fx, fy, cx, cy) per frame")
    if H <= 0 or W <= 0 or len(m) * H * W >= 1 << 31:
        raise ValueError(f"{who}: H and W must be positive and T * H * W below 2^31")
    if not (np.isfinite(v).all() and np.isfinite(m).all() and np.isfinite(k).all()):
        raise ValueError(f"{who}: a vertex, pose or intrinsic is not finite")
    if not (k[:, :2] > 0).all():
        raise ValueError(f"{who}: fx and fy must be positive")
    if not (math.isfinite(znear) and znear > 0 and math.isfinite(zfar) and zfar > znear and zfar <= ZFAR_MAX):
        raise ValueError(f"{who}: 0 < znear < zfar <= {ZFAR_MAX} (depth_mm holds 16 bits of millimetres)")
    return v, f, m, k


def world2cam_from(cam_to_world):
    """Camera-to-world [T,4,4] (or [4,4]) -> world-to-camera [T,3,4] by ``numpy.linalg.inv``: the one inverse of the whole path."""
    c = np.asarray(cam_to_world, np.float64)
    c = c[None] if c.ndim == 2 else c
    if c.ndim != 3 or c.shape[1:] != (4, 4):
        raise ValueError("cam_to_world must be [T,4,4] or [4,4]")
    return np.ascontiguousarray(np.linalg.inv(c)[:, :3, :])


def intrinsics4(K, T):
    """``K`` as [T,4] = fx, fy, cx, cy from (fx, fy, cx, cy), a 3x3 matrix, or one of either per frame."""
    k = np.asarray(K, np.float64)
    if k.shape[-2:] == (3, 3):
        k = np.stack([k[..., 0, 0], k[..., 1, 1], k[..., 0, 2], k[..., 1, 2]], axis=-1)
    if k.shape[-1] != 4:
        raise ValueError("K must be (fx, fy, cx, cy) or a 3x3 matrix, one for all frames or one per frame")
    return np.ascontiguousarray(np.broadcast_to(k.reshape(-1, 4), (T, 4)) if k.size == 4 else k.reshape(T, 4))


def check_masks(masks, T, H, W, who="render_mesh"):
    if masks is None:
        return None
    mk = np.asarray(masks)
    mk = mk[None] if mk.ndim == 2 else mk
    if mk.dtype != np.uint8 or mk.shape != (T, H, W):
        raise ValueError(f"{who}: masks must be uint8 [T,H,W]")
    return np.ascontiguousarray(mk)


def rescaled_size_and_intrinsics(size_wh, K, output_resolution):
    """The output size and intrinsics of the script's ``rescale_image_depthmap`` / ``camera_matrix_of_crop`` (``:97-146``, ``force=True``, no
    crop): ``size_wh`` = (W, H) of the input, ``K`` its 3x3 intrinsics in the OpenCV convention (pixel centres at integers),
    ``output_resolution`` = (W, H) to be covered -> ``((W_out, H_out), K_out 3x3 OpenCV, scale)``.  The smallest scale (plus 1e-8) at which
    both output sides reach the request; the principal point is scaled in the colmap convention (pixel centres at halves) and moved by
    half of what the floor cut off.  Pinned by tests/golden/render_golden.npz."""
    in_res = np.array(size_wh)
    out_req = np.array(output_resolution)
    scale = max(out_req / in_res) + 1e-8
    out_res = np.floor(in_res * scale).astype(int)
    margins = in_res * scale - out_res
    k = np.array(K, dtype=np.float64, copy=True)
    k[0, 2] += 0.5; k[1, 2] += 0.5
    k[:2, :] *= scale
    k[:2, 2] -= 0.5 * margins
    k[0, 2] -= 0.5; k[1, 2] -= 0.5
    return (int(out_res[0]), int(out_res[1])), k, float(scale)


def nearest_resize(a, out_wh):
    """``cv2.resize(a, out_wh, interpolation=cv2.INTER_NEAREST)`` restated: ``src = min(floor(dst * in / out), in - 1)`` per axis.  UNPINNED
    (OpenCV is not installed where this project is built)."""
    h, w = a.shape[:2]
    wo, ho = out_wh
    cols = np.minimum(np.floor(np.arange(wo) * (1.0 / (wo / w))).astype(np.int64), w - 1)
    rows = np.minimum(np.floor(np.arange(ho) * (1.0 / (ho / h))).astype(np.int64), h - 1)
    return a[rows][:, cols]


def render_mesh(verts, faces, cam_to_world, K, H, W, masks=None, znear=ZNEAR, zfar=ZFAR):
    """``verts`` float32 [NV,3], ``faces`` int [NF,3], ``cam_to_world`` [T,4,4] (OpenCV axes), ``K`` = (fx, fy, cx, cy) or 3x3, one or one per
    frame, in the convention in which pixel (col, row) looks along (col + 0.5, row + 0.5); ``masks`` uint8 [T,H,W] or None ->
    ``(depth_mm uint16 [T,H,W], normal uint8 [T,H,W,3], tri_index int32 [T,H,W])``.  depth_mm is 0 where nothing is hit or ``mask < 255``;
    the normal is 0 where nothing is hit; tri_index is -1 there."""
    m_all = world2cam_from(cam_to_world)
    T = len(m_all)
    v, f, m_all, k_all = check_render_args(verts, faces, m_all, intrinsics4(K, T), H, W, znear, zfar)
    mk = check_masks(masks, T, H, W)
    v64 = v.astype(np.float64)
    a, b = v64[f[:, 1]] - v64[f[:, 0]], v64[f[:, 2]] - v64[f[:, 0]]
    with np.errstate(over="ignore", invalid="ignore"):
        n_world = _cross(a, b)
        l2 = (n_world[:, 0] * n_world[:, 0] + n_world[:, 1] * n_world[:, 1]) + n_world[:, 2] * n_world[:, 2]
        keep = (l2 > 0.0) & (l2 < np.inf)
    depth = np.zeros((T, H, W), np.uint16); normal = np.zeros((T, H, W, 3), np.uint8); index = np.empty((T, H, W), np.int32)
    for t in range(T):
        best, D = _render_frame(v64, f, keep, m_all[t], k_all[t], H, W, float(znear), float(zfar))
        z32, tri, empty = _decode_key(best)
        mm = (z32 * np.float32(1000.0)).astype(np.int32).astype(np.uint16)             # trunc(fl32(fl32(z) * 1000f)); below 65536
        if mk is not None:
            mm[mk[t] < 255] = 0
        depth[t], index[t] = mm, tri
        normal[t] = _encode_normals(n_world, l2, D, tri, empty, m_all[t])
    return depth, normal, index
