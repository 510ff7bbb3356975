"""Depth / normal visualisation panels - mirrors the reference's ``utils/vis_utils.py:38-135,139-231`` (``save_depth_normal_maps``,
``get_vertical_colorbar``, ``colorize_np`` / ``colorize``) as ``eval.py:58-62`` calls them under ``vis_depth: True``.

One image per frame: ``rgb | normals * 0.5 + 0.5 | depth through Spectral_r over the clip's min..max | 5 black columns | colour bar``.
The composition exists twice with the same float32 arithmetic: on the device (``Engine.vis_depth_range`` /
``Engine.vis_panels``, kernels/vis.hip) and here in numpy (``depth_range`` / ``colorize`` / ``panels_u8``).  Every step is one float32
operation; bytes are ``trunc(x * 255)`` saturated to 0..255 with NaN -> 0.  Only the colour bar strip needs matplotlib (it is text
rendering); the colour table itself ships as data, so the panels need nothing but numpy.
"""
import os
import threading
import warnings

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SPECTRAL_R_LUT = np.loadtxt(os.path.join(_HERE, "spectral_r_lut.txt"), dtype=np.float64).astype(np.float32)      # [256,3]; written by tools/make_spectral_lut.py
SPECTRAL_R_LUT.setflags(write=False)

_f32 = np.float32
_cbar_lock = threading.Lock()
_warned = set()


def _warn_once(key, msg):
    if key not in _warned:
        _warned.add(key)
        warnings.warn(msg, stacklevel=3)


def _np(x, dtype=np.float32):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=dtype)


def _u8(v):
    """trunc to a byte: saturates to 0..255, NaN -> 0 (``ndarray.astype(np.uint8)`` is undefined outside that range)"""
    with np.errstate(invalid="ignore"):
        v = np.where(v > 0, v, _f32(0))
        return np.minimum(v, _f32(255)).astype(np.uint8)


def unit_to_u8(x):
    """float32 in [0,1] -> byte, ``trunc(fl32(x * 255))``"""
    return _u8(np.asarray(x, _f32) * _f32(255))


def depth_range(depth):
    """(vmin, vmax) of the clip as float32, NaN ignored; ``(0, 0)`` when nothing is left (``ug_vis_depth_range``)."""
    d = _np(depth).reshape(-1)
    d = d[~np.isnan(d)]
    if d.size == 0:
        return _f32(0), _f32(0)
    return d.min(), d.max()


def colorize(depth, vmin, vmax, lut=SPECTRAL_R_LUT):
    """``[...]`` float32 depth -> ``[...,3]`` uint8 through the 256-entry table: x = clamp(d, vmin, vmax), u = (x - vmin) / (vmax - vmin),
    i = min(int(u * 256), 255), each step rounded to float32.  NaN depth or ``vmax == vmin`` (0 / 0) gives black, matplotlib's "bad" colour."""
    d, vmin, vmax = _np(depth), _f32(vmin), _f32(vmax)
    lut8 = unit_to_u8(_np(lut).reshape(256, 3))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x = np.minimum(np.maximum(d, vmin), vmax)
        u = (x - vmin) / _f32(vmax - vmin)
        v = u * _f32(256)
        bad = np.isnan(u)
        i = np.where(v > 0, np.minimum(v, _f32(255)), _f32(0)).astype(np.int64)      # v in [255, 256] is entry 255; NaN -> 0, blacked out below
    out = lut8[i]
    out[bad] = 0
    return out


def panel_width(W, rgbs, cbar):
    return (W if rgbs else 0) + 2 * W + (5 + cbar.shape[1] if cbar is not None else 0)


def panels_u8(depth, normals, vmin, vmax, lut=SPECTRAL_R_LUT, rgbs=None, cbar=None):
    """Host mirror of ``ug_vis_panels``: depth ``[T,H,W]``, normals ``[T,H,W,3]``, optional rgbs ``[T,H,W,3]`` in [0,1] and colour bar strip
    ``[H,Wc,3]`` -> uint8 ``[T,H,Wp,3]``."""
    d, n = _np(depth), _np(normals)
    T, H, W = d.shape
    if n.shape != (T, H, W, 3):
        raise ValueError("panels_u8: depth must be [T,H,W] and normals [T,H,W,3]")
    parts = []
    if rgbs is not None:
        r = _np(rgbs)
        if r.shape != (T, H, W, 3):
            raise ValueError("panels_u8: rgbs must be [T,H,W,3]")
        parts.append(unit_to_u8(r))
    parts.append(unit_to_u8(n * _f32(0.5) + _f32(0.5)))
    parts.append(colorize(d, vmin, vmax, lut))
    if cbar is not None:
        c = _np(cbar)
        if c.ndim != 3 or c.shape[0] != H or c.shape[2] != 3 or c.shape[1] == 0:
            raise ValueError("panels_u8: cbar must be [H,Wc,3] with Wc > 0")
        parts.append(np.zeros((T, H, 5, 3), np.uint8))
        parts.append(np.broadcast_to(unit_to_u8(c), (T, *c.shape)))
    return np.ascontiguousarray(np.concatenate(parts, axis=2))


def _area_weights(n_in, n_out):
    """[n_out, n_in] weights of an area average: the share of output cell o (n_in / n_out input cells wide) that input cell i covers"""
    edges = np.arange(n_out + 1, dtype=np.float64) * (n_in / n_out)
    lo, hi = edges[:-1, None], edges[1:, None]
    cell = np.arange(n_in, dtype=np.float64)[None, :]
    w = np.clip(np.minimum(hi, cell + 1) - np.maximum(lo, cell), 0.0, None)
    return w / w.sum(axis=1, keepdims=True)


def area_resize(im, h, w):
    """``[H,W,C]`` float image -> ``[h,w,C]`` float32, every output pixel the area-weighted mean of the input pixels it covers (what
    ``cv2.resize(..., interpolation=cv2.INTER_AREA)`` computes when shrinking; float64 sums, one rounding)."""
    im = np.asarray(im, np.float64)
    out = np.einsum("oh,hwc->owc", _area_weights(im.shape[0], h), im)
    out = np.einsum("pw,owc->opc", _area_weights(im.shape[1], w), out)
    return out.astype(np.float32)


def colorbar_strip(h, vmin, vmax, cmap_name="Spectral_r", cbar_precision=2):
    """The reference's vertical colour bar: a 2 x 8 inch, 100 dpi matplotlib figure holding one colour bar with six ticks from ``vmin`` to
    ``vmax`` (labels rounded to ``cbar_precision`` digits, size 18), rendered with Agg to 800 x 200 and reduced to ``[h, int(200 / 800 * h), 3]``
    float32 in [0,1] by an area average.  ``None`` (with one warning) when matplotlib cannot be imported: the panel then ends after the depth."""
    try:
        import matplotlib as mpl
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.colorbar import Colorbar
        from matplotlib.figure import Figure
    except ImportError:
        _warn_once("matplotlib", "matplotlib is not importable: the visualisation panels are written without the colour bar")
        return None
    vmin, vmax = float(vmin), float(vmax)
    with _cbar_lock, warnings.catch_warnings():
        warnings.simplefilter("ignore")              # a constant clip (vmin == vmax) makes matplotlib warn about singular limits
        fig = Figure(figsize=(2, 8), dpi=100)
        canvas = FigureCanvasAgg(fig)
        ax = fig.add_subplot(111)
        ticks = np.linspace(vmin, vmax, 6)
        cb = Colorbar(ax, cmap=mpl.colormaps[cmap_name], norm=mpl.colors.Normalize(vmin=vmin, vmax=vmax), ticks=ticks, orientation="vertical")
        labels = [str(np.round(t, cbar_precision)) for t in ticks]
        if cbar_precision == 0:
            labels = [s[:-2] for s in labels]
        cb.set_ticklabels(labels)
        cb.ax.tick_params(labelsize=18, rotation=0)
        canvas.draw()
        buf, (width, height) = canvas.print_to_buffer()
    im = np.frombuffer(buf, np.uint8).reshape(height, width, 4)[:, :, :3].astype(np.float32) / _f32(255)
    if h != im.shape[0]:
        w = int(im.shape[1] / im.shape[0] * h)
        if w < 1:
            return None                              # narrower than a pixel at this height: no strip
        im = np.clip(area_resize(im, h, w), 0.0, 1.0)
    return im


def _writer():
    """(write(path_without_extension, uint8 image) -> path, extension): imageio when importable, else Pillow; WebP like the reference when
    the encoder is there, else PNG"""
    try:
        import imageio.v2 as iio
        ext = ".webp"
        try:
            from PIL import features
            if not features.check("webp"):
                ext = ".png"
        except ImportError:
            pass
        return (lambda stem, im: (iio.imwrite(stem + ext, im), stem + ext)[1]), ext
    except ImportError:
        from PIL import Image, features
        ext = ".webp" if features.check("webp") else ".png"
        if ext == ".png":
            _warn_once("webp", "this Pillow build cannot encode WebP: the visualisation panels are written as PNG")
        return (lambda stem, im: (Image.fromarray(im).save(stem + ext), stem + ext)[1]), ext


def save_depth_normal_maps(depth_maps, normal_maps, path, rgbs=None, engine=None):
    """The reference's ``save_depth_normal_maps`` plus ``engine``: writes ``path/frame_%04d.webp`` (one panel per frame) and returns the
    panels, uint8 ``[T,H,Wp,3]``.  With an ``Engine`` the range and the panels come from the device (``depth_maps`` / ``normal_maps`` =
    ``None``: the tensors resident after the last run; ``rgbs="resident"``: the resident input frames) and only bytes come back;
    without one the numpy mirror composes them."""
    d = None if depth_maps is None else _np(depth_maps)
    n = None if normal_maps is None else _np(normal_maps)
    r = rgbs if rgbs is None or isinstance(rgbs, str) else _np(np.stack([_np(x) for x in rgbs], 0) if isinstance(rgbs, (list, tuple)) else rgbs)
    if engine is not None:
        vmin, vmax = engine.vis_depth_range(d)
        H = d.shape[1] if d is not None else (n.shape[1] if n is not None else engine._shape[1])
        panels = engine.vis_panels(vmin, vmax, SPECTRAL_R_LUT, depth=d, normals=n, rgbs=r, cbar=colorbar_strip(H, vmin, vmax))
    else:
        if d is None or n is None or isinstance(r, str):
            raise ValueError("save_depth_normal_maps: resident tensors need an engine")
        vmin, vmax = depth_range(d)
        panels = panels_u8(d, n, vmin, vmax, SPECTRAL_R_LUT, rgbs=r, cbar=colorbar_strip(d.shape[1], vmin, vmax))
    write, _ = _writer()
    for i, im in enumerate(panels):
        write(os.path.join(path, f"frame_{i:04d}"), im)
    return panels


def write_ply(path, points, colors=None):
    """A point cloud as binary little-endian PLY: float32 x y z and uint8 red green blue per vertex (``vis_pcd``).
    ``colors`` float in [0, 1] (``u8 = trunc(c * 255)`` after clipping) or ``None`` for white."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    col = np.full((len(pts), 3), 255, np.uint8) if colors is None else (np.clip(np.asarray(colors, np.float32).reshape(-1, 3), 0.0, 1.0) * np.float32(255)).astype(np.uint8)
    rec = np.empty(len(pts), np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
    rec["xyz"], rec["rgb"] = pts, col
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(pts))
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(rec.tobytes())


def read_ply(path):
    """What ``write_ply`` wrote -> ``(points float32 [n,3], colours uint8 [n,3])``."""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").split("\n")
    if head[0] != "ply" or head[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: not a binary little-endian PLY")
    n = int(next(l for l in head if l.startswith("element vertex")).split()[2])
    rec = np.frombuffer(raw, np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]), count=n, offset=end)
    return rec["xyz"].copy(), rec["rgb"].copy()
