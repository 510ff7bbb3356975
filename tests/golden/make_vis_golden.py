#!/usr/bin/env python
"""Golden vectors for the visualisation panels, made like make_depth_global_golden.py: the REFERENCE's own
``utils/vis_utils.py`` (``save_depth_normal_maps``, lines 38-84, with ``colorize`` / ``colorize_np`` / ``get_vertical_colorbar``) is imported by
path from /root/reference (read-only) and run on seeded inputs.  Writes tests/golden/vis_golden.npz - data only; the other fixtures keep
their bytes.

Modules the reference imports and this machine lacks are stubbed: ``roma``, ``tqdm``, ``open3d`` (unused by the functions called), ``cv2``
(``cv2.resize`` = the numpy area average of unigeo_amd.harness.vis - cv2.INTER_AREA itself is NOT what ran, so the stored strip is "the
reference's colour bar code + our area average"), ``imageio.v2`` (``imwrite`` keeps the array it is given and writes a real image, so the
reference's following ``Image.open`` works).  ``matplotlib.cm.get_cmap`` no longer exists in matplotlib >= 3.9: shimmed to
``matplotlib.colormaps[name]``.

Input at 3 x 20 x 28: depth in 0.9 .. 10 holding the clip's min and max pixels and, for several table rows k, the smallest float32 depth
whose ``u * 256`` is exactly k together with its predecessor (row k - 1) - the edge where a differently rounded division shows; unit
normals with the six axis directions (components -1, 0, 1) among them; rgbs = uint8 / 255 as the reference's prepare_gt_label makes them,
every byte value 0..255 present.  Run once with rgbs and once without.  Stored: the inputs, the uint8 panels the reference handed to
``imwrite``, the colour bar strip it produced (float32, fed back by the tests), vmin, vmax and the colour table.
"""
import importlib.util
import os
import sys
import tempfile
import types

import matplotlib
import matplotlib.cm
import numpy as np
import torch
from PIL import Image

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from unigeo_amd.harness import vis  # noqa: E402

f32 = np.float32
captured, strips = [], []


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__path__ = []
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _resize(im, size, interpolation=None):
    w, h = size
    out = vis.area_resize(im, h, w)
    strips.append(out)
    return out


def _imwrite(path, arr):
    captured.append(np.array(arr, copy=True))
    Image.fromarray(arr).save(path)


for name in ("roma", "tqdm", "open3d"):
    if name not in sys.modules:
        _stub(name)
_stub("cv2", resize=_resize, INTER_AREA=3)
iio = _stub("imageio")
iio.v2 = _stub("imageio.v2", imwrite=_imwrite)
if not hasattr(matplotlib.cm, "get_cmap"):
    matplotlib.cm.get_cmap = lambda name: matplotlib.colormaps[name]

spec = importlib.util.spec_from_file_location("ref_vis_utils", os.path.join(REF, "utils", "vis_utils.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

rng = np.random.default_rng(20261018)
T, H, W = 3, 20, 28
VMIN, VMAX = f32(0.9), f32(10.0)


def table_row(x):
    u = f32(f32(x) - VMIN) / f32(VMAX - VMIN)
    return u * f32(256)


depth = rng.uniform(1.0, 9.9, (T, H, W)).astype(f32)
depth[0, 0, 0], depth[2, H - 1, W - 1] = VMIN, VMAX
edges = []
for k in (1, 2, 3, 64, 100, 128, 129, 200, 254, 255):
    x = f32(float(VMIN) + k / 256.0 * (float(VMAX) - float(VMIN)))
    while table_row(x) >= k:
        x = np.nextafter(x, f32(0))
    lo = x                                        # the largest depth of row k - 1
    x = np.nextafter(lo, f32(100))                # the smallest depth of row k
    if table_row(x) == k:                         # u * 256 lands on the integer exactly
        edges.append((k, lo, x))
assert len(edges) >= 5, edges
for j, (k, lo, x) in enumerate(edges):
    depth[1, 2 + j // 10, 2 + 2 * (j % 10)], depth[1, 2 + j // 10, 3 + 2 * (j % 10)] = lo, x
print(f"{len(edges)} table rows k with a float32 depth whose u * 256 == k exactly:", [k for k, _, _ in edges])

normals = rng.standard_normal((T, H, W, 3))
normals = (normals / np.linalg.norm(normals, axis=-1, keepdims=True)).astype(f32)
for j, ax in enumerate([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]):
    normals[0, 1, j] = ax

u8 = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
u8.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
rgbs = torch.from_numpy(u8) / 255.0               # as the reference's prepare_gt_label: a float32 tensor
assert rgbs.dtype == torch.float32 and len(np.unique(u8)) == 256

G = {"depth": depth, "normals": normals, "rgbs": rgbs.numpy().copy(), "rgbs_u8": u8}
with tempfile.TemporaryDirectory() as tmp:
    for tag, kw in (("rgb", {"rgbs": [r for r in rgbs]}), ("norgb", {})):
        captured.clear(); strips.clear()
        ref.save_depth_normal_maps(torch.from_numpy(depth.copy()), torch.from_numpy(normals.copy()), tmp, **kw)
        assert len(captured) == T and len(strips) == T and all(np.array_equal(s, strips[0]) for s in strips)
        G["panels_" + tag] = np.stack(captured, 0)
        G["cbar_" + tag] = strips[0].astype(f32)
assert np.array_equal(G["cbar_rgb"], G["cbar_norgb"])
G["cbar"] = G.pop("cbar_rgb"); del G["cbar_norgb"]
G["vmin"], G["vmax"] = f32(depth.min()), f32(depth.max())
assert G["vmin"] == VMIN and G["vmax"] == VMAX
G["lut"] = matplotlib.colormaps["Spectral_r"](np.arange(256))[:, :3].astype(f32)

Wc = G["cbar"].shape[1]
assert G["panels_rgb"].shape == (T, H, 3 * W + 5 + Wc, 3) and G["panels_norgb"].shape == (T, H, 2 * W + 5 + Wc, 3)
back = G["panels_rgb"][:, :, :W]
print(f"rgb bytes that come back as k - 1 (fl32(k / 255) * 255 truncated): {int((back.astype(int) == u8.astype(int) - 1).sum())} of {u8.size}; "
      f"as k: {int((back == u8).sum())}; distinct k affected: {len(np.unique(u8[back != u8]))}")
assert ((back == u8) | (back.astype(int) == u8.astype(int) - 1)).all()
mine = vis.panels_u8(depth, normals, G["vmin"], G["vmax"], G["lut"], rgbs=G["rgbs"], cbar=G["cbar"])
print("host mirror equals the reference's panels:", np.array_equal(mine, G["panels_rgb"]), "- differing bytes:", int((mine != G["panels_rgb"]).sum()))
np.savez_compressed(os.path.join(OUT, "vis_golden.npz"), **G)
print("wrote", os.path.join(OUT, "vis_golden.npz"), {k: (v.shape, str(v.dtype)) for k, v in G.items()})
