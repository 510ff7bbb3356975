#!/usr/bin/env python
"""Visualisation panels of one 25 x 384 x 512 clip: host composition against device composition, in ONE process with
interleaved rounds (tools/time_cfg.py's scheme).  The clip's depth and normals are made resident by one run of the tiny-width model (the
panels do not care what the numbers are); the colour bar strip is rendered once, before the timing, and handed to both legs.  Each round times
  (1) host  : download depth + normals (ug_dc_get_outputs), range and panels by the numpy mirror (harness/vis.py)
  (2) device: ug_vis_depth_range + ug_vis_panels on the resident tensors and frames, uint8 panels downloaded
with a host clock around calls that end in a device synchronise, and checks that both legs give the same bytes.  Encoding the 25 images
(the same work after either leg) is timed once and reported separately.
usage: time_vis.py [rounds]"""
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unigeo_amd import weights as W
from unigeo_amd.harness import vis
from unigeo_amd.model.depthcrafter import DepthCrafter
from unigeo_amd.pipeline import DepthCrafterPipelineHIP, make_noise
from unigeo_amd.synthetic import synthetic_clip

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
T, H, W_ = 25, 384, 512
u, v, c = W.tiny_cfgs()
pipe = DepthCrafterPipelineHIP.from_state(W.random_state(W.unet_manifest(u), 1), W.random_state(W.vae_manifest(v), 2), W.random_state(W.clip_manifest(c), 3),
                                          cfgs=(u, v, c), workspace_bytes=16 << 30)
eng = pipe.engine
clip = synthetic_clip(T, H, W_)
frames, K = DepthCrafter.prepare_input(None, clip), np.stack(clip["intrinsics"], 0)
nl, na = make_noise(T, H, W_, 0)
eng.set_inputs(frames, nl, na, K)
eng.run(1, 8, with_normals=True)
LUT = vis.SPECTRAL_R_LUT


def host_leg(cbar):
    _, depth, normals = eng.get_outputs(frames=False, depth=True, normals=True)
    vmin, vmax = vis.depth_range(depth)
    return vis.panels_u8(depth, normals, vmin, vmax, LUT, rgbs=frames, cbar=cbar)


def device_leg(cbar):
    vmin, vmax = eng.vis_depth_range()
    return eng.vis_panels(vmin, vmax, LUT, rgbs="resident", cbar=cbar)


vmin, vmax = eng.vis_depth_range()
cbar = vis.colorbar_strip(H, vmin, vmax)
if cbar is None:                                   # no matplotlib on this machine: a strip of the same size, so that both legs move the same bytes
    cbar = np.random.default_rng(0).uniform(size=(H, H // 4, 3)).astype(np.float32)
a, b = host_leg(cbar), device_leg(cbar)            # warm-up of both legs
assert a.shape == b.shape == (T, H, 3 * W_ + 5 + cbar.shape[1], 3), (a.shape, b.shape)
assert np.array_equal(a, b), f"{int((a != b).sum())} bytes differ"
print(f"clip {T} x {H} x {W_}, depth {float(vmin):.4f} .. {float(vmax):.4f}, panels {b.shape} = {b.nbytes / 1e6:.1f} MB; "
      f"host leg downloads {(T * H * W_ * 4 * 4) / 1e6:.1f} MB, device leg {b.nbytes / 1e6:.1f} MB", flush=True)
res = {"host": [], "device": []}
for rnd in range(rounds):
    for name, leg in (("host", host_leg), ("device", device_leg)):
        t0 = time.perf_counter(); out = leg(cbar); dt = time.perf_counter() - t0
        assert np.array_equal(out, b), name
        res[name].append(dt)
        print(f"round {rnd} {name:6s}: {dt * 1e3:8.2f} ms/clip", flush=True)
h, d = (float(np.median(res[k])) for k in ("host", "device"))
print(f"summary (median of {rounds} rounds): host {h * 1e3:.2f} ms/clip (min {min(res['host']) * 1e3:.2f}, max {max(res['host']) * 1e3:.2f}), "
      f"device {d * 1e3:.2f} ms/clip (min {min(res['device']) * 1e3:.2f}, max {max(res['device']) * 1e3:.2f}), host / device {h / d:.2f} x", flush=True)
write, ext = vis._writer()
with tempfile.TemporaryDirectory() as tmp:
    t0 = time.perf_counter()
    for i, im in enumerate(b):
        write(os.path.join(tmp, f"frame_{i:04d}"), im)
    dt = time.perf_counter() - t0
print(f"encoding {T} {ext} images (either leg, not part of the figures above): {dt * 1e3:.1f} ms/clip", flush=True)
eng.close()
