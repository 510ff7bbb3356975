#!/usr/bin/env python
"""Classifier-free guidance on the full-size clip (25 x 384 x 512, 25 steps, 40 GB arena), in ONE process with interleaved rounds (box-to-box
spread is +-4 %, so the variants are only compared inside one process; tools/ab_clip.py's scheme).  Each round times
  (a) guidance_scale = 1          - the unguided path
  (b) guidance_scale = 1.2        - one batched UNet pass over the conditional and the unconditional video per step
  (c) guidance_scale = 1.2        - two unbatched UNet passes per step (UG_CFG_SEQUENTIAL=1, a measurement-only switch of the engine)
and prints ms per clip, frames/s and each variant's own ug_workspace_peak (one clip in a FRESH context with the plugin's default 24 GiB arena: the
arena's high-water mark is per context, so the timing context's would mix the variants); every output is checked finite.
usage: time_cfg.py [rounds]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unigeo_amd import weights as W
from unigeo_amd.model.depthcrafter import DepthCrafter
from unigeo_amd.pipeline import DepthCrafterPipelineHIP, make_noise
from unigeo_amd.synthetic import synthetic_clip

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
T, H, W_, STEPS, G = 25, 384, 512, 25, 1.2
u, v, c = W.UNetCfg(), W.VAECfg(), W.CLIPCfg()
states = (W.random_state(W.unet_manifest(u), 42), W.random_state(W.vae_manifest(v), 43), W.random_state(W.clip_manifest(c), 44))   # = from_random(seed=42)
clip = synthetic_clip(T, H, W_)
frames, K = DepthCrafter.prepare_input(None, clip), np.stack(clip["intrinsics"], 0)
nl, na = make_noise(T, H, W_, 0)
VARIANTS = (("a_g1", 1.0, "0"), ("b_g1.2_batched", G, "0"), ("c_g1.2_sequential", G, "1"))

peak = {}
for name, g, seq in VARIANTS:           # each variant's own workspace peak: one clip in a fresh context, default arena (24 GiB)
    os.environ["UG_CFG_SEQUENTIAL"] = seq
    p1 = DepthCrafterPipelineHIP.from_state(*states, cfgs=(u, v, c))
    p1.engine.set_inputs(frames, nl, na, K)
    p1.engine.set_guidance(g)
    p1.engine.run(STEPS, 8)
    peak[name] = p1.engine.workspace_peak()
    p1.engine.close()
    del p1

pipe = DepthCrafterPipelineHIP.from_state(*states, cfgs=(u, v, c), workspace_bytes=40 << 30)
eng = pipe.engine
eng.set_inputs(frames, nl, na, K)


def select(g, seq):
    os.environ["UG_CFG_SEQUENTIAL"] = seq
    eng.set_guidance(g)


for name, g, seq in VARIANTS:           # warm-up of every variant (code objects, lane plans)
    select(g, seq)
    eng.run(STEPS, 8)
    fr, _, _ = eng.get_outputs(frames=True, depth=False)
    assert np.isfinite(fr).all(), name
outs = {}
res = {name: [] for name, _, _ in VARIANTS}
for rnd in range(rounds):
    for name, g, seq in VARIANTS:
        select(g, seq)
        t0 = time.perf_counter(); eng.run(STEPS, 8); eng.run(STEPS, 8); dt = (time.perf_counter() - t0) / 2
        fr, _, _ = eng.get_outputs(frames=True, depth=False)
        assert np.isfinite(fr).all(), name
        outs[name] = fr
        res[name].append(dt)
        print(f"round {rnd} {name:18s}: {dt * 1e3:8.1f} ms/clip  {T / dt:6.2f} frames/s", flush=True)
select(1.0, "0")
print("summary (median over rounds; workspace peak = ug_workspace_peak of one clip of the variant in a fresh context, 24 GiB arena):")
for name, _, _ in VARIANTS:
    dt = float(np.median(res[name]))
    print(f"  {name:18s}: {dt * 1e3:8.1f} ms/clip  {T / dt:6.2f} frames/s  workspace peak {peak[name] / 2**30:6.2f} GiB", flush=True)
a, b, c = (float(np.median(res[n])) for n, _, _ in VARIANTS)
print(f"  (b) vs (c): {c / b:.3f} x  ((c) / (b) time, > 1.03 keeps the batched pass); (b) / (a) time {b / a:.3f}, (c) / (a) {c / a:.3f}")
print(f"  max |b - c| on the decoded frames: {float(np.abs(outs['b_g1.2_batched'] - outs['c_g1.2_sequential']).max()):.3e}; "
      f"max |a - b|: {float(np.abs(outs['a_g1'] - outs['b_g1.2_batched']).max()):.3e}")
eng.close()
