#!/usr/bin/env python
"""Wall time of DepthCrafter.forward(data) as reference eval.py:39 calls it (torch imported first) on the full-size synthetic clip, beside the bare ug_dc_run with resident inputs.

--noise host (default): the default input path (host noise + prefetch thread, float32 frames).
--noise device: a second plugin instance on the SAME pipeline in the device input mode (uint8 frames, noise generated on the GPU from the seed);
the two legs alternate clip by clip in one process, so that they see the same box in the same state.  Medians and spread (min .. max) per leg."""
import argparse, os, sys, time
import torch  # noqa: F401  (first, as eval.py does)
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unigeo_amd.pipeline import DepthCrafterPipelineHIP
from unigeo_amd.synthetic import synthetic_clip
from unigeo_amd.model.depthcrafter import DepthCrafter
ap = argparse.ArgumentParser()
ap.add_argument("--noise", choices=("host", "device"), default="host")
ap.add_argument("--clips", type=int, default=5, help="timed clips per leg")
args = ap.parse_args()
T, H, W = 25, 384, 512
pipe = DepthCrafterPipelineHIP.from_random(seed=42, workspace_bytes=40 << 30)


def plugin(noise):
    plug = DepthCrafter.__new__(DepthCrafter)
    plug.pipeline, plug.num_inference_steps, plug.seed, plug._calls, plug.device, plug.noise = pipe, 25, 0, 0, "hip:0", noise
    return plug


legs = {"host": plugin("host")}
if args.noise == "device":
    legs["device"] = plugin("device")
data = synthetic_clip(T, H, W, seed=1234)
for _ in range(2):
    for plug in legs.values():
        plug.forward(data)
ts = {k: [] for k in legs}
for _ in range(args.clips):
    for k, plug in legs.items():
        t0 = time.perf_counter(); out = plug.forward(data); ts[k].append(time.perf_counter() - t0)
for k, t in ts.items():
    print(f"forward(data) noise={k} ms:", " ".join(f"{x * 1e3:.1f}" for x in t),
          f"median {np.median(t) * 1e3:.1f} spread {min(t) * 1e3:.1f} .. {max(t) * 1e3:.1f} best {T / min(t):.2f} frames/s", flush=True)
eng = pipe.engine
tr = []
for _ in range(3):
    t0 = time.perf_counter(); eng.run(25, 8, with_normals=True); tr.append(time.perf_counter() - t0)
print("ug_dc_run (resident inputs, with normals) ms:", " ".join(f"{t * 1e3:.1f}" for t in tr), f"best {T / min(tr):.2f} frames/s")
# the input step alone (upload + conversions / generation, ends in a stream synchronise), alternating
if args.noise == "device":
    from unigeo_amd.pipeline import make_noise
    f32 = legs["host"].prepare_input(data)
    u8 = np.stack([np.asarray(x).astype(np.uint8) for x in data["images"]], 0)
    K = np.stack(data["intrinsics"], 0)
    nl, na = make_noise(T, H, W, 0)
    tu = {"set_inputs (float32 frames, host noise)": [], "set_inputs_ex (uint8 frames, seed)": []}
    for i in range(6):
        t0 = time.perf_counter(); eng.set_inputs(f32, nl, na, K); t1 = time.perf_counter(); eng.set_inputs_ex(u8, seed=i, intrinsics=K); t2 = time.perf_counter()
        if i:
            tu["set_inputs (float32 frames, host noise)"].append(t1 - t0); tu["set_inputs_ex (uint8 frames, seed)"].append(t2 - t1)
    for k, t in tu.items():
        print(f"{k} ms:", " ".join(f"{x * 1e3:.2f}" for x in t), f"median {np.median(t) * 1e3:.2f}")
    t0 = time.perf_counter(); make_noise(T, H, W, 1); print(f"make_noise (host draw) ms: {(time.perf_counter() - t0) * 1e3:.1f}")
