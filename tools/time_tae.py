"""Temporal alignment error on the device against its numpy mirror on one synthetic clip: a smooth surface with a
step edge seen by a camera that turns about 0.03 rad and moves a few centimetres per frame, 1 % noise on the prediction, 5 % invalid ground
truth, a random mask.  One process, the two legs interleaved run by run, so that both see the same machine state.  The device leg is
`Engine.eval_tae` with the prediction passed from the host - the relative poses built on the host, the uploads of prediction, ground truth,
mask and tables, the fill, the splat, the score and the readback of the block partials - bracketed by two HIP events on the default stream
(the call returns with its own stream idle, so the events enclose all of it) and by the host clock; the host leg is
`temporal_alignment_error` under the host clock.  Neither leg asks for the maps.  A step that overruns its limit ends the process, so nothing
else is started on the device after it.

    python tools/time_tae.py                              # 25 x 384 x 512, stride 1
    python tools/time_tae.py --shape 3 520 512 --repeat 7

Prints one line per run and a last line of JSON: the medians with their spread, and whether the two legs agree."""
import argparse
import faulthandler
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_clip(shape, seed=0):
    T, H, W = shape
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    clean = np.stack([2.0 + 0.5 * np.sin(3.0 * x + 0.2 * t) + 0.3 * np.cos(2.0 * y - 0.1 * t) + (x + 0.3 * y > 0.7 + 0.02 * t) for t in range(T)], 0)
    gt = clean.astype(np.float32)
    gt[rng.uniform(size=shape) < 0.05] = 0.0
    pred = ((clean * (1.0 + 0.01 * rng.standard_normal(shape)) - 0.1) / 1.7).astype(np.float32)
    K = np.tile(np.array([[0.9 * W, 0, W / 2], [0, 0.9 * W, H / 2], [0, 0, 1]], np.float32), (T, 1, 1))
    poses, cur = np.zeros((T, 4, 4), np.float32), np.eye(4)
    for t in range(T):
        poses[t] = cur
        a = 0.03
        step = np.array([[math.cos(a), 0, math.sin(a), 0.04], [0, 1, 0, 0.01], [-math.sin(a), 0, math.cos(a), 0.02], [0, 0, 0, 1]])
        cur = cur @ step
    return pred, gt, rng.uniform(size=shape) > 0.2, K, poses, (np.float32(1.7), np.float32(0.1))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=[25, 384, 512], metavar=("T", "H", "W"))
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds one run of one leg may take")
    ap.add_argument("--workspace-gib", type=float, default=2.0)
    args = ap.parse_args()
    if args.repeat < 1:
        ap.error("--repeat must be at least 1")

    import torch
    from unigeo_amd._lib import Engine
    from unigeo_amd.harness import temporal_alignment_error
    pred, gt, mask, K, poses, fit = synthetic_clip(tuple(args.shape))
    print(f"clip {tuple(args.shape)}: {gt.size} pixels, {2 * max(args.shape[0] - args.stride, 0)} directed pairs", flush=True)
    eng = Engine(0, workspace_bytes=int(args.workspace_gib * (1 << 30)), persist_bytes=1 << 20)
    dev_ev, dev_clock, host_clock = [], [], []
    close = lambda a, b: bool(a["TAE pixels"] == b["TAE pixels"] and abs(a["TAE"] - b["TAE"]) <= 1e-10 * abs(b["TAE"]))
    try:
        faulthandler.dump_traceback_later(args.limit, exit=True)
        eng.eval_tae(gt, poses, K, fit, mask, pred=pred, stride=args.stride)      # warm-up: code objects loaded, clocks up
        faulthandler.cancel_dump_traceback_later()
        for i in range(args.repeat):
            faulthandler.dump_traceback_later(args.limit, exit=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            dres = eng.eval_tae(gt, poses, K, fit, mask, pred=pred, stride=args.stride)
            e1.record()
            e1.synchronize()
            dev_clock.append(time.perf_counter() - t0)
            dev_ev.append(e0.elapsed_time(e1) / 1e3)
            faulthandler.cancel_dump_traceback_later()
            faulthandler.dump_traceback_later(args.limit, exit=True)
            t0 = time.perf_counter()
            hres = temporal_alignment_error(pred, gt, poses, K, fit, custom_mask=mask, stride=args.stride)
            host_clock.append(time.perf_counter() - t0)
            faulthandler.cancel_dump_traceback_later()
            print(f"run {i}: device {dev_ev[-1]:.4f} s (events) {dev_clock[-1]:.4f} s (host clock), host mirror {host_clock[-1]:.3f} s, "
                  f"agree: {close(dres, hres)}", flush=True)
    finally:
        eng.close()
    stat = lambda v: {"median": round(float(np.median(v)), 5), "min": round(min(v), 5), "max": round(max(v), 5)}
    print(json.dumps({"shape": args.shape, "pixels": int(gt.size), "stride": args.stride, "runs": args.repeat, "device_events_s": stat(dev_ev),
                      "device_host_clock_s": stat(dev_clock), "host_mirror_s": stat(host_clock), "tae_device": dres["TAE"], "tae_host": hres["TAE"],
                      "pairs": dres["TAE pairs"], "pixels_scored": dres["TAE pixels"], "agree": close(dres, hres)}))


if __name__ == "__main__":
    main()
