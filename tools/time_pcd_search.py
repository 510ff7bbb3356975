"""Brute force against the exact grid search on one synthetic cloud pair: a wavy surface seen by T jittered H x W
frames and a copy of it turned by 0.01 rad, shifted and perturbed - the case eval_pcd's ICP has to pull back.  Host clock around the calls
(uploads and downloads included), one process, every step under its own limit: a step that overruns it ends the process, so nothing else is
started on the device after it.

    python tools/time_pcd_search.py --shape 4 256 256 --keep 1.0            # 262 144 points per cloud: one pass and the whole call, both ways
    python tools/time_pcd_search.py --shape 25 384 512 --keep 0.75 --skip-nn   # about 3.7 M masked points: brute force answers with the pair cap

Every timed step runs --repeat times (default 5) and reports the median with its spread.  Prints one line per step and a last line of JSON."""
import argparse
import faulthandler
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def clip_clouds(T, H, W, keep, seed=0, noise=0.002):
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.linspace(-1, 1, W), np.linspace(-1, 1, H), indexing="xy")
    xy = np.stack([np.broadcast_to(u, (T, H, W)), np.broadcast_to(v, (T, H, W))], -1) + rng.uniform(-0.5, 0.5, (T, H, W, 2)) * (2.0 / max(H, W))
    gt = np.concatenate([xy, (0.2 * np.sin(3.0 * xy[..., 0]) * np.cos(2.0 * xy[..., 1]) + 0.1 * xy[..., 0] + 3.0)[..., None]], -1)
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(0.01) * K + (1 - np.cos(0.01)) * (K @ K)
    pred = gt @ R.T + np.array([0.01, -0.005, 0.008]) + rng.normal(0.0, noise, gt.shape)
    mask = rng.uniform(size=(T, H, W)) < keep
    return pred.astype(np.float32), gt.astype(np.float32), mask


def step(name, limit, fn, record, repeat=1):
    """Runs fn `repeat` times (once after an error) under one limit for all of them -> its last result; records the median and the spread."""
    faulthandler.dump_traceback_later(limit, exit=True)      # the whole process ends at the limit: no later step touches the device
    times, out, err = [], None, None
    for _ in range(repeat):
        t0 = time.perf_counter()
        try:
            out = fn()
        except RuntimeError as e:
            out, err = None, str(e)
        times.append(time.perf_counter() - t0)
        if err:
            break
    faulthandler.cancel_dump_traceback_later()
    med = float(np.median(times))
    record[name] = {"seconds": round(med, 5), "min": round(min(times), 5), "max": round(max(times), 5), "runs": len(times), "error": err}
    print(f"{name}: median {med:.4f} s of {len(times)} (min {min(times):.4f}, max {max(times):.4f})" + (f"  ERROR {err[:160]}" if err else ""),
          flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=[4, 256, 256], metavar=("T", "H", "W"))
    ap.add_argument("--keep", type=float, default=1.0, help="share of the pixels the mask keeps")
    ap.add_argument("--limit", type=int, default=300, help="seconds one step (all its repeats) may take")
    ap.add_argument("--repeat", type=int, default=5, help="runs per timed step: the median and the spread are reported")
    ap.add_argument("--workspace-gib", type=float, default=4.0)
    ap.add_argument("--skip-nn", action="store_true", help="no single nearest-neighbour pass (its brute-force side needs nq * nt <= 2^40)")
    ap.add_argument("--skip-brute-call", action="store_true")
    args = ap.parse_args()

    from unigeo_amd._lib import Engine
    pred, gt, mask = clip_clouds(*args.shape, args.keep)
    n = int(mask.sum())
    rec = {"shape": args.shape, "points": n}
    print(f"clip {tuple(args.shape)}: {n} masked points per cloud", flush=True)
    eng = Engine(0, workspace_bytes=int(args.workspace_gib * (1 << 30)), persist_bytes=1 << 20)
    same = lambda a, b: all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() for k in eng.PCD_KEYS) and \
        a["transformation"].tobytes() == b["transformation"].tobytes() and a["icp_iterations"] == b["icp_iterations"]
    try:
        step("warm-up (eval_pcd, 4096 points, both searches)", args.limit,
             lambda: [eng.eval_pcd(pred, gt, mask, downsample_num=4096, return_clouds=False, search=s) for s in ("brute", "grid")], rec)
        if not args.skip_nn:
            q, t = pred.reshape(-1, 3)[mask.reshape(-1)].astype(np.float64), gt.reshape(-1, 3)[mask.reshape(-1)].astype(np.float64)
            b = step("one nearest-neighbour pass, brute", args.limit, lambda: eng.op_pcd_nn(q, t), rec, args.repeat)
            g = step("one nearest-neighbour pass, grid", args.limit, lambda: eng.op_pcd_nn_grid(q, t), rec, args.repeat)
            if b is not None and g is not None:
                rec["nn_same_bytes"] = bool(b[0].tobytes() == g[0].tobytes() and b[1].tobytes() == g[1].tobytes())
                rec["nn_stats"] = g[2]
                print(f"  same bytes: {rec['nn_same_bytes']}  {g[2]}", flush=True)
        b = None
        if not args.skip_brute_call:
            b = step("whole call, search=brute", args.limit, lambda: eng.eval_pcd(pred, gt, mask, return_clouds=False), rec, args.repeat)
        g = step("whole call, search=grid", args.limit, lambda: eng.eval_pcd(pred, gt, mask, return_clouds=False, search="grid"), rec,
                 args.repeat)
        if g is not None:
            st = g["search_stats"]
            rec["call_stats"] = st
            rec["call_leftover_share"] = st["leftover"] / max(1, st["settled"] + st["leftover"])
            rec["icp_iterations"] = g["icp_iterations"]
            rec["metrics"] = {k: g[k] for k in eng.PCD_KEYS}
            print(f"  iterations {g['icp_iterations']}  {st}  leftover share {rec['call_leftover_share']:.5f}", flush=True)
            if b is not None:
                rec["call_same_bytes"] = bool(same(b, g))
                print(f"  same bytes: {rec['call_same_bytes']}", flush=True)
    finally:
        eng.close()
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
