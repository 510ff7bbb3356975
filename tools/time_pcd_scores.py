"""What the threshold scores and the voxel IoU add to one eval_pcd call: the same call with and without
``fscore_thresholds: [0.02, 0.05, 0.1]`` / ``voxel_sizes: [0.05]``, in one process, at the two sizes section 18 reports - 10 000 sampled
points with the brute-force search, and a 4 x 256 x 256 clip unsampled (262 144 points) with ``search: grid``.  The cloud pair is that of
tools/time_pcd_search.py.  Host clock around the calls (uploads and downloads included); every step runs --repeat times under one limit and
reports the median with its spread; a step that overruns its limit ends the process, so nothing else is started on the device after it.  No
bound is asserted: the added time is reported next to the call it is added to.

    python tools/time_pcd_scores.py

Prints one line per step and a last line of JSON."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

THRESHOLDS, VOXEL_SIZES = [0.02, 0.05, 0.1], [0.05]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=[4, 256, 256], metavar=("T", "H", "W"))
    ap.add_argument("--sampled", type=int, default=10000, help="points of the sampled, brute-force case")
    ap.add_argument("--limit", type=int, default=240, help="seconds one step (all its repeats) may take")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--workspace-gib", type=float, default=4.0)
    args = ap.parse_args()

    from time_pcd_search import clip_clouds, step
    from unigeo_amd._lib import Engine
    pred, gt, mask = clip_clouds(*args.shape, 1.0)
    rec = {"shape": args.shape, "points": int(mask.sum()), "fscore_thresholds": THRESHOLDS, "voxel_sizes": VOXEL_SIZES}
    eng = Engine(0, workspace_bytes=int(args.workspace_gib * (1 << 30)), persist_bytes=1 << 20)
    extra = {"fscore_thresholds": THRESHOLDS, "voxel_sizes": VOXEL_SIZES}
    cases = [(f"{args.sampled} sampled points, search=brute", {"downsample_num": args.sampled, "seed": 0}),
             (f"{rec['points']} points unsampled, search=grid", {"search": "grid"})]
    try:
        step("warm-up (4096 points, both searches, with the options)", args.limit,
             lambda: [eng.eval_pcd(pred, gt, mask, downsample_num=4096, return_clouds=False, search=s, **extra) for s in ("brute", "grid")], rec)
        for name, kw in cases:
            a = step(f"{name}: eval_pcd", args.limit, lambda: eng.eval_pcd(pred, gt, mask, return_clouds=False, **kw), rec, args.repeat)
            b = step(f"{name}: eval_pcd with the options", args.limit, lambda: eng.eval_pcd(pred, gt, mask, return_clouds=False, **kw, **extra), rec,
                     args.repeat)
            if a is None or b is None:
                continue
            t0, t1 = rec[f"{name}: eval_pcd"]["seconds"], rec[f"{name}: eval_pcd with the options"]["seconds"]
            same = all(a[k] == b[k] for k in eng.PCD_KEYS) and a["transformation"].tobytes() == b["transformation"].tobytes()
            rec[f"{name}: added"] = {"seconds": round(t1 - t0, 5), "share": round((t1 - t0) / t0, 4), "same_existing_outputs": bool(same),
                                     "scores": {k: v for k, v in b.items() if "@" in k}, "score_counts": b["score_counts"].tolist(),
                                     "voxel_counts": b["voxel_counts"].tolist()}
            print(f"  added {t1 - t0:+.4f} s ({100 * (t1 - t0) / t0:+.2f} %), existing outputs the same: {same}; {rec[f'{name}: added']['scores']}",
                  flush=True)
    finally:
        eng.close()
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
