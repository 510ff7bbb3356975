"""Wall time of the point-map step on one synthetic clip: T cameras of focal f looking at a wavy surface, each turned and
moved a little further than the one before, points rounded to float32 with optional noise.  Host clock around engine.pointmap_focal and
engine.pointmap_poses (uploads and downloads included), one process, every step under its own limit: a step that overruns it ends the process,
so nothing else is started on the device after it.

    python tools/time_pointmap.py                               # 25 x 384 x 512
    python tools/time_pointmap.py --shape 3 24 32 --mirror      # also the numpy mirror's time, and how far the device lies from it

Every timed step runs --repeat times (default 3) and reports the median with its spread.  Prints one line per step and a last line of JSON."""
import argparse
import faulthandler
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def clip_points(T, H, W, f, noise, seed=0):
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    z = 2.25 + 0.6 * np.sin(u / (W / 5.0)) * np.cos(v / (H / 4.0)) + rng.uniform(-0.1, 0.1, (H, W))
    ext = np.tile(np.eye(4), (T, 1, 1))
    pts = np.zeros((T, H, W, 3))
    for k in range(T):
        a = 0.02 * k                                            # about 1.1 degrees and 2 cm a frame
        ca, sa = np.cos(a), np.sin(a)
        ext[k, :3, :3] = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]]) @ np.array([[1, 0, 0], [0, np.cos(a / 2), -np.sin(a / 2)], [0, np.sin(a / 2), np.cos(a / 2)]])
        ext[k, :3, 3] = [0.02 * k, 0.01 * np.sin(0.5 * k), 0.005 * k]
        cam = np.stack([(u - W / 2) * z / f, (v - H / 2) * z / f, z], -1)
        pts[k] = (cam - ext[k, :3, 3]) @ ext[k, :3, :3]
    if noise:
        pts += rng.normal(0, noise, pts.shape)
    return pts.astype(np.float32), ext


def step(name, limit, fn, record, repeat=1):
    faulthandler.dump_traceback_later(limit, exit=True)      # the whole process ends at the limit: no later step touches the device
    times, out = [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    faulthandler.cancel_dump_traceback_later()
    med = float(np.median(times))
    record[name] = {"seconds": round(med, 5), "min": round(min(times), 5), "max": round(max(times), 5), "runs": len(times)}
    print(f"{name}: median {med:.4f} s of {len(times)} (min {min(times):.4f}, max {max(times):.4f})", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=[25, 384, 512], metavar=("T", "H", "W"))
    ap.add_argument("--focal", type=float, default=None, help="focal of the synthetic cameras (default 0.8 * W)")
    ap.add_argument("--noise", type=float, default=0.005, help="Gaussian sigma added to the points, metres")
    ap.add_argument("--limit", type=int, default=120, help="seconds one step (all its repeats) may take")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--mirror", action="store_true", help="also run harness/pointmap.py on the host (slow at full size)")
    args = ap.parse_args()

    from unigeo_amd._lib import Engine
    T, H, W = args.shape
    f_true = args.focal or 0.8 * W
    pts, ext = clip_points(T, H, W, f_true, args.noise)
    rec = {"shape": args.shape, "focal_true": f_true, "noise": args.noise}
    eng = Engine(0, workspace_bytes=1 << 30, persist_bytes=1 << 20)
    try:
        step("warm-up (one frame)", args.limit, lambda: eng.pointmap_poses(pts[:1], eng.pointmap_focal(pts[0])), rec)
        f = step("pointmap_focal", args.limit, lambda: eng.pointmap_focal(pts[0]), rec, args.repeat)
        res = step("pointmap_poses", args.limit, lambda: eng.pointmap_poses(pts, f), rec, args.repeat)
        rot = res["extrinsics"][:, :3, :3] @ ext[:, :3, :3].transpose(0, 2, 1)
        ang = np.degrees(np.arccos(np.clip((np.trace(rot, axis1=1, axis2=2) - 1) / 2, -1, 1)))
        rec.update(focal=f, iterations=int(res["iterations"].sum()), iterations_max=int(res["iterations"].max()),
                   inlier_share=float(res["n_inliers"].sum() / (T * H * W)), reproj_rms_max=float(res["reproj_rms"].max()),
                   rotation_error_deg_max=float(ang.max()), translation_error_max=float(np.linalg.norm(res["extrinsics"][:, :3, 3] - ext[:, :3, 3], axis=1).max()))
        print(f"  focal {f:.6f} (true {f_true}), {rec['iterations']} iterations over {T} frames (most {rec['iterations_max']}), inlier share "
              f"{rec['inlier_share']:.4f}, rotation error {rec['rotation_error_deg_max']:.3g} deg, translation error {rec['translation_error_max']:.3g} m", flush=True)
        if args.mirror:
            from unigeo_amd.harness.pointmap import pointmap_poses
            ref = step("numpy mirror, pointmap_poses", args.limit * 10, lambda: pointmap_poses(pts, focal=f), rec)
            rec["device_minus_mirror"] = float(np.abs(res["extrinsics"] - ref["extrinsics"]).max())
            rec["same_iterations"] = bool(np.array_equal(res["iterations"], ref["iterations"]))
            print(f"  |device - mirror| {rec['device_minus_mirror']:.3g}, same iteration counts: {rec['same_iterations']}", flush=True)
    finally:
        eng.close()
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
