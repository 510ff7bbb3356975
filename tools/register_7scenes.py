#!/usr/bin/env python
"""python tools/register_7scenes.py ROOT (--scenes chess/seq-03 ... | --split-file FILE) [--device [ID]] [--invalid drop] [--overwrite] [--batch 17]
Writes ``frame-*.depth.proj.png`` next to every raw ``frame-*.depth.png`` of the named 7-Scenes sequences: the Kinect depth warped into the
colour camera, as 16-bit PNG through Pillow.  The batch replacement for the reference's
``dataset/sevenScenes/preprocess.py`` - the same files, bit for bit, without scikit-image, joblib or its loop over every pixel - for whoever
wants the files on disk; ``sevenScenesDataset(register=...)`` needs none of them.

ROOT is the 7-Scenes folder; a scene is a path below it that holds the frames (``chess/seq-03``), named on the command line or one per line in
--split-file.  Without --device the numpy mirror runs; with it the GPU does (no fallback).  --invalid drop leaves raw 65535, the dataset's
marker of an invalid pixel, out - NOT what the reference's files hold.  An existing output is kept unless --overwrite is given."""
import argparse
import glob
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unigeo_amd.harness.rgbd import SEVEN_SCENES_SIZE, register_depth


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[1])
    ap.add_argument("root")
    ap.add_argument("--scenes", nargs="+"); ap.add_argument("--split-file")
    ap.add_argument("--device", nargs="?", type=int, const=0, default=None); ap.add_argument("--invalid", choices=("keep", "drop"), default="keep")
    ap.add_argument("--overwrite", action="store_true"); ap.add_argument("--batch", type=int, default=17)
    a = ap.parse_args(argv)
    if (a.scenes is None) == (a.split_file is None):
        ap.error("name the sequences with --scenes or with --split-file")
    scenes = a.scenes
    if scenes is None:
        with open(a.split_file) as f:
            scenes = [ln.strip() for ln in f.read().splitlines() if ln.strip()]
    if a.device is None:
        run = lambda clip: register_depth(clip, a.invalid)
    else:
        from unigeo_amd._lib import Engine                    # raises without the library or a GPU
        eng = Engine(a.device, workspace_bytes=256 << 20, persist_bytes=1 << 20)
        run = lambda clip: eng.prep_register_depth(clip, invalid=a.invalid)
    written = kept = 0
    for sc in scenes:
        base = os.path.join(a.root, sc)
        if not os.path.isdir(base):
            raise FileNotFoundError(f"7-Scenes sequence not found: {base}")
        todo, had = [], kept
        for src in sorted(glob.glob(os.path.join(base, "*.depth.png"))):
            dst = src[:-len("depth.png")] + "depth.proj.png"
            if os.path.exists(dst) and not a.overwrite:
                kept += 1
            else:
                todo.append((src, dst))
        for i in range(0, len(todo), max(a.batch, 1)):
            part = todo[i:i + max(a.batch, 1)]
            frames = []
            for src, _ in part:
                d = np.array(Image.open(src))
                if d.shape != SEVEN_SCENES_SIZE or d.dtype.kind not in "ui" or d.min() < 0 or d.max() > 65535:
                    raise ValueError(f"{src}: raw 7-Scenes depth is one 16-bit channel of {SEVEN_SCENES_SIZE[0]} x {SEVEN_SCENES_SIZE[1]}")
                frames.append(d.astype(np.uint16))
            for (_, dst), out in zip(part, run(np.stack(frames))):
                Image.fromarray(out).save(dst)
                written += 1
        print(f"{sc}: {len(todo)} of {len(todo) + kept - had} frames registered")
    print(f"{written} files written, {kept} existing files kept")
    return written


if __name__ == "__main__":
    main()
