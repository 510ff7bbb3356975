#!/usr/bin/env python
"""UG_LIB_PATH=<libunigeo_hip.so of the commit to pin> python tests/golden/make_eval_pins.py [--out FILE] [--compare FILE]
Pins for the on-device evaluation entry points (tests/test_eval_pins_gpu.py): runs every case of tests/eval_pin_cases.py - seeded inputs, made
again by the test and never stored - on the selected build of the library and writes what it returns to tests/golden/eval_pins.npz, one
array per ``<case>/<key>``: small outputs raw, per-pixel maps of more than 300 elements as the SHA-256 of their bytes.  Needs a GPU; run once,
on the build of the commit BEFORE a change that must not move a bit (a second ``git worktree`` of it, ``make -C unigeo_amd/csrc``), never in
a test.  ``--compare`` checks a second run against a written file instead of writing: a case that differs between two runs of one build
is not reproducible and cannot be pinned."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(HERE, "eval_pins.npz"))
    ap.add_argument("--compare", default=None)
    args = ap.parse_args()
    from eval_pin_cases import CASES
    from unigeo_amd import _lib
    print(f"library: {_lib.LIB_PATH}", flush=True)
    eng = _lib.Engine(0, workspace_bytes=2 << 30, persist_bytes=1 << 20)
    pins = {}
    try:
        for name, run in CASES.items():
            for key, val in run(eng).items():
                pins[f"{name}/{key}"] = np.ascontiguousarray(val)
            print(f"{name}: done", flush=True)
    finally:
        eng.close()
    if args.compare:
        ref = np.load(args.compare, allow_pickle=False)
        bad = sorted(k for k in set(ref.files) | set(pins) if k not in pins or k not in ref.files or ref[k].tobytes() != pins[k].tobytes())
        print(f"compared {len(pins)} arrays with {args.compare}: {len(bad)} differ {bad[:20]}")
        sys.exit(3 if bad else 0)
    np.savez_compressed(args.out, **pins)
    print(f"wrote {args.out}: {len(pins)} arrays, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
