#!/usr/bin/env python
"""python tests/golden/make_gt_normals_golden.py --reference <UniGeo checkout>
Golden for the normals fitted from depth (unigeo_amd/harness/normals.py ``fit_normals``, ``ug_prep_gt_normals``): runs
the REFERENCE's own ``get_surface_normal_np`` (utils/geometry_utils.py:73-134, patch_size 5) on hole-free float32 point frames and stores its
answers in tests/golden/gt_normals_golden.npz.  ``cv2``, which that module imports and this path never calls, is stubbed.  Runs where the
reference is checked out, never in a test.

The frames are 24 x 32 - multiples of 4: the reference solves in 4 x 4 blocks of int(size / 4) pixels and leaves the remainder rows and
columns as the random numbers it starts from - back-projected with focal 40 from millimetre depth by the float32 loaders' arithmetic
(tests/gt_normals_fixtures.py): the tilted plane at 2 m, the frontal plane at 3.5 m, and a curved surface (a paraboloid bowl) so that the pin
is not about planes alone.  The reference zero-pads its window sums ('same' convolution), so only pixels at least 2 from the border are its
fit; the test compares those.

The file holds
  points       float32 [3,3,24,32]  the input frames, OpenGL camera coordinates, channel first (fit_normals' layout)
  ref32        float32 [3,24,32,3]  get_surface_normal_np on the float32 points
  noise_deg    float64 [3]          per frame, the largest interior angle between that and get_surface_normal_np on the same points widened
                                    to float64: the reference's own float32 noise, the pin's bound (the test allows twice it)
  quant_deg    float64 [2]          tilted, frontal: the largest interior angle between the float64 run on the millimetre-quantised plane and the
                                    plane's analytic normal - what the quantisation costs a full 5 x 5 window; the analytic test adds it to
                                    the distance of an unquantised fit
  quant_scene_deg float64 [2]       tilted, frontal: the same distance on the fixtures' two-plane scene with its hole, its 65535 pixel and its
                                    step (radius 2, edge 0.05, majority count), over the valid pixels at least 2 columns from the step, from
                                    gt_normals_fixtures.loop_fit - a per-pixel numpy.linalg.solve in float64, independent of fit_normals.  A
                                    window cut by the hole or the border holds fewer points and pays more for the quantisation than a full one
Angles are taken between renormalised vectors with atan2(|a x b|, a . b) (gt_normals_fixtures.angle_deg)."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))                    # tests/: gt_normals_fixtures
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))   # the repository: unigeo_amd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("UNIGEO_REFERENCE"), required="UNIGEO_REFERENCE" not in os.environ,
                    help="a checkout of the reference (UniGeo); it is only read")
    ref = ap.parse_args().reference
    sys.modules["cv2"] = types.ModuleType("cv2")
    spec = importlib.util.spec_from_file_location("ref_geometry_utils", os.path.join(ref, "utils", "geometry_utils.py"))
    geom = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(geom)
    import gt_normals_fixtures as fx

    u, v = np.meshgrid(np.arange(fx.W), np.arange(fx.H))
    bowl = 2.5 + 0.002 * ((u - 14.0) ** 2 + 1.5 * (v - 10.0) ** 2)                       # metres; curved everywhere
    depths = [fx.plane_depth(fx.N_TILT, fx.D_TILT, fx.K40), fx.plane_depth(fx.N_FRONT, fx.D_FRONT, fx.K40), bowl]
    points = np.stack([fx.backproject(fx.quantise(d), fx.K40)[0] for d in depths])        # float32 [3,3,H,W]; no hole: every mask is full
    I = (slice(2, fx.H - 2), slice(2, fx.W - 2))
    ref32, noise, quant = [], [], []
    for p in points:
        hw3 = np.ascontiguousarray(p.transpose(1, 2, 0))
        np.random.seed(0)                                                                 # the remainder rows it would leave random: none at 24 x 32
        a = geom.get_surface_normal_np(hw3)
        np.random.seed(0)
        b = geom.get_surface_normal_np(hw3.astype(np.float64))
        assert a.dtype == np.float32 and a.shape == (fx.H, fx.W, 3)
        ref32.append(a)
        noise.append(fx.angle_deg(a[I], b[I]).max())
        if len(ref32) <= 2:                                                               # the two planes: what the quantisation costs
            quant.append(fx.angle_deg(b[I], fx.truth_gl((fx.N_TILT, fx.N_FRONT)[len(ref32) - 1])).max())
    c, mask = fx.backproject(fx.scene_raw()[0], fx.K40)
    N, ok, _ = fx.loop_fit(c.transpose(1, 2, 0), mask)
    scene = [fx.angle_deg(N[:, cols][ok[:, cols]], fx.truth_gl(n)).max()
             for cols, n in ((slice(0, fx.STEP - 2), fx.N_TILT), (slice(fx.STEP + 2, fx.W), fx.N_FRONT))]
    np.savez_compressed(os.path.join(OUT, "gt_normals_golden.npz"), points=points, ref32=np.stack(ref32), noise_deg=np.array(noise),
                        quant_deg=np.array(quant), quant_scene_deg=np.array(scene))
    print("noise_deg", noise, "quant_deg", quant, "quant_scene_deg", scene)


if __name__ == "__main__":
    main()
