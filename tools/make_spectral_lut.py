#!/usr/bin/env python
"""Writes unigeo_amd/harness/spectral_r_lut.txt: the 256 RGB entries of matplotlib's Spectral_r colour map - the table the visualisation
panels colour depth with - as text, one "r g b" row per entry, each value the shortest decimal that reads back as
matplotlib's float64; harness/vis.py rounds them to float32 as the reference's pipeline does.  Shipped as data so that the panels need no
matplotlib where they are composed; tests/test_vis_cpu.py compares it with matplotlib's table when matplotlib is importable."""
import os

import matplotlib
import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unigeo_amd", "harness", "spectral_r_lut.txt")
lut = matplotlib.colormaps["Spectral_r"](np.arange(256))[:, :3]
assert lut.shape == (256, 3) and lut.dtype == np.float64 and lut.min() >= 0 and lut.max() <= 1
with open(OUT, "w") as f:
    f.write("# matplotlib Spectral_r, 256 rows of r g b in [0,1]; written by tools/make_spectral_lut.py\n")
    for row in lut:
        f.write(" ".join(repr(float(v)) for v in row) + "\n")
assert np.array_equal(np.loadtxt(OUT, dtype=np.float64), lut)
print("wrote", OUT, lut.shape, "matplotlib", matplotlib.__version__)
