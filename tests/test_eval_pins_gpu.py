"""GPU: every on-device evaluation entry point returns the bytes that tests/golden/eval_pins.npz holds - recorded by
tests/golden/make_eval_pins.py from the build of the commit before the evaluation kernels were folded onto one reduction
(kernels/eval_reduce.h), one fit kernel and one metric kernel.  The cases, their sizes and their seeded inputs live in
tests/eval_pin_cases.py.  Also the one edge that the fold moved: a NaN prediction on a valid pixel of ug_eval_depth."""
import os

import numpy as np
import pytest

from eval_pin_cases import CASES

pytestmark = pytest.mark.gpu

PINS = np.load(os.path.join(os.path.dirname(__file__), "golden", "eval_pins.npz"), allow_pickle=False)


def test_the_pins_cover_the_cases_and_nothing_else():
    assert {k.split("/")[0] for k in PINS.files} == set(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_the_bytes_are_the_pinned_ones(engine, name):
    got = CASES[name](engine)
    assert sorted(f"{name}/{k}" for k in got) == sorted(k for k in PINS.files if k.startswith(name + "/"))
    for key, val in got.items():
        want = PINS[f"{name}/{key}"]
        val = np.ascontiguousarray(val)
        assert val.dtype == want.dtype and val.shape == want.shape, key
        assert val.tobytes() == want.tobytes(), f"{key}: got {val.ravel()[:13]} pinned {want.ravel()[:13]}"


def test_a_nan_prediction_on_a_valid_pixel_gives_a_nan_scale(engine):
    """Outside the contract (include/unigeo_hip.h): the call still returns, s is NaN and the pixels are counted as numpy counts them."""
    rng = np.random.default_rng(3)
    gt = rng.uniform(0.5, 6.0, 257).astype(np.float32)
    gt[::9] = 0.0
    pred = (0.7 * gt + 0.3).astype(np.float32)
    mask = rng.uniform(size=257) > 0.2
    gt[5], mask[5], pred[5] = 2.0, True, np.nan
    res, (s, _) = engine.eval_depth(gt, mask, pred=pred)
    assert np.isnan(s) and res["valid_pixels"] == int(((gt > 0) & (gt < 80.0) & mask).sum())
