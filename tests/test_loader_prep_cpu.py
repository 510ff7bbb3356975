"""CPU: the tables behind ``prep="device"`` of the ScanNet++ loader against the host recipe they restate -
``_resize`` through scipy - and the ``prep`` plumbing.  The device side is tests/test_loader_prep_gpu.py."""
import os

import numpy as np
import pytest

from unigeo_amd.harness import parse_dataset_config
from unigeo_amd.harness.scannetpp import ScannetPPDataset, _resize, resize_pick, resize_restated, resize_taps

ROOT = os.path.join(os.path.dirname(__file__), "golden", "scannetpp_scene")

# (Hi, Wi, Ho, Wo): plain, ragged, larger radii, up-scaling (no filter, mirrored zoom taps at the border), one axis unchanged
SHAPES = [(24, 32, 12, 16), (37, 53, 12, 16), (97, 131, 24, 32), (146, 219, 48, 64), (20, 28, 24, 40), (64, 96, 64, 32)]
# sources so small that the gaussian radius reaches or exceeds the axis length (the mirror wraps more than once).  Tried: all of these;
# scipy accepts every one and the restatement agrees (<= 3e-14), so none was dropped.
REACH = [(5, 7, 1, 2), (2, 2, 1, 1), (1, 6, 1, 1), (2, 3, 1, 1), (4, 4, 1, 1), (3, 3, 1, 2), (7, 2, 2, 1), (6, 1, 1, 1)]
TINY = REACH + [(3, 64, 2, 5)]          # radius 24 on 64 columns: does not reach the length, but the longest rows here (50 taps)
PAIRS = [(24, 12), (37, 12), (97, 24), (219, 64), (20, 24), (1168, 384), (1752, 512)]


def _radius(n_in, n_out):
    sigma = max(0.0, (n_in / n_out - 1) / 2)
    return int(4 * sigma + 0.5) if sigma > 0 else 0


@pytest.mark.parametrize("hi,wi,ho,wo", SHAPES + TINY)
def test_restated_resize_matches_the_scipy_recipe_in_float64(hi, wi, ho, wo):
    x = np.random.default_rng(hi * 1000 + wi).uniform(0, 255, (2, hi, wi))
    ref = _resize(x, ho, wo, 1, True)
    got = resize_restated(x, ho, wo)
    assert ref.dtype == np.float64 and got.dtype == np.float64 and got.shape == (2, ho, wo)
    err = np.abs(got - ref).max()
    print(f"{hi}x{wi}->{ho}x{wo}: max |restated - _resize| = {err:.2e}")
    assert err <= 1e-10


def test_tiny_sources_do_reach_the_radius():
    assert all(_radius(hi, ho) >= hi or _radius(wi, wo) >= wi for hi, wi, ho, wo in REACH)


@pytest.mark.parametrize("n_in,n_out", PAIRS + [(1, 1), (13, 13)])
def test_pick_tables_equal_the_order0_resize(n_in, n_out):
    ramp = np.arange(n_in, dtype=np.float64)
    pick = resize_pick(n_in, n_out)
    assert pick.dtype == np.int32 and pick.shape == (n_out,)
    rows = _resize(np.repeat(ramp[:, None], 3, 1), n_out, 3, 0, False)[:, 0]          # rows resized, columns untouched
    cols = _resize(np.repeat(ramp[None, :], 3, 0), 3, n_out, 0, False)[0]
    np.testing.assert_array_equal(rows, pick)
    np.testing.assert_array_equal(cols, pick)


@pytest.mark.parametrize("n_in,n_out", PAIRS + [(1, 1), (13, 13), (5, 1), (64, 5), (2, 1), (9, 2), (28, 40)])
def test_tap_tables_are_normalised_short_and_in_range(n_in, n_out):
    idx, w = resize_taps(n_in, n_out)
    assert idx.dtype == np.int32 and w.dtype == np.float64 and idx.shape == w.shape and idx.shape[0] == n_out
    assert np.abs(w.sum(1) - 1).max() <= 1e-15
    assert idx.shape[1] <= 2 * _radius(n_in, n_out) + 2
    assert idx.min() >= 0 and idx.max() < n_in and (w >= 0).all()
    if n_in == n_out:
        assert idx.shape[1] == 1 and (idx[:, 0] == np.arange(n_in)).all() and (w == 1).all()


def test_real_scale_reads_ten_rows():
    assert resize_taps(1168, 384)[0].shape[1] == 10


def test_prep_is_validated_and_forwarded():
    with pytest.raises(ValueError):
        ScannetPPDataset(ROOT, scenes=["sceneA"], clip_length=3, clip_overlap=1, prep="gpu")
    assert ScannetPPDataset(ROOT, scenes=["sceneA"], clip_length=3, clip_overlap=1).prep == "host"
    ds = ScannetPPDataset(ROOT, scenes=["sceneA"], clip_length=3, clip_overlap=1, prep="device", device_id=3)
    assert ds.prep == "device" and ds.device_id == 3 and ds.engine is None and len(ds) == 2       # the engine comes with the first sample
    cfg = {"root": ROOT, "h": 12, "w": 16}
    assert "prep" not in parse_dataset_config(cfg)
    assert parse_dataset_config(dict(cfg, prep="device"))["prep"] == "device"
    assert parse_dataset_config(dict(cfg, prep="host"))["prep"] == "host"
