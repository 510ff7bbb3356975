"""CPU: the pieces of bench.py's plain run that need no GPU - the seeded weight synthesis and --dump-outputs."""
import numpy as np

import bench
from unigeo_amd import weights as W


def test_random_state_tiled_tensors_equal_the_plain_formula():
    """random_state scales and casts the 4M-sample block of a big tensor before tiling it: the same bits as tiling first (what the benchmark's
    weights, the full-size goldens and every seeded test were made with)."""
    man = {"big.weight": (1100, 4000), "small.weight": (64, 32), "small.bias": (64,)}
    got = W.random_state(man, 5)
    rng = np.random.default_rng(5)
    big = np.resize(rng.standard_normal(1 << 22, dtype=np.float32), 1100 * 4000).reshape(1100, 4000) * np.float32(1.0 / np.sqrt(4000))
    small = rng.standard_normal((64, 32), dtype=np.float32) * np.float32(1.0 / np.sqrt(32))
    bias = 0.05 * rng.standard_normal(64)
    for name, want in (("big.weight", big), ("small.weight", small), ("small.bias", bias)):
        a = got[name]
        assert a.dtype == np.float16 and a.flags.c_contiguous and a.tobytes() == want.astype(np.float16).tobytes(), name


def test_dump_outputs_fits_the_budget_with_a_fixed_sample(tmp_path):
    """The headline clip's outputs (depth [25,384,512], decoded frames [25,384,512,3]: 79 MB of float32) within 64 MB: depth whole, then a
    seeded sample of the frames that is the same in every run."""
    rng = np.random.default_rng(1)
    depth = rng.random((25, 384, 512), dtype=np.float32)
    frames = rng.random((25, 384, 512, 3), dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("depth", depth), ("frames", frames)])
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["depth.npy", "frames_sample.npy"]
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 64_000_000
    assert np.array_equal(np.load(tmp_path / "a" / "depth.npy"), depth)
    s = np.load(tmp_path / "a" / "frames_sample.npy")
    assert s.dtype == np.float32 and s.size > frames.size // 2
    idx = np.sort(np.random.default_rng(0).choice(frames.size, s.size, replace=False))
    assert np.array_equal(s, frames.reshape(-1)[idx])
    for f in files:
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes()
