"""Seeded on-device noise and uint8 frame upload, CPU side: the numpy restatement (tests/noise_oracle.py) against the
published Philox4x32-10 known answers, its statistics at the full clip size, the exported symbols, and the argument handling of the pipeline
call and the plugin with recording fakes (no GPU)."""
import os
import re
import threading
from types import SimpleNamespace

import numpy as np
import pytest

import noise_oracle as NO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT = ("ug_dc_set_inputs_ex", "ug_dc_get_noise")
TEST_ONLY = ("ug_op_philox_u32", "ug_op_randn", "ug_op_u8_to_frames")
FULL = (25, 384, 512)
SEEDS = (0, 7, 2 ** 40 + 3)


# ---------------------------------------------------------------------------------------------- 1. the yardstick
def _hex(words):
    return " ".join(f"{int(np.asarray(w).reshape(-1)[0]):08x}" for w in words)


def test_restatement_reproduces_the_random123_known_answers():
    assert _hex(NO.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _hex(NO.philox4x32_10((ones,) * 4, (ones, ones))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(NO.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # the counter / key layout of the definition: block q of (seed, stream) is counter (q lo, q hi, stream, 0) under key (seed lo, seed hi)
    q, seed = (5 << 32) | 9, (3 << 32) | 4
    got = NO.philox_blocks(seed, 1, q, 2)
    for i in range(2):
        want = NO.philox4x32_10((9 + i, 5, 1, 0), (4, 3))
        assert [int(w[0]) for w in want] == [int(v) for v in got[i]]
    # a block offset that carries into the second counter word
    got = NO.philox_blocks(0, 0, (1 << 32) - 1, 2)
    assert [int(v) for v in got[1]] == [int(w[0]) for w in NO.philox4x32_10((0, 1, 0, 0), (0, 0))]


def test_uniforms_are_exact_in_float32_and_inside_the_open_interval():
    x = np.array([0, 511, 512, 2 ** 32 - 1], dtype=np.uint32)
    u64, u32 = NO.uniform(x, np.float64), NO.uniform(x, np.float32)
    assert u32.dtype == np.float32
    want = [2.0 ** -24, 2.0 ** -24, 3 * 2.0 ** -24, 1.0 - 2.0 ** -24]
    assert u64.tolist() == want
    assert u32.astype(np.float64).tolist() == want                      # nothing rounded on the way through float32
    assert (u32 > 0).all() and (u32 < 1).all()
    assert NO.MAX_ABS == pytest.approx(5.768, abs=5e-4)
    assert np.sqrt(-2.0 * np.log(u64[0])) == pytest.approx(NO.MAX_ABS, rel=1e-12)


def test_randn_slices_are_consistent_with_the_element_index():
    """Element e depends on (seed, stream, e) only: any offset / length reads the same sequence."""
    full = NO.randn(11, 0, 0, 64)
    for e0, n in ((0, 5), (1, 6), (3, 7), (13, 17), (4, 8)):
        assert np.array_equal(NO.randn(11, 0, e0, n), full[e0:e0 + n])
    assert not np.array_equal(NO.randn(11, 1, 0, 64), full)
    assert not np.array_equal(NO.randn(11 + (1 << 32), 0, 0, 64), full)
    assert np.isfinite(full).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_restatement_stays_inside_the_statistical_bounds_at_full_size(seed):
    """The 5-sigma gates of the full-size GPU test, on the definition itself (measured when written: worst 1.7 sigma over the three seeds)."""
    lat, aug = NO.make_noise(*FULL, seed)
    assert aug.shape == (25, 3, 384, 512) and lat.shape == (25, 4, 48, 64)
    for name, val, bound in NO.moment_checks(lat, aug):
        print(f"seed {seed}: {name}: {val:.3e} (bound {bound:.3e}, {5 * val / bound:.2f} sigma)")
        assert val < bound, (seed, name, val, bound)
    assert max(np.abs(lat).max(), np.abs(aug).max()) <= NO.MAX_ABS


# ---------------------------------------------------------------------------------------------- 2. exports
def _declared(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return set(re.findall(r"\b(ug_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))


def test_new_entry_points_are_exported_and_declared_in_the_right_header():
    from unigeo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load_library()
    for s in PRODUCT + TEST_ONLY:
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS, s
    prod, test = _declared("unigeo_hip.h"), _declared("unigeo_hip_test.h")
    assert set(PRODUCT) <= prod
    assert set(TEST_ONLY) <= test
    assert not [s for s in prod if s.startswith("ug_op_")]
    assert "ug_dc_set_inputs" in prod                                   # the default entry point stays


# ---------------------------------------------------------------------------------------------- 3. pipeline call, recording engine
class _RecEngine:
    def __init__(self):
        self.log = []

    def set_inputs(self, *a, **kw):
        self.log.append(("set_inputs", a, kw)); self._thw = np.asarray(a[0]).shape[:3]

    def set_inputs_ex(self, frames, **kw):
        self.log.append(("set_inputs_ex", (frames,), kw))
        f = np.asarray(frames)
        self._thw = (f.shape[0], f.shape[2], f.shape[3]) if f.dtype == np.uint8 else f.shape[:3]

    def set_guidance(self, g):
        self.log.append(("set_guidance", (g,), {}))

    def run(self, *a, **kw):
        self.log.append(("run", a, kw))

    def get_outputs(self, frames=True, depth=True, normals=False):
        self.log.append(("get_outputs", (), {"frames": frames, "depth": depth, "normals": normals}))
        T, H, W = self._thw
        return np.zeros((T, H, W, 3), np.float32), np.zeros((T, H, W), np.float32), None


def _pipe():
    from unigeo_amd.pipeline import DepthCrafterPipelineHIP
    eng = _RecEngine()
    return DepthCrafterPipelineHIP(eng, None, None, None), eng


def _no_host_draw(monkeypatch):
    import unigeo_amd.pipeline as P

    def boom(*a, **kw):
        raise AssertionError("host noise drawn in device mode")
    monkeypatch.setattr(P, "make_noise", boom)


def test_device_mode_reaches_the_engine_as_a_seed_with_no_host_draw(monkeypatch):
    _no_host_draw(monkeypatch)
    pipe, eng = _pipe()
    u8 = np.arange(2 * 3 * 64 * 128, dtype=np.uint8).reshape(2, 3, 64, 128)
    out = pipe(u8, num_inference_steps=1, window_size=2, noise="device", seed=2 ** 40 + 3)
    assert out.depth.shape == (2, 64, 128)
    name, (frames,), kw = eng.log[0]
    assert name == "set_inputs_ex" and frames.dtype == np.uint8 and frames.shape == (2, 3, 64, 128) and np.array_equal(frames, u8)
    assert kw == {"seed": 2 ** 40 + 3, "intrinsics": None}
    assert [e[0] for e in eng.log] == ["set_inputs_ex", "set_guidance", "run", "get_outputs"]
    # float frames + device noise; the seed defaults to the pipeline's
    pipe, eng = _pipe()
    pipe.seed = 5
    f32 = np.zeros((2, 64, 64, 3), np.float32)
    pipe(f32, num_inference_steps=1, window_size=2, noise="device", height=64, width=64)
    name, (frames,), kw = eng.log[0]
    assert name == "set_inputs_ex" and frames.dtype == np.float32 and frames.shape == (2, 64, 64, 3) and kw["seed"] == 5
    assert "noise_latents" not in kw and "noise_aug" not in kw


def test_conflicting_arguments_and_bad_shapes_raise_before_the_engine_is_touched(monkeypatch):
    _no_host_draw(monkeypatch)
    from unigeo_amd.pipeline import make_noise  # noqa: F401  (patched: must not be reached)
    pipe, eng = _pipe()
    u8 = np.zeros((2, 3, 64, 64), np.uint8)
    nl, na = np.zeros((2, 4, 8, 8), np.float32), np.zeros((2, 3, 64, 64), np.float32)
    bad = [
        dict(video=u8, noise="device", noise_latents=nl, noise_aug=na),          # noise arrays together with device noise
        dict(video=u8, noise="device", noise_latents=nl),
        dict(video=u8, noise="device", noise_aug=na),
        dict(video=u8, noise="gpu"),                                             # any other value
        dict(video=u8, noise=None),
        dict(video=np.zeros((2, 64, 64, 3), np.uint8), noise="device"),          # uint8 must be planar
        dict(video=np.zeros((2, 3, 64), np.uint8), noise="device"),
        dict(video=np.zeros((2, 3, 64, 96), np.uint8), noise="device"),          # not multiples of 64
        dict(video=np.zeros((2, 3, 64, 64), np.float32), noise="device"),        # float input keeps today's checks: channels-last
        dict(video=u8, noise="device", height=32),
        dict(video=u8, noise="device", guidance_scale=float("nan")),
        dict(video=u8, noise="device", seed=-1),
        dict(video=u8, noise="device", seed=2 ** 64),
        dict(video=np.zeros((130, 3, 64, 64), np.uint8), noise="device", window_size=129),
    ]
    for kw in bad:
        kw = dict(kw)
        kw.setdefault("window_size", 2)
        with pytest.raises(ValueError):
            pipe(kw.pop("video"), num_inference_steps=1, **kw)
    assert eng.log == []


def test_default_calls_record_what_they_record_today():
    from unigeo_amd.pipeline import make_noise
    pipe, eng = _pipe()
    rng = np.random.default_rng(1)
    frames = rng.uniform(0, 1, (2, 64, 64, 3))                       # float64 in: converted to float32 as before
    K = np.tile(np.eye(3, dtype=np.float32), (2, 1, 1))
    pipe(frames, num_inference_steps=3, window_size=2, seed=9, intrinsics=K, with_normals=True, return_frames=False)
    assert [e[0] for e in eng.log] == ["set_inputs", "set_guidance", "run", "get_outputs"]
    name, a, kw = eng.log[0]
    assert kw == {} and len(a) == 4
    rl, ra = make_noise(2, 64, 64, 9)
    assert a[0].dtype == np.float32 and np.array_equal(a[0], frames.astype(np.float32))
    assert np.array_equal(a[1], rl) and np.array_equal(a[2], ra) and a[3] is K
    assert eng.log[1][1] == (1.0,)
    assert eng.log[2][1:] == ((3, 8), {"with_normals": True, "window": 0, "overlap": 25})
    assert eng.log[3][2] == {"frames": False, "depth": True, "normals": True}
    # explicit noise arrays: passed through untouched, no draw
    pipe, eng = _pipe()
    pipe(frames.astype(np.float32), num_inference_steps=1, window_size=2, noise_latents=rl, noise_aug=ra, noise="host")
    name, a, kw = eng.log[0]
    assert name == "set_inputs" and a[1] is rl and a[2] is ra and a[3] is None
    # uint8 planar frames with host noise: the extended call, noise drawn by make_noise(seed) as for float frames
    pipe, eng = _pipe()
    pipe(np.zeros((2, 3, 64, 64), np.uint8), num_inference_steps=1, window_size=2, seed=9)
    name, (f,), kw = eng.log[0]
    assert name == "set_inputs_ex" and f.dtype == np.uint8 and set(kw) == {"noise_latents", "noise_aug", "intrinsics"}
    assert np.array_equal(kw["noise_latents"], rl) and np.array_equal(kw["noise_aug"], ra)


# ---------------------------------------------------------------------------------------------- 4. plugin, recording pipeline
class _RecPipeline:
    def __init__(self):
        self.calls = []

    def __call__(self, frames, **kw):
        self.calls.append((frames, kw))
        T, _, H, W = frames.shape
        return SimpleNamespace(frames=[None], depth=np.ones((T, H, W), np.float32), normals=np.zeros((T, H, W, 3), np.float32))


def _data(T, H, W, index=None, seed=0):
    rng = np.random.default_rng(seed)
    d = {"images": [rng.uniform(0, 255, (3, H, W)).astype(np.float32) for _ in range(T)], "intrinsics": [np.eye(3, dtype=np.float32)] * T}
    if index is not None:
        d["_index"] = index
    return d


def _plugin(seed=7):
    from unigeo_amd.model.depthcrafter import DepthCrafter
    p = DepthCrafter.__new__(DepthCrafter)
    p.pipeline, p.num_inference_steps, p.seed, p._calls, p.device, p.noise = _RecPipeline(), 2, seed, 0, "cpu", "device"
    return p


def test_plugin_device_mode_starts_no_thread_and_passes_seed_and_uint8_frames(monkeypatch):
    _no_host_draw(monkeypatch)
    p = _plugin(seed=7)
    before = threading.active_count()
    plan = [(2, 64, 64, 0), (2, 64, 64, 1), (2, 64, 64, 10), (2, 64, 64, 18), (3, 64, 128, 4)]
    for T, H, W, idx in plan:
        d = _data(T, H, W, idx, seed=idx)
        out = p.forward(d)
        assert threading.active_count() == before
        assert getattr(p, "_noise_pf", None) is None
        assert tuple(out["pred_depths"].shape) == (T, H, W) and tuple(out["pred_normals"].shape) == (T, H, W, 3)
        frames, kw = p.pipeline.calls[-1]
        assert frames.dtype == np.uint8 and frames.shape == (T, 3, H, W)
        # the same pixels prepare_input would have made, before its transpose and division
        assert np.array_equal(frames.transpose(0, 2, 3, 1).astype(np.float32) / 255.0, p.prepare_input(d))
        assert kw["noise"] == "device" and kw["seed"] == 7 + idx
        assert kw.get("noise_latents") is None and kw.get("noise_aug") is None
        assert kw["height"] == H and kw["width"] == W and kw["with_normals"] is True and kw["return_frames"] is False
    # anonymous samples: the call counter (continues from the calls above)
    p = _plugin(seed=100)
    for k in range(3):
        p.forward(_data(2, 64, 64))
    assert [kw["seed"] for _, kw in p.pipeline.calls] == [100, 101, 102]
    assert threading.active_count() == before


def test_plugin_rejects_an_unknown_noise_mode_before_loading_anything():
    from unigeo_amd.model.depthcrafter import DepthCrafter
    with pytest.raises(ValueError):
        DepthCrafter(noise="cuda", synthetic_weights=True, tiny=True)
