"""Seeded on-device noise and uint8 frame upload on the MI355X: the generator kernel against the numpy restatement
(tests/noise_oracle.py) bit for bit on the raw words and within twice the float32 evaluation's own error on the normals, exact-n writes, the
statistics at the full clip size, the uint8 conversion bit for bit, and the device-mode pipeline against the default host-noise path with
NO tolerance (plain, windowed, guided, two contexts, the plugin).  Tiny full-topology configuration unless said otherwise."""
import threading

import numpy as np
import pytest

import noise_oracle as NO
from util import report

pytestmark = pytest.mark.gpu

FULL = (25, 384, 512)


@pytest.fixture(scope="module")
def tiny():
    from unigeo_amd.pipeline import DepthCrafterPipelineHIP
    from unigeo_amd import weights as W
    pipe = DepthCrafterPipelineHIP.from_random(seed=42, cfgs=W.tiny_cfgs(), workspace_bytes=3 << 30)
    yield pipe
    pipe.engine.set_guidance(1.0)
    pipe.engine.close()


@pytest.fixture(scope="module")
def floor():
    """The yardstick of every comparison of device normals with the definition: the definition evaluated in numpy float32 against its float64
    evaluation, max-abs over 8 M Box-Muller pairs (seed 7, noise_aug stream, blocks 0 .. 2^22 - 1).  Returns (floor, float64 reference)."""
    words = NO.philox_blocks(7, NO.STREAM_AUG, 0, 1 << 22)
    ref = NO.normals_from_words(words, np.float64).reshape(-1)
    fl = float(np.abs(NO.normals_from_words(words, np.float32).reshape(-1).astype(np.float64) - ref).max())
    assert 1e-6 < fl < 4e-6, fl                               # 2.0e-6 when this was written
    return fl, ref


def _u8_clip(T, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (T, 3, H, W), dtype=np.uint8)


def _prepare_input(u8_tchw):
    """DepthCrafter.prepare_input on the same images (the plugin's own code, no GPU involved)."""
    from unigeo_amd.model.depthcrafter import DepthCrafter
    return DepthCrafter.prepare_input(None, {"images": list(u8_tchw)})


# ---------------------------------------------------------------------------------------------- 5. raw words
@pytest.mark.parametrize("seed", [0, 7, 7 + (1 << 32), (0xDEADBEEF << 32) | 7, 2 ** 64 - 1])
@pytest.mark.parametrize("stream", [0, 1])
def test_philox_words_equal_the_restatement_bit_for_bit(engine, seed, stream):
    for q0, nb in ((0, 4096), ((1 << 32) - 1000, 3000), ((5 << 32) + 12345, 257), (2 ** 62 - 3, 1)):   # the second range carries into counter word 1
        got = engine.op_philox_u32(seed, stream, q0, nb)
        assert got.dtype == np.uint32 and got.shape == (nb, 4)
        assert np.array_equal(got, NO.philox_blocks(seed, stream, q0, nb)), (seed, stream, q0)


def test_philox_kernel_reproduces_the_known_answer_and_separates_seeds_and_streams(engine):
    assert [f"{v:08x}" for v in engine.op_philox_u32(0, 0, 0, 1)[0]] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    a = engine.op_philox_u32(7, 0, 0, 64)
    assert not np.array_equal(a, engine.op_philox_u32(7 + (1 << 32), 0, 0, 64))      # seeds that differ in the high word only
    assert not np.array_equal(a, engine.op_philox_u32(7, 1, 0, 64))


# ---------------------------------------------------------------------------------------------- 6. normals
def test_randn_within_twice_the_float32_floor_of_the_definition(engine, floor):
    """Reference: the definition in float64 on the same words.  Floor: the same definition in numpy float32, its own max-abs distance from
    float64 (2.0e-6 on 8 M pairs).  The device gets 2 x that floor - logf / sincos on the device are specified to a couple of ulp where
    numpy's are within one."""
    floor, ref = floor
    got = engine.op_randn(7, NO.STREAM_AUG, 0, ref.size)     # 16 M elements = the 8 M pairs of the floor
    assert got.dtype == np.float32 and np.isfinite(got).all()
    err = float(np.abs(got.astype(np.float64) - ref).max())
    report("device randn vs float64 definition", err, tol=2 * floor, kind="max|err|", floor_numpy_float32=floor)
    assert err <= 2 * floor, (err, floor)
    assert float(np.abs(got).max()) <= 5.768
    # the other stream, a high block offset: same bound, same reference construction
    e0 = ((1 << 32) - 8) * 4
    ref2 = NO.randn(2 ** 40 + 3, 1, e0, 4096)
    got2 = engine.op_randn(2 ** 40 + 3, 1, e0, 4096)
    assert float(np.abs(got2.astype(np.float64) - ref2).max()) <= 2 * floor


@pytest.mark.parametrize("e0,n", [(0, 1), (0, 2), (0, 3), (0, 1025), (0, 4098), (0, 263), (1, 4096), (3, 1021), (7, 6), (2, 1), (5, 3),
                                  (4, 4096), ((1 << 34) + 1, 777)])
def test_randn_tails_and_odd_offsets_write_exactly_n_values(engine, floor, e0, n):
    guard, fill = 64, -123.5
    buf = engine.op_randn(11, 1, e0, n, guard=guard, fill=fill)
    assert buf.shape == (n + guard,)
    assert (buf[n:] == np.float32(fill)).all(), "guard words after the buffer were written"
    got = buf[:n]
    assert np.isfinite(got).all() and not (got == np.float32(fill)).any() and float(np.abs(got).max()) <= 5.768
    ref = NO.randn(11, 1, e0, n)
    assert float(np.abs(got.astype(np.float64) - ref).max()) <= 2 * floor[0]
    # element e depends on (seed, stream, e) only: the same elements from an aligned launch that starts earlier
    base = engine.op_randn(11, 1, e0 - e0 % 4, n + 8)
    assert np.array_equal(got, base[e0 % 4: e0 % 4 + n])


# ---------------------------------------------------------------------------------------------- 7. full size, through the product entry points
def test_full_size_noise_statistics_via_set_inputs_and_get_noise(engine, floor):
    T, H, W = FULL
    seed = 7
    u8 = np.zeros((T, 3, H, W), np.uint8)
    engine.set_inputs_ex(u8, seed=seed)
    lat, aug = engine.get_noise()
    assert lat.shape == (T, 4, H // 8, W // 8) and aug.shape == (T, 3, H, W) and lat.dtype == aug.dtype == np.float32
    assert np.isfinite(lat).all() and np.isfinite(aug).all()
    assert max(float(np.abs(lat).max()), float(np.abs(aug).max())) <= 5.768
    for name, val, bound in NO.moment_checks(lat, aug):
        report(f"full-size device noise, seed {seed}: {name}", val, tol=bound, kind="abs")
        assert val < bound, (name, val, bound)
    # the same numbers as the op-level kernel and the definition (spot checks at both ends of both tensors)
    n_aug, n_lat = aug.size, lat.size
    for stream, flat, n in ((NO.STREAM_AUG, aug.reshape(-1), n_aug), (NO.STREAM_LATENTS, lat.reshape(-1), n_lat)):
        for e0 in (0, n - 4096):
            assert np.array_equal(flat[e0:e0 + 4096], engine.op_randn(seed, stream, e0, 4096))
            assert float(np.abs(flat[e0:e0 + 4096].astype(np.float64) - NO.randn(seed, stream, e0, 4096)).max()) <= 2 * floor[0]


# ---------------------------------------------------------------------------------------------- 8. uint8 frames
def test_u8_to_frames_equals_prepare_input_bit_for_bit(engine):
    T, H, W = 3, 40, 104                                     # H != W, not multiples of 64 (the op only needs H * W % 4 == 0)
    rng = np.random.default_rng(3)
    u8 = np.empty((T, 3, H, W), np.uint8)
    for t in range(T):
        for c in range(3):                                   # all 256 values in every channel of every frame, in a different order each
            plane = np.concatenate([np.arange(256), rng.integers(0, 256, H * W - 256)]).astype(np.uint8)
            u8[t, c] = rng.permutation(plane).reshape(H, W)
    assert all(np.unique(u8[:, c]).size == 256 for c in range(3))
    got = engine.op_u8_to_frames(u8)
    want = _prepare_input(u8)
    assert got.shape == want.shape == (T, H, W, 3) and got.dtype == want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and through the product entry point: every combination of frame format x noise source leaves the same resident inputs
    u8 = _u8_clip(2, 64, 128, 4)
    nl, na = NO.make_noise(2, 64, 128, 5, np.float32)
    engine.set_inputs_ex(u8, noise_latents=nl, noise_aug=na)
    gl, ga = engine.get_noise()
    assert np.array_equal(gl, nl) and np.array_equal(ga, na)
    engine.set_inputs(_prepare_input(u8), nl, na)
    gl, ga = engine.get_noise()
    assert np.array_equal(gl, nl) and np.array_equal(ga, na)
    with pytest.raises(RuntimeError):
        engine._ck(engine.lib.ug_dc_set_inputs_ex(engine.ctx, u8.ctypes.data, 1, 2, 64, 128, nl.ctypes.data, None, 0, None))   # one noise array only
    with pytest.raises(RuntimeError):
        engine._ck(engine.lib.ug_dc_set_inputs_ex(engine.ctx, u8.ctypes.data, 1, 2, 64, 96, None, None, 0, None))              # same checks as ug_dc_set_inputs


# ---------------------------------------------------------------------------------------------- 9. equivalence, no tolerance
def _device_then_host(pipe, u8, seed, **kw):
    """Device mode (uint8 frames, seed) -> download the noise -> the default path with those arrays and prepare_input's float frames."""
    dev = pipe(u8, noise="device", seed=seed, with_normals=True, **kw)
    nl, na = pipe.engine.get_noise()
    host = pipe(_prepare_input(u8), noise_latents=nl, noise_aug=na, with_normals=True, **kw)
    return dev, host, (nl, na)


def _same(a, b):
    for x, y, what in ((a.depth, b.depth, "depth"), (a.frames[0], b.frames[0], "frames"), (a.normals, b.normals, "normals")):
        assert x is not None and np.isfinite(x).all(), what
        assert np.array_equal(x, y), f"{what}: device-mode run differs from the host-noise run on the same noise"


CASES = {
    "plain": dict(T=3, kw=dict(num_inference_steps=2, window_size=3)),
    "windowed": dict(T=11, kw=dict(num_inference_steps=2, window_size=6, overlap=2)),         # T > window_size: windows at 0 and 4 (6 frames), ragged tail of 3 frames at 8
    "guided": dict(T=3, kw=dict(num_inference_steps=2, window_size=3, guidance_scale=1.2)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_device_mode_equals_the_host_path_on_the_same_noise(tiny, floor, case):
    T, kw = CASES[case]["T"], CASES[case]["kw"]
    u8 = _u8_clip(T, 64, 128, 21)
    K = np.tile(np.array([[100.0, 0, 64], [0, 100.0, 32], [0, 0, 1]], np.float32), (T, 1, 1))
    dev, host, (nl, na) = _device_then_host(tiny, u8, 2 ** 40 + 3, intrinsics=K, **kw)
    _same(dev, host)
    assert float(np.ptp(dev.depth)) > 0
    # the resident noise is the definition's
    rl, ra = NO.make_noise(T, 64, 128, 2 ** 40 + 3)
    assert float(np.abs(nl - rl).max()) <= 2 * floor[0] and float(np.abs(na - ra).max()) <= 2 * floor[0]


# ---------------------------------------------------------------------------------------------- 10. determinism, contexts, seeds, plugin
def test_same_seed_twice_and_two_seeds(tiny):
    u8 = _u8_clip(3, 64, 64, 22)
    a = tiny(u8, noise="device", seed=5, num_inference_steps=2, window_size=3, with_normals=False)
    na = tiny.engine.get_noise()
    other = tiny(u8, noise="device", seed=6, num_inference_steps=2, window_size=3)
    nb = tiny.engine.get_noise()
    b = tiny(u8, noise="device", seed=5, num_inference_steps=2, window_size=3)
    nc = tiny.engine.get_noise()
    assert np.array_equal(a.depth, b.depth) and np.array_equal(a.frames[0], b.frames[0])
    assert np.array_equal(na[0], nc[0]) and np.array_equal(na[1], nc[1])
    assert not np.array_equal(na[0], nb[0]) and not np.array_equal(na[1], nb[1])
    assert abs(float(np.corrcoef(na[1].reshape(-1), nb[1].reshape(-1))[0, 1])) < 5 / np.sqrt(na[1].size)
    assert not np.array_equal(a.depth, other.depth)


def test_second_context_running_concurrently_gives_the_solo_result(tiny):
    from unigeo_amd.pipeline import DepthCrafterPipelineHIP
    from unigeo_amd import weights as W
    second = DepthCrafterPipelineHIP.from_random(seed=42, cfgs=W.tiny_cfgs(), workspace_bytes=3 << 30)
    try:
        clips = {0: (_u8_clip(3, 64, 128, 30), 100), 1: (_u8_clip(3, 64, 128, 31), 2 ** 63 + 9)}
        K = np.tile(np.array([[100.0, 0, 64], [0, 100.0, 32], [0, 0, 1]], np.float32), (3, 1, 1))
        kw = dict(noise="device", num_inference_steps=2, window_size=3, with_normals=True, intrinsics=K)
        solo = {i: tiny(u8, seed=s, **kw) for i, (u8, s) in clips.items()}
        solo_noise_1 = tiny.engine.get_noise()                        # of clip 1, the last solo run
        out, errs = {}, []
        start = threading.Barrier(2)

        def work(i, pipe):
            try:
                start.wait(timeout=60)
                for _ in range(3):                                   # a few clips each, so that the two contexts overlap on the GPU
                    out[i] = pipe(clips[i][0], seed=clips[i][1], **kw)
            except Exception as e:   # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=work, args=(0, tiny)), threading.Thread(target=work, args=(1, second))]
        [t.start() for t in th]
        [t.join(timeout=300) for t in th]
        assert not errs, errs
        assert not any(t.is_alive() for t in th)
        for i in (0, 1):
            _same(out[i], solo[i])
        n2 = second.engine.get_noise()
        assert np.array_equal(n2[0], solo_noise_1[0]) and np.array_equal(n2[1], solo_noise_1[1])     # not context-dependent
    finally:
        second.engine.close()


def test_plugin_device_mode_equals_the_pipeline_call_and_returns_the_reference_types():
    import torch
    from unigeo_amd.model.depthcrafter import DepthCrafter
    from unigeo_amd.synthetic import synthetic_clip
    before = threading.active_count()
    model = DepthCrafter(synthetic_weights=True, tiny=True, noise="device", num_inference_steps=2, seed=40, workspace_bytes=3 << 30)
    try:
        T, H, W = 3, 64, 128
        data = synthetic_clip(T, H, W, seed=3)
        data["_index"] = 2
        out = model.forward(data)
        assert threading.active_count() == before and getattr(model, "_noise_pf", None) is None
        assert set(out) == {"pred_depths", "pred_normals"}
        d, n = out["pred_depths"], out["pred_normals"]
        assert isinstance(d, torch.Tensor) and d.dtype == torch.float32 and tuple(d.shape) == (T, H, W) and d.device.type == "cpu"
        assert isinstance(n, torch.Tensor) and n.dtype == torch.float32 and tuple(n.shape) == (T, H, W, 3) and n.device.type == "cpu"
        assert torch.isfinite(d).all() and torch.isfinite(n).all()
        # the pipeline call of the equivalence test: device mode, then the default path on the downloaded noise and prepare_input's frames
        u8 = np.stack([np.asarray(x).astype(np.uint8) for x in data["images"]], 0)
        K = np.stack([np.asarray(k, dtype=np.float32).reshape(3, 3) for k in data["intrinsics"]], 0)
        kw = dict(num_inference_steps=2, window_size=T, intrinsics=K)
        dev, host, _ = _device_then_host(model.pipeline, u8, 42, **kw)
        _same(dev, host)
        assert np.array_equal(d.numpy(), host.depth) and np.array_equal(n.numpy(), host.normals)
        assert np.array_equal(model.prepare_input(data), _prepare_input(u8))
    finally:
        model.pipeline.engine.close()
