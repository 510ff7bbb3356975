"""GPU: ``ug_prep_register_depth`` (kernels/register.hip) against the reference's files in
tests/golden/register_golden.npz and, bit for bit, against the host mirror ``register_depth`` on the inputs of tests/test_register_depth_cpu.py;
its error paths; ``sevenScenesDataset(register="device")`` against ``register="host"``."""
import ctypes as C

import numpy as np
import pytest

import register_fixtures as rf
from unigeo_amd._lib import REG_DROP_SENTINEL, RegisterOptsC
from unigeo_amd.harness import rgbd
from unigeo_amd.harness.rgbd import register_depth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return rf.golden()


@pytest.fixture(scope="module")
def scene(tmp_path_factory, gold):
    return rf.write_scene(str(tmp_path_factory.mktemp("reg7")), *gold)


def test_device_equals_the_reference_files(engine, gold):
    raw, expected = gold
    got = engine.prep_register_depth(raw)
    assert got.dtype == np.uint16 and got.shape == (2, 480, 640)
    assert np.array_equal(got, expected)
    assert np.array_equal(engine.prep_register_depth(raw[1]), expected[1])           # [H,W] in, [H,W] out
    assert engine.prep_register_depth(raw).tobytes() == got.tobytes()                # two runs, equal bytes


@pytest.mark.parametrize("invalid", ["keep", "drop"])
def test_device_equals_host_on_three_distinct_frames(engine, gold, invalid):
    raw, _ = gold
    clip = np.stack([raw[1], raw[0], np.roll(raw[1], 37, axis=1)])                   # T = 3: a frame index that goes wrong shows
    host = register_depth(clip, invalid)
    assert not np.array_equal(host[0], host[2]) and not np.array_equal(host[0], host[1])
    dev = engine.prep_register_depth(clip, invalid=invalid)
    assert np.array_equal(dev, host)
    assert engine.prep_register_depth(clip, invalid=invalid).tobytes() == dev.tobytes()


def test_device_equals_host_on_grid_tails_and_hand_built_cases(engine):
    raw = rf.all_values_frame()                                                      # 37 x 53
    for opts in (rf.identity_opts(585.0), rf.identity_opts(585.0, half_pixel=False), rf.identity_opts(60.0, dst_focal=33.0), None):
        for invalid in ("keep", "drop"):
            assert np.array_equal(engine.prep_register_depth(raw, opts, invalid), register_depth(raw, invalid, opts)), (opts, invalid)
    out = engine.prep_register_depth(raw, rf.identity_opts(585.0))
    assert np.array_equal(out[raw > 0], rf.millimetre_round_trip(raw)[raw > 0])
    for one in (1234, 0, 65535):                                                     # 1 x 1
        px = np.array([[one]], np.uint16)
        for invalid in ("keep", "drop"):
            assert np.array_equal(engine.prep_register_depth(px, rf.identity_opts(585.0), invalid), register_depth(px, invalid, rf.identity_opts(585.0)))
    assert engine.prep_register_depth(np.array([[1234]], np.uint16), rf.identity_opts(585.0))[0, 0] == 1234
    raw, opts, expected = rf.tie_case()
    assert np.array_equal(engine.prep_register_depth(raw, opts), expected)
    raw, opts = rf.collision_case()
    assert np.array_equal(engine.prep_register_depth(raw, opts), register_depth(raw, opts=opts))
    zero = np.zeros((2, 480, 640), np.uint16)
    assert not engine.prep_register_depth(zero).any()


def test_a_clip_longer_than_one_chunk(engine, gold):
    """41 frames of 480 x 640 take more than the 96 MB one chunk may: the second chunk starts at the right frame and writes to the right place."""
    raw, expected = gold
    order = np.arange(41) % 2
    got = engine.prep_register_depth(raw[order])
    assert np.array_equal(got, expected[order])


def _call(engine, depth, T, H, W, opts, out):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return engine.lib.ug_prep_register_depth(engine.ctx, p(depth), T, H, W, None if opts is None else C.byref(opts), p(out))


def _opts(engine, **kw):
    o = RegisterOptsC()
    engine.lib.ug_register_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_errors_name_the_problem_and_leave_the_context_usable(engine, gold):
    raw, expected = gold
    d = np.ascontiguousarray(raw[:1])
    out = np.zeros_like(d)
    nan, inf = float("nan"), float("inf")
    bad_m = _opts(engine)
    bad_m.src2dst[5] = nan
    cases = [((None, 1, 480, 640, None, out), "NULL"), ((d, 1, 480, 640, None, None), "NULL"),
             ((d, 0, 480, 640, None, out), "positive"), ((d, 1, -480, 640, None, out), "positive"), ((d, 1, 480, 0, None, out), "positive"),
             ((d, 1 << 15, 1 << 8, 1 << 8, None, out), "2^31"),                      # rejected before anything is read
             ((d, 1, 480, 640, _opts(engine, flags=2), out), "0x2"), ((d, 1, 480, 640, _opts(engine, flags=REG_DROP_SENTINEL | 8), out), "0x8"),
             ((d, 1, 480, 640, _opts(engine, src_focal=0.0), out), "src_focal"), ((d, 1, 480, 640, _opts(engine, dst_focal=nan), out), "dst_focal"),
             ((d, 1, 480, 640, _opts(engine, src_focal=inf), out), "src_focal"), ((d, 1, 480, 640, _opts(engine, dst_focal=-525.0), out), "dst_focal"),
             ((d, 1, 480, 640, _opts(engine, divisor=0.0), out), "divisor"), ((d, 1, 480, 640, _opts(engine, divisor=nan), out), "divisor"),
             ((d, 1, 480, 640, _opts(engine, max_valid=-1.0), out), "max_valid"), ((d, 1, 480, 640, _opts(engine, max_valid=inf), out), "max_valid"),
             ((d, 1, 480, 640, bad_m, out), "src2dst")]
    for args, word in cases:
        assert _call(engine, *args) != 0, word
        assert word in engine.lib.ug_last_error(engine.ctx).decode(), (word, engine.lib.ug_last_error(engine.ctx).decode())
        assert not out.any()
        assert _call(engine, d, 1, 480, 640, None, out) == 0                         # the context is usable: a valid call succeeds
        assert np.array_equal(out, expected[:1])
        out[:] = 0
    assert _call(engine, d, 1, 480, 640, _opts(engine, flags=REG_DROP_SENTINEL), out) == 0
    assert np.array_equal(out, register_depth(d, "drop"))
    with pytest.raises(ValueError):
        engine.prep_register_depth(raw.astype(np.int32))
    with pytest.raises(ValueError):
        engine.prep_register_depth(raw, invalid="clear")


@pytest.mark.parametrize("prep", ["device", "host"])
def test_loader_register_device_equals_register_host(engine, scene, prep):
    kw = dict(scenes=[rf.SCENE], clip_length=2, clip_overlap=0, input_size=(48, 64), target_size=(48, 64), prep=prep, engine=engine)
    host = rgbd.sevenScenesDataset(scene, register="host", **kw)
    dev = rgbd.sevenScenesDataset(scene, register="device", **kw)
    assert len(host) == len(dev) == 1
    rf.assert_same_sample(host[0], dev[0])
    assert dev.last_timing["register"] > 0 and host.last_timing["register"] > 0
    drop_h = rgbd.sevenScenesDataset(scene, register="host", register_invalid="drop", **kw)[0]
    drop_d = rgbd.sevenScenesDataset(scene, register="device", register_invalid="drop", **kw)[0]
    rf.assert_same_sample(drop_h, drop_d)
    assert np.stack(drop_d["mask"]).sum() < np.stack(dev[0]["mask"]).sum()
