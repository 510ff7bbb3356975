"""CPU: the 7-Scenes depth registration on the host (``register_depth`` of unigeo_amd/harness/rgbd.py) against
tests/golden/register_golden.npz - the ``*.depth.proj.png`` files the reference's own ``process_scene`` wrote for two synthetic raw frames
(tests/golden/make_register_golden.py) -, the UNPINNED ``invalid="drop"`` mode by its properties, hand-built tie / collision / identity cases
against a scalar restatement, ``sevenScenesDataset(register="host")`` against the default loader on a scene that holds both kinds of file,
and the new entry points in the library and its product header.  The same inputs go to the device in tests/test_register_depth_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import register_fixtures as rf
from unigeo_amd.harness import parse_dataset_config, rgbd
from unigeo_amd.harness.rgbd import RegisterOpts, register_depth

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gold():
    return rf.golden()


@pytest.fixture(scope="module")
def scene(tmp_path_factory, gold):
    return rf.write_scene(str(tmp_path_factory.mktemp("reg7")), *gold)


def _ds(root, **kw):
    return rgbd.sevenScenesDataset(root, scenes=[rf.SCENE], clip_length=2, clip_overlap=0, **kw)


def test_host_mirror_equals_the_reference_files(gold):
    raw, expected = gold
    assert raw.dtype == expected.dtype == np.uint16 and raw.shape == expected.shape == (2, 480, 640)
    got = register_depth(raw)
    assert got.dtype == np.uint16 and got.shape == raw.shape
    assert np.array_equal(got, expected)
    assert np.array_equal(register_depth(raw[1]), expected[1])                       # [H,W] in, [H,W] out
    assert not np.array_equal(expected[0], expected[1])


def test_the_golden_holds_wrapped_pixels(gold):
    """Pixels whose fl32(1000 * z) is 65536 or more and comes out modulo 65536: the branch cannot go untested."""
    raw, expected = gold
    for k in range(2):
        z = rgbd._register_zbuf(raw[k], False, RegisterOpts())
        v = (np.float32(1000.0) * z).astype(np.int64)
        wrapped = (z <= 1000) & (v >= 65536)
        assert wrapped.sum() > 1000
        assert np.array_equal(expected[k][wrapped].astype(np.int64) + 65536, v[wrapped])
        assert expected[k][wrapped].max() < 1000                                    # 65.5 .. 66.5 m read as less than a metre


def test_drop_takes_no_pixel_from_a_sentinel(gold):
    raw, expected = gold
    drop = register_depth(raw, "drop")
    cleared = raw.copy()
    cleared[raw == 65535] = 0
    assert np.array_equal(drop, register_depth(cleared))                            # as if the marker were a missing pixel
    assert np.array_equal(drop, register_depth(cleared, "drop"))
    for k in range(2):                                                              # equal to "keep" wherever no sentinel splat won
        z_keep = rgbd._register_zbuf(raw[k], False, RegisterOpts())
        z_real = rgbd._register_zbuf(raw[k], True, RegisterOpts())
        sentinel_won = z_keep != z_real
        assert sentinel_won.sum() > 1000 and (z_real[sentinel_won] == 2000).all()   # it only ever fills holes: 65 m loses to any surface
        assert np.array_equal(drop[k][~sentinel_won], expected[k][~sentinel_won])
        assert (drop[k][sentinel_won] == 0).all()
    with pytest.raises(ValueError, match="invalid"):
        register_depth(raw, "clear")


def test_identity_returns_the_input():
    """No motion, equal focals, the half pixel taken back: every valid pixel stays where it is and comes out as trunc(fl32(1000 * fl32(raw /
    1000))) - raw itself except where that product rounds below the integer."""
    raw = rf.all_values_frame()
    out = register_depth(raw, opts=rf.identity_opts(585.0))
    valid = raw > 0
    trip = rf.millimetre_round_trip(raw)
    exact = valid & (trip == raw)
    assert exact.sum() > 0.95 * valid.sum()
    assert np.array_equal(out[exact], raw[exact])
    assert np.array_equal(out[valid], trip[valid]) and (out[~valid] == 0).all()
    assert np.array_equal(out, rf.loop_reference(raw, rf.identity_opts(585.0)))
    allv = np.arange(1, 65535, dtype=np.uint16)
    assert (rf.millimetre_round_trip(allv) != allv).sum() == 739 and (allv - rf.millimetre_round_trip(allv)).max() == 1


def test_a_projection_on_one_half_rounds_to_even():
    raw, opts, expected = rf.tie_case()
    assert np.array_equal(register_depth(raw, opts=opts), expected)
    assert np.array_equal(rf.loop_reference(raw, opts), expected)


def test_sixteen_sources_per_target_the_nearest_wins():
    raw, opts = rf.collision_case()
    out = register_depth(raw, opts=opts)
    assert np.array_equal(out, rf.loop_reference(raw, opts))
    assert 30 <= (out > 0).sum() <= 80                                              # 768 sources on about 6 x 8 targets
    assert out[out > 0].min() == rf.millimetre_round_trip(raw[raw > 0]).min()       # the nearest of all survives
    assert np.array_equal(register_depth(np.zeros((5, 7), np.uint16)), np.zeros((5, 7), np.uint16))


def test_python_defaults_are_the_library_defaults():
    from unigeo_amd import _lib
    o = _lib.RegisterOptsC()
    _lib.load_library().ug_register_opts_default(C.byref(o))
    d = RegisterOpts()
    assert (o.src_focal, o.dst_focal, o.divisor, o.max_valid, o.flags) == (d.src_focal, d.dst_focal, d.divisor, d.max_valid, 0)
    assert tuple(o.src2dst) == tuple(d.src2dst) and len(d.src2dst) == 12
    assert (d.src_focal, d.dst_focal) == (585.0, 525.0)


def test_new_symbols_are_exported_and_declared():
    from unigeo_amd import _lib
    lib = _lib.load_library()
    txt = open(os.path.join(os.path.dirname(G), "..", "include", "unigeo_hip.h")).read()
    for s in ("ug_register_opts_default", "ug_prep_register_depth"):
        assert s in _lib.EXPORTS and hasattr(lib, s) and f" {s}(" in txt
    assert "UG_REG_DROP_SENTINEL 1" in txt and _lib.REG_DROP_SENTINEL == 1


@pytest.mark.parametrize("size", [None, (48, 64)])
def test_loader_register_host_equals_the_default_loader(scene, size):
    kw = {} if size is None else dict(input_size=size, target_size=size)
    default, reg = _ds(scene, **kw), _ds(scene, register="host", **kw)
    assert default.samples[0][0].depth_paths == [f"frame-{t:06d}.depth.proj.png" for t in range(2)]
    assert reg.samples[0][0].depth_paths == [f"frame-{t:06d}.depth.png" for t in range(2)]
    assert len(default) == len(reg) == 1
    a, b = default[0], reg[0]
    rf.assert_same_sample(a, b)
    assert np.stack(b["mask"]).shape[-2:] == (size or (480, 640)) and 0.5 < np.stack(b["mask"]).mean() < 0.9
    assert reg.last_timing["register"] > 0 and default.last_timing is None
    assert rgbd.sevenScenesDataset.layout.depth_pattern == "*.depth.proj.png"      # the class keeps the default layout


def test_loader_register_drop_differs_only_in_the_mask_it_loses(scene):
    keep, drop = _ds(scene, register="host")[0], _ds(scene, register="host", register_invalid="drop")[0]
    mk, md = np.stack(keep["mask"]), np.stack(drop["mask"])
    assert (md <= mk).all() and md.sum() < mk.sum()


def test_loader_errors(scene, tmp_path, gold):
    with pytest.raises(ValueError, match="register"):
        _ds(scene, register="gpu")
    with pytest.raises(ValueError, match="register_invalid"):
        _ds(scene, register="host", register_invalid="clear")
    small = rf.write_scene(str(tmp_path / "small"), *gold, size=(24, 32))
    assert _ds(small)[0]["images"][0].shape == (3, 24, 32)                          # the default loader takes any size
    with pytest.raises(ValueError, match="480 x 640"):
        _ds(small, register="host")[0]
    scenes = os.path.join(G, "rgbd_scenes")
    for L, sc in (("bonn", "rgbd_bonn_balloon2"), ("neuralrgbd", "breakfast_room"), ("replica", "room_0"), ("scannetv2", "scene0707_00")):
        with pytest.raises(ValueError, match="register"):
            rgbd.LAYOUTS[L](os.path.join(scenes, L), scenes=[sc], register="host")
        rgbd.LAYOUTS[L](os.path.join(scenes, L), scenes=[sc], register=None)


def test_batch_tool_writes_the_reference_files(tmp_path, gold, capsys):
    import importlib.util
    from PIL import Image
    spec = importlib.util.spec_from_file_location("register_7scenes", os.path.join(os.path.dirname(G), "..", "tools", "register_7scenes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    raw, expected = gold
    root = rf.write_scene(str(tmp_path / "s"), raw, np.zeros_like(expected))        # stale outputs in place
    proj = [os.path.join(root, rf.SCENE, f"frame-{t:06d}.depth.proj.png") for t in range(2)]
    assert tool.main([root, "--scenes", rf.SCENE]) == 0 and not np.array(Image.open(proj[0])).any()       # kept without --overwrite
    os.remove(proj[1])
    assert tool.main([root, "--scenes", rf.SCENE, "--batch", "1"]) == 1
    assert np.array_equal(np.array(Image.open(proj[1])), expected[1]) and not np.array(Image.open(proj[0])).any()
    split = tmp_path / "split.txt"
    split.write_text(rf.SCENE + "\n")
    assert tool.main([root, "--split-file", str(split), "--overwrite"]) == 2
    for t in range(2):
        got = np.array(Image.open(proj[t]))
        assert got.dtype == np.uint16 and np.array_equal(got, expected[t])
    rf.assert_same_sample(_ds(root)[0], _ds(root, register="host")[0])             # the loader reads them as it reads the reference's
    with pytest.raises(SystemExit):
        tool.main([root])


def test_config_keys_reach_the_dataset():
    cfg = {"root": "r", "h": 48, "w": 64}
    assert "register" not in parse_dataset_config(cfg) and "register_invalid" not in parse_dataset_config(cfg)
    out = parse_dataset_config(dict(cfg, register="device", register_invalid="drop"))
    assert out["register"] == "device" and out["register_invalid"] == "drop"


def test_default_loader_on_the_existing_fixture_is_unchanged():
    """Without ``register`` the 7-Scenes loader globs, reads and returns what it did: the samples of tests/golden/rgbd_golden.npz."""
    with np.load(os.path.join(G, "rgbd_golden.npz")) as f:
        g = {k: f[k] for k in f.files if k.startswith("7scenes_")}
    ds = rgbd.sevenScenesDataset(os.path.join(G, "rgbd_scenes", "7scenes"), scenes=["chess/seq-03"], clip_length=3, clip_overlap=0)
    assert ds.register is None and list(ds.samples[0][0].depth_paths) == g["7scenes_depth"].tolist()
    assert len(ds) == 2
    for ci in range(2):
        s = ds[ci]
        assert list(s.keys()) == g[f"7scenes_c{ci}_keys"].tolist() + ["_index", "_dataset"]
        assert s["image_names"] == g[f"7scenes_c{ci}_names"].tolist()
        for k in ("images", "extrinsics", "intrinsics", "cam_coord", "world_coord", "mask"):
            a = np.stack(s[k])
            assert a.dtype == g[f"7scenes_c{ci}_{k}"].dtype and a.tobytes() == g[f"7scenes_c{ci}_{k}"].tobytes(), k
