"""GPU: ``ug_prep_render_mesh`` (kernels/render.hip) byte for byte against the host mirror ``render_mesh`` on the
meshes of tests/render_fixtures.py; a clip longer than one chunk; its error paths; tools/render_scannetpp.py --device against the host run."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
from PIL import Image

import render_fixtures as rf
from unigeo_amd._lib import RenderOptsC
from unigeo_amd.harness.render import render_mesh, world2cam_from

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_VGA = (400.0, 410.0, 323.0, 241.0)

CASES = {
    "box3": lambda: (*rf.box(), rf.box_poses()[:3], rf.K_BOX, rf.H, rf.W),                       # T = 3 distinct poses: a frame index that goes wrong shows
    "floor": lambda: (*rf.floor(), rf.identity_pose(), rf.K_BOX, rf.H, rf.W),                    # straddles the camera plane: the whole-frame box
    "diag": lambda: (*rf.diag_quad(), rf.identity_pose(), rf.K_DIAG, rf.H, rf.W),                # edge values of exactly 0
    "dup": lambda: (*rf.duplicates(), rf.identity_pose(), rf.K_BOX, rf.H, rf.W),                 # equal depths: the index decides
    "grid": lambda: (*rf.bumpy_grid(), rf.identity_pose(), rf.GRID_K, *rf.GRID_HW),              # boxes from one pixel to the frame: both walks
    "box_37x53": lambda: (*rf.box(), rf.box_poses()[3:5], (30.0, 29.0, 26.4, 18.7), 37, 53),
    "box_1x1": lambda: (*rf.box(), rf.box_poses()[:2], (1.0, 1.0, 0.5, 0.5), 1, 1),
    "empty": lambda: (*rf.plane(z=-2.0), rf.identity_pose(), rf.K_BOX, rf.H, rf.W),
}


def _same(got, ref):
    for g, r, what in zip(got, ref, ("depth_mm", "normal", "tri_index")):
        assert g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes(), (what, int((g != r).sum()))


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_mirror(engine, name):
    args = CASES[name]()
    got = engine.prep_render_mesh(*args)
    _same(got, rf.mirror(name))
    _same(engine.prep_render_mesh(*args), got)                            # two runs, equal bytes
    if name == "grid":                                                    # the case has boxes on both sides of the kernel's threshold
        idx = rf.mirror(name)[2]
        counts = np.bincount(idx[idx >= 0], minlength=2000)
        assert (counts[counts > 0] <= 4).sum() > 100 and counts.max() > 1000
    if name == "empty":
        assert not got[0].any() and not got[1].any() and (got[2] == -1).all()


def test_mask_and_null_outputs(engine):
    mesh, poses = rf.box(), rf.box_poses()[:3]
    mask = np.full((3, rf.H, rf.W), 255, np.uint8)
    mask[1, :9, :] = 0
    mask[2, 5, 5] = 254
    _same(engine.prep_render_mesh(*mesh, poses, rf.K_BOX, rf.H, rf.W, masks=mask), render_mesh(*mesh, poses, rf.K_BOX, rf.H, rf.W, masks=mask))
    ref = rf.mirror("box3")
    depth, normal, index = engine.prep_render_mesh(*mesh, poses, rf.K_BOX, rf.H, rf.W, with_index=False)      # tri_index = NULL, mask = NULL
    assert index is None and np.array_equal(depth, ref[0]) and np.array_equal(normal, ref[1])
    near = engine.prep_render_mesh(*mesh, poses, rf.K_BOX, rf.H, rf.W, znear=1.0, zfar=2.0)
    _same(near, render_mesh(*mesh, poses, rf.K_BOX, rf.H, rf.W, znear=1.0, zfar=2.0))
    assert (near[2] == -1).any() and (near[2] >= 0).any()


def test_a_clip_longer_than_one_chunk(engine):
    """480 x 640 takes 18 bytes per pixel on the device, 18 frames per 96 MB chunk: 21 frames in alternating poses need a second chunk, which
    must start at the right camera and write to the right place."""
    ref = rf.mirror("box_vga")
    assert not np.array_equal(ref[0][0], ref[0][1])
    order = np.arange(21) % 2
    got = engine.prep_render_mesh(*rf.box(), rf.box_poses()[:2][order], K_VGA, 480, 640)
    _same(got, tuple(r[order] for r in ref))


def _call(engine, verts, NV, faces, NF, w2c, K, T, H, W, mask, opts, depth, normal, index):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return engine.lib.ug_prep_render_mesh(engine.ctx, p(verts), NV, p(faces), NF, p(w2c), p(K), T, H, W, p(mask),
                                          None if opts is None else C.byref(opts), p(depth), p(normal), p(index))


def _opts(engine, **kw):
    o = RenderOptsC()
    engine.lib.ug_render_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_errors_name_the_problem_and_leave_the_context_usable(engine):
    v, f = rf.box()
    v, f = np.ascontiguousarray(v), np.ascontiguousarray(f)
    m = world2cam_from(rf.box_poses()[:1])
    k = np.array([rf.K_BOX], np.float64)
    H, W = rf.H, rf.W
    ref = tuple(r[:1] for r in rf.mirror("box3"))
    depth, normal, index = np.zeros((1, H, W), np.uint16), np.zeros((1, H, W, 3), np.uint8), np.zeros((1, H, W), np.int32)
    nan, inf = float("nan"), float("inf")

    def edited(a, i, val):
        b = a.copy()
        b.reshape(-1)[i] = val
        return b

    good = dict(verts=v, NV=8, faces=f, NF=12, w2c=m, K=k, T=1, H=H, W=W, mask=None, opts=None, depth=depth, normal=normal, index=index)
    cases = [(dict(verts=None), "NULL"), (dict(faces=None), "NULL"), (dict(w2c=None), "NULL"), (dict(K=None), "NULL"), (dict(depth=None), "NULL"),
             (dict(normal=None), "NULL"),
             (dict(NV=0), "positive"), (dict(NF=0), "positive"), (dict(T=0), "positive"), (dict(H=-4), "positive"), (dict(W=0), "positive"),
             (dict(NF=1 << 31), "2^31"), (dict(T=1 << 15, H=1 << 8, W=1 << 8), "2^31"),              # rejected before anything is read
             (dict(faces=edited(f, 7, 8)), "face index"), (dict(faces=edited(f, 0, -1)), "face index"), (dict(NV=7), "face index"),
             (dict(w2c=edited(m, 5, nan)), "world2cam"), (dict(K=edited(k, 2, inf)), "K"), (dict(verts=edited(v, 4, nan)), "vertex"),
             (dict(K=edited(k, 0, 0.0)), "fx"), (dict(K=edited(k, 1, -41.0)), "fy"),
             (dict(opts=_opts(engine, znear=0.0)), "znear"), (dict(opts=_opts(engine, znear=nan)), "znear"),
             (dict(opts=_opts(engine, zfar=0.05)), "zfar"), (dict(opts=_opts(engine, zfar=0.01)), "zfar"),
             (dict(opts=_opts(engine, zfar=65.536)), "65.535"), (dict(opts=_opts(engine, zfar=inf)), "zfar"),
             (dict(opts=_opts(engine, flags=1)), "0x1"), (dict(opts=_opts(engine, flags=0x12)), "0x12")]
    for change, word in cases:
        assert _call(engine, **{**good, **change}) != 0, word
        err = engine.lib.ug_last_error(engine.ctx).decode()
        assert word in err, (word, err)
        assert not depth.any() and not normal.any() and not index.any()   # nothing written
        assert _call(engine, **good) == 0                                 # the context is usable: a valid call succeeds
        _same((depth, normal, index), ref)
        depth[:] = 0; normal[:] = 0; index[:] = 0
    assert _call(engine, **{**good, "opts": _opts(engine, zfar=65.535)}) == 0
    with pytest.raises(ValueError):
        engine.prep_render_mesh(v, f, rf.box_poses()[:1], rf.K_BOX, H, W, masks=np.zeros((1, H, W), np.float32))
    with pytest.raises(ValueError):
        engine.prep_render_mesh(v, f + 1, rf.box_poses()[:1], rf.K_BOX, H, W)


def test_profile_names_the_renderer(engine):
    engine.profile_begin()
    engine.prep_render_mesh(*rf.box(), rf.box_poses()[:3], rf.K_BOX, rf.H, rf.W)
    prof = engine.profile_end()
    assert prof["render_mesh"]["calls"] == 1 and prof["render_mesh"]["ms"] > 0


def test_tool_on_the_device_equals_the_host_run(engine, tmp_path):
    spec = importlib.util.spec_from_file_location("render_scannetpp", os.path.join(ROOT, "tools", "render_scannetpp.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    raw, host, dev = str(tmp_path / "raw"), str(tmp_path / "host"), str(tmp_path / "dev")
    names = rf.write_raw_scene(raw)
    common = ["--scenes", rf.SCENE, "--target-resolution", "64", "--frames-per-call", "4", "--lossless"]
    assert tool.main([raw, host, *common]) == 6
    assert tool.main([raw, dev, *common, "--device"], engine=engine) == 6
    for n in names:
        for sub, ext in (("depth", ".png"), ("normal", ".webp"), ("images", ".webp")):
            a = np.array(Image.open(os.path.join(host, rf.SCENE, sub, n + ext)))
            b = np.array(Image.open(os.path.join(dev, rf.SCENE, sub, n + ext)))
            assert np.array_equal(a, b), (sub, n)
    with np.load(os.path.join(host, rf.SCENE, "scene_metadata.npz")) as a, np.load(os.path.join(dev, rf.SCENE, "scene_metadata.npz")) as b:
        for key in ("trajectories", "intrinsics", "images"):
            assert np.array_equal(a[key], b[key])
