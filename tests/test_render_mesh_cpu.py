"""CPU: the ScanNet++ mesh renderer on the host (``render_mesh`` of unigeo_amd/harness/render.py) on hand-built
meshes whose image is known without a renderer; the PLY reader; the output size and intrinsics of the rescale against the reference's own
function (tests/golden/render_golden.npz); tools/render_scannetpp.py end to end on a tiny raw scene; the new entry points in the library
and its product header.  The same meshes go to the device in tests/test_render_mesh_gpu.py."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
from PIL import Image

import render_fixtures as rf
from unigeo_amd.harness.ply import read_ply_mesh, write_ply_mesh
from unigeo_amd.harness.render import render_mesh, rescaled_size_and_intrinsics
from unigeo_amd.harness.scannetpp import ScannetPPDataset
from unigeo_amd.harness.vis import write_ply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = rf.H, rf.W


def tool():
    spec = importlib.util.spec_from_file_location("render_scannetpp", os.path.join(ROOT, "tools", "render_scannetpp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fronto_parallel_plane():
    """z = 2 everywhere.  The normal facing the camera is (0, 0, 1) in the OpenGL camera frame the script rotates into: 255 in z.  Its zero
    components pass the first quantisation as q = 128, decode to m = +1/255 and re-encode by truncation as trunc(128.0) = 128 where the
    rotation keeps their sign and as trunc(127.0) = 127 where it flips it - the script's own asymmetry.  In a world frame that is the
    OpenGL camera frame both keep their sign: (128, 128, 255); with OpenCV world axes the y component is flipped: (128, 127, 255)."""
    depth, normal, index = render_mesh(*rf.plane(-2.0), rf.gl_world_pose(), rf.K_BOX, H, W)
    assert depth.shape == (1, H, W) and depth.dtype == np.uint16 and normal.shape == (1, H, W, 3) and normal.dtype == np.uint8
    assert index.dtype == np.int32 and (index >= 0).all()
    assert (depth == 2000).all()
    assert (normal == np.uint8([128, 128, 255])).all()
    depth, normal, _ = render_mesh(*rf.plane(2.0), rf.identity_pose(), rf.K_BOX, H, W)
    assert (depth == 2000).all()
    assert (normal == np.uint8([128, 127, 255])).all()


def test_quad_whose_diagonal_passes_through_pixel_centres():
    depth, _, index = rf.mirror("diag")
    assert (index >= 0).all() and (depth == 1000).all()                   # no empty pixel: an edge value of exactly 0 counts for both sides
    rows = np.arange(H)
    assert (index[0, rows, rows + 8] == 0).all()                          # on the shared edge both triangles cover at equal depth: the first drawn wins
    assert (index[0, rows, rows + 9] == 0).all() and (index[0, rows[1:], rows[1:] + 7] == 1).all()


def test_closed_box_from_inside_has_no_empty_pixel():
    """20 seeded poses inside the 12-triangle box: every ray meets a wall, and every shared edge is watertight because the two triangles on
    it see edge values of exactly opposite sign."""
    depth, normal, index = rf.mirror("box20")
    assert index.shape == (20, H, W)
    assert int((index < 0).sum()) == 0
    assert int((depth == 0).sum()) == 0 and depth.max() <= 1000 * np.linalg.norm(np.array(rf.BOX_HALF) + 0.5) + 1
    assert normal.reshape(-1, 3).any(axis=1).all()


def test_floor_that_straddles_the_camera_plane():
    """y = 1 below the camera: the pixel of row r sees it at z = 1 / ry.  depth_mm = trunc(fl32(fl32(z) * 1000)): two float32 roundings, 2^-23
    relative together, and a truncation - so 1000 / ry - depth_mm lies in (-tol, 1 + tol) with tol = 2^-22 * 1000 / ry."""
    depth, normal, index = rf.mirror("floor")
    fy, cy = rf.K_BOX[1], rf.K_BOX[3]
    ry = ((np.arange(H) + 0.5) - cy) / fy
    seen = (ry > 0) & (1.0 / np.where(ry > 0, ry, 1.0) <= 20.0)
    assert seen.sum() >= 20 and (~seen).sum() >= 20
    assert not depth[0, ~seen].any() and (index[0, ~seen] == -1).all() and not normal[0, ~seen].any()      # at or above the horizon; beyond zfar
    mm = 1000.0 / ry[seen]
    diff = mm[:, None] - depth[0, seen].astype(np.float64)
    tol = (mm * 2.0 ** -22)[:, None]
    assert (diff > -tol).all() and (diff < 1 + tol).all()
    assert (index[0, seen] >= 0).all()
    assert (normal[0, seen] == np.uint8([128, 255, 127])).all()          # facing up in the GL camera: m = (1/255, -1, 1/255), g = (1/255, 1, -1/255)


def test_coplanar_duplicates_go_to_the_smaller_index():
    depth, normal, index = rf.mirror("dup")
    hit = index[0] >= 0
    assert hit.sum() > 500 and (~hit).sum() > 100
    assert (index[0][hit] == 0).all() and (depth[0][hit] == 1500).all()
    d2, n2, i2 = render_mesh(*rf.duplicates(flip=True), rf.identity_pose(), rf.K_BOX, H, W)      # the other winding first: still index 0 ...
    assert np.array_equal(i2, index) and np.array_equal(d2, depth)
    assert np.array_equal(n2, normal)                                    # ... and a back-facing triangle gives its front-facing twin's normal


def test_back_face_normal_equals_front_face_and_degenerates_are_skipped():
    v, f = rf.duplicates()
    front = render_mesh(v, f[:1], rf.identity_pose(), rf.K_BOX, H, W)
    back = render_mesh(v, f[1:], rf.identity_pose(), rf.K_BOX, H, W)
    for a, b in zip(front, back):
        assert np.array_equal(a, b)
    assert (front[1][front[2] >= 0] == np.uint8([128, 127, 255])).all()
    depth, _, index = render_mesh(*rf.with_degenerate(), rf.identity_pose(), rf.K_BOX, H, W)
    assert set(np.unique(index)) == {2, 3} and (depth == 2000).all()      # the two degenerate triangles at z = 1 hide nothing
    v, f = rf.with_degenerate()
    d, n, i = render_mesh(v, f[:2], rf.identity_pose(), rf.K_BOX, H, W)   # nothing but degenerate triangles: an empty image
    assert not d.any() and not n.any() and (i == -1).all()


def test_mask_and_range():
    mask = np.full((1, H, W), 255, np.uint8)
    mask[0, :5, :7] = 0
    mask[0, 9, 9] = 254
    depth, normal, index = render_mesh(*rf.plane(), rf.identity_pose(), rf.K_BOX, H, W, masks=mask)
    assert not depth[0, :5, :7].any() and depth[0, 9, 9] == 0 and (depth[mask == 255] == 2000).all()
    assert (normal == np.uint8([128, 127, 255])).all() and (index >= 0).all()                  # the mask leaves the normal (and the index) alone
    # the cut-offs act on the computed z, which is 2 to a few float64 roundings: 1e-9 either side of it decides
    for kw, seen in (({"znear": 2.5}, False), ({"zfar": 1.5}, False), ({"znear": 2.0 + 1e-9}, False), ({"zfar": 2.0 - 1e-9}, False),
                     ({"zfar": 2.0 + 1e-9}, True), ({"znear": 2.0 - 1e-9, "zfar": 2.5}, True)):
        d, n, i = render_mesh(*rf.plane(), rf.identity_pose(), rf.K_BOX, H, W, **kw)
        assert (d == 2000).all() and (i >= 0).all() if seen else (not d.any() and not n.any() and (i == -1).all()), kw
    d, _, i = rf.mirror("empty")                                          # a plane behind the camera
    assert not d.any() and (i == -1).all()
    for kw in ({"znear": 0.0}, {"zfar": 0.01}, {"zfar": 70.0}, {"znear": float("nan")}):
        with pytest.raises(ValueError):
            render_mesh(*rf.plane(), rf.identity_pose(), rf.K_BOX, H, W, **kw)
    with pytest.raises(ValueError):
        render_mesh(rf.plane()[0], np.int32([[0, 1, 4]]), rf.identity_pose(), rf.K_BOX, H, W)
    with pytest.raises(ValueError):
        render_mesh(*rf.plane(), rf.identity_pose(), (0.0, 40.0, 32.0, 24.0), H, W)


def test_ply_reader_round_trips(tmp_path):
    v, f = rf.bumpy_grid(n=6)
    for ascii_ in (False, True):
        p = str(tmp_path / f"mesh_{int(ascii_)}.ply")
        write_ply_mesh(p, v, f, ascii=ascii_)
        v2, f2 = read_ply_mesh(p)
        assert v2.dtype == np.float32 and f2.dtype == np.int32
        assert np.array_equal(v2, v) and np.array_equal(f2, f)
    # other scalar vertex properties of other types, x / y / z picked by name, uint indices, a scalar face property
    head = ("ply\nformat binary_little_endian 1.0\ncomment made by hand\nelement vertex 4\nproperty uchar red\nproperty double z\nproperty float x\n"
            "property short flag\nproperty float y\nelement face 2\nproperty list uchar uint vertex_indices\nproperty uchar label\nend_header\n")
    vert = np.zeros(4, np.dtype([("red", "u1"), ("z", "<f8"), ("x", "<f4"), ("flag", "<i2"), ("y", "<f4")]))
    vert["x"], vert["y"], vert["z"], vert["red"] = v[:4, 0], v[:4, 1], v[:4, 2], 9
    face = np.zeros(2, np.dtype([("n", "u1"), ("v", "<u4", 3), ("label", "u1")]))
    face["n"], face["v"] = 3, [[0, 1, 2], [0, 2, 3]]
    p = str(tmp_path / "props.ply")
    with open(p, "wb") as fh:
        fh.write(head.encode() + vert.tobytes() + face.tobytes())
    v3, f3 = read_ply_mesh(p)
    assert np.array_equal(v3, v[:4]) and np.array_equal(f3, np.int32([[0, 1, 2], [0, 2, 3]]))
    # the project's point-cloud writer: vertices with colours, no faces
    p = str(tmp_path / "cloud.ply")
    write_ply(p, v, np.full((len(v), 3), 0.5))
    v4, f4 = read_ply_mesh(p)
    assert np.array_equal(v4, v) and f4.shape == (0, 3)
    # a face that is no triangle
    for ascii_ in (False, True):
        p = str(tmp_path / f"quad_{int(ascii_)}.ply")
        body = (b"0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n" if ascii_
                else np.float32([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]).tobytes() + bytes([4]) + np.int32([0, 1, 2, 3]).tobytes())
        with open(p, "wb") as fh:
            fh.write((f"ply\nformat {'ascii' if ascii_ else 'binary_little_endian'} 1.0\nelement vertex 4\nproperty float x\nproperty float y\n"
                      "property float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n").encode() + body)
        with pytest.raises(ValueError, match="triangles"):
            read_ply_mesh(p)


def test_rescaled_size_and_intrinsics_match_the_reference():
    with np.load(os.path.join(ROOT, "tests", "golden", "render_golden.npz")) as g:
        assert len(g["in_size"]) == 3 and [1920, 1440] in g["in_size"].tolist()
        for size, K, target, out_size, K_out, K_colmap in zip(g["in_size"], g["K_in"], g["target"], g["out_size"], g["K_out"], g["K_colmap"]):
            got_size, got_K, _ = rescaled_size_and_intrinsics(tuple(size), K, (int(target), int(target) * 3.0 / 4))
            assert got_size == tuple(out_size)
            assert np.array_equal(got_K, K_out)
            assert np.array_equal(tool().colmap_intrinsics(got_K), K_colmap)
    assert rescaled_size_and_intrinsics((1920, 1440), np.eye(3), (920, 690.0))[0] == (920, 690)


def test_tool_end_to_end(tmp_path):
    """A raw scene -> the processed layout -> ``ScannetPPDataset``: the depth files hold the mirror's array, the blanked corner is invalid."""
    raw, out = str(tmp_path / "raw"), str(tmp_path / "processed")
    names = rf.write_raw_scene(raw)
    t = tool()
    assert t.main([raw, out, "--scenes", rf.SCENE, "--target-resolution", "64", "--frames-per-call", "4", "--lossless"]) == 6
    scene = os.path.join(out, rf.SCENE)
    with np.load(os.path.join(scene, "scene_metadata.npz")) as meta:
        assert meta["images"].tolist() == names
        poses, Ks = meta["trajectories"], meta["intrinsics"]
    assert poses.shape == (6, 4, 4) and Ks.shape == (6, 3, 3)
    assert np.allclose(Ks[2], [[42.0, 0, 32.1], [0, 41.0, 24.2], [0, 0, 1]], atol=1e-5)             # colmap convention: + 0.5
    mask = np.full((6, 48, 64), 255, np.uint8)
    mask[:, :5, :7] = 0
    depth, normal, _ = render_mesh(*rf.box(), poses, Ks, 48, 64, masks=mask)
    for i, n in enumerate(names):
        assert np.array_equal(np.array(Image.open(os.path.join(scene, "depth", n + ".png"))), depth[i])
        assert np.array_equal(np.array(Image.open(os.path.join(scene, "normal", n + ".webp"))), normal[i])
        assert Image.open(os.path.join(scene, "images", n + ".webp")).size == (64, 48)
    assert not depth[:, :5, :7].any() and (depth[:, 5:, 7:] > 0).all() and normal[:, :5, :7].any()
    assert t.main([raw, out, "--scenes", rf.SCENE, "--target-resolution", "64"]) == 0               # the scene exists: kept
    ds = ScannetPPDataset(out, scenes=[rf.SCENE], clip_length=2)
    sample = ds[0]                                                       # frames 0 and 3 of the scene (every third frame)
    assert len(sample["mask"]) == 2
    for j, i in enumerate((0, 3)):
        m = np.asarray(sample["mask"][j])
        assert not m[:5, :7].any() and m[5:, 7:].all()
        assert np.array_equal(-np.asarray(sample["cam_coord"][j])[2], depth[i].astype(np.float32) / 1000)


def test_library_and_header_carry_the_new_entry_points():
    from unigeo_amd import _lib
    lib = _lib.load_library()
    txt = open(os.path.join(ROOT, "include", "unigeo_hip.h")).read()
    for s in ("ug_render_opts_default", "ug_prep_render_mesh"):
        assert s in _lib.EXPORTS and hasattr(lib, s) and f" {s}(" in txt
    o = _lib.RenderOptsC()
    lib.ug_render_opts_default(ctypes.byref(o))
    assert (o.znear, o.zfar, o.flags) == (0.05, 20.0, 0)
