"""CPU: the RGB-D loaders of unigeo_amd/harness/rgbd.py against tests/golden/rgbd_golden.npz - what the reference's
own ``*Sequence`` / ``*Sample`` classes return on the scenes under tests/golden/rgbd_scenes (tests/golden/make_rgbd_golden.py) -, the UNPINNED
parts (TUM reader, resize) against scipy / ``_resize``, and ``prepare_gt_label`` / ``evaluate`` on samples without ground-truth normals."""
import hashlib
import os
import shutil

import numpy as np
import pytest

from unigeo_amd.harness import SyntheticGeometryDataset, evaluate, import_class_from_module, prepare_gt_label
from unigeo_amd.harness import rgbd
from unigeo_amd.harness.scannetpp import _resize

G = os.path.join(os.path.dirname(__file__), "golden")
SCENES = os.path.join(G, "rgbd_scenes")
SCENE = {"7scenes": "chess/seq-03", "bonn": "rgbd_bonn_balloon2", "neuralrgbd": "breakfast_room", "replica": "room_0", "scannetv2": "scene0707_00"}
LAYOUTS = sorted(SCENE)
CLIP = dict(clip_length=3, clip_overlap=0)
ARRAYS = ("images", "extrinsics", "intrinsics", "cam_coord", "world_coord", "mask")
STRIDE = 16                                                  # the sub-grid of ScanNetv2's 480 x 640 arrays the golden keeps


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(G, "rgbd_golden.npz")) as f:
        return {k: f[k] for k in f.files}


def _dataset(L, **kw):
    return rgbd.LAYOUTS[L](os.path.join(SCENES, L), scenes=[SCENE[L]], **CLIP, **kw)


@pytest.fixture(scope="module")
def native():
    """layout -> (dataset, first clip, last clip) at native size on the host; read-only."""
    out = {}
    for L in LAYOUTS:
        ds = _dataset(L)
        out[L] = (ds, ds[0], ds[len(ds) - 1])
    return out


@pytest.mark.parametrize("L", [x for x in LAYOUTS if x != "bonn"])
def test_sequence_matches_the_reference(gold, native, L):
    seq = native[L][0].samples[0][0]
    assert np.array_equal(np.asarray(seq.extrinsics), gold[f"{L}_ext"])
    assert np.array_equal(np.asarray(seq.intrinsics), gold[f"{L}_K"])
    assert list(seq.rgb_paths) == gold[f"{L}_rgb"].tolist() and list(seq.depth_paths) == gold[f"{L}_depth"].tolist()
    assert list(seq.clips.keys()) == gold[f"{L}_clip_keys"].tolist()
    assert np.array_equal(np.array(list(seq.clips.values())), gold[f"{L}_clip_ids"])
    assert seq.clips[3][-1] == seq.clips[3][-2]              # the padded last clip shows


def test_the_fixtures_show_the_gap_the_order_and_the_dropped_block(gold):
    assert gold["neuralrgbd_rgb"].tolist() == [f"images/img{i}.png" for i in (0, 3, 7, 10)]          # block 4 invalid, removed before the gap
    assert gold["replica_rgb"].tolist() == [f"imap/00/rgb/rgb_{i}.png" for i in (0, 3, 6, 9)]          # by number, not by name
    assert gold["scannetv2_rgb"].tolist() == [f"color_270/{i:06d}.jpg" for i in (0, 20, 40, 60)]
    assert len(gold["7scenes_rgb"]) == 5


@pytest.mark.parametrize("L", LAYOUTS)
def test_sample_matches_the_reference(gold, native, L):
    ds = native[L][0]
    assert len(ds) == 2
    for ci in range(2):
        s = native[L][1 + ci]
        assert list(s.keys()) == gold[f"{L}_c{ci}_keys"].tolist() + ["_index", "_dataset"]
        assert "cam_normal" not in s and "world_normal" not in s
        assert s["_index"] == ci and s["_dataset"] == ds.base_dataset == ds.layout.base_dataset
        assert s["scene_name"] == str(gold[f"{L}_c{ci}_scene"]) and s["image_names"] == gold[f"{L}_c{ci}_names"].tolist()
        assert s["keyview_idx"] == 0 and s["caption"] == "" and s["_base"] == ds.root
        for k in ARRAYS:
            a = np.stack(s[k])
            if L == "scannetv2" and k not in ("extrinsics", "intrinsics"):
                assert a.shape[-2:] == (480, 640)
                if f"{L}_c{ci}_{k}_sha256" in gold:                                           # the whole array, bit for bit
                    assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() == str(gold[f"{L}_c{ci}_{k}_sha256"]), k
                a = a[..., ::STRIDE, ::STRIDE]
            g = gold[f"{L}_c{ci}_{k}"]
            assert a.dtype == g.dtype == np.float32 and a.shape == g.shape, k
            assert np.array_equal(a, g), k
            assert np.array_equal(np.signbit(a), np.signbit(g)), k                            # -0 where the reference has -0


def test_the_fixtures_hold_the_edge_cases(native):
    for L, zero, far in (("7scenes", (5, 5), (6, 6)), ("neuralrgbd", (5, 5), (6, 6)), ("replica", (5, 5), (6, 6)), ("scannetv2", (16, 32), (32, 48)),
                         ("bonn", (5, 5), None)):              # Replica: source pixels (5, 9) and (6, 10), four columns cropped
        m = np.stack(native[L][1]["mask"])
        assert m[(slice(None),) + zero].max() == 0 and m.mean() > 0.9, L
        if far is not None:
            assert m[(slice(None),) + far].max() == 0, L
    m = np.stack(native["neuralrgbd"][1]["mask"])
    assert m[:, 7, 7].min() == 1 and m[:, 7, 8].max() == 0    # 10.000 m stays, 10.001 m goes
    s = native["replica"][1]
    assert s["images"][0].shape == (3, 24, 32) and s["intrinsics"][0][0, 2] == np.float32(599.5 - 4) and s["intrinsics"][0][1, 2] == np.float32(339.5)
    y = np.stack(native["scannetv2"][1]["cam_coord"])[:, 1, 240]
    assert np.signbit(y[np.stack(native["scannetv2"][1]["mask"])[:, 240] > 0]).all() and not y.any()     # y = -0 on the principal row


def test_bonn_float64_depth_differs_from_float32_depth(gold, native):
    """The golden (the reference's float64 depth) is what the loader gives; the same clip through float32 depth differs in x."""
    class Bonn32(rgbd.BonnLayout):
        depth_f64 = False
    root = os.path.join(SCENES, "bonn")
    seq32 = rgbd.RGBDSequence(root, SCENE["bonn"], Bonn32(), **CLIP)
    s32 = rgbd.load_clip(root, seq32, seq32.clips[0])
    c64, c32, g = np.stack(native["bonn"][1]["cam_coord"]), np.stack(s32["cam_coord"]), gold["bonn_c0_cam_coord"]
    valid = gold["bonn_c0_mask"] > 0
    assert np.array_equal(c64, g)
    assert np.array_equal(np.stack(s32["mask"]), gold["bonn_c0_mask"])
    n = int((c32[:, 0][valid] != g[:, 0][valid]).sum())
    print(f"float32 depth: x differs in {n} of {int(valid.sum())} valid pixels")
    assert n >= 1 and np.array_equal(c32[:, 2], g[:, 2])


@pytest.mark.parametrize("L", LAYOUTS)
def test_resized_sample_is_resize_of_the_native_sample(native, L):
    size = (48, 64) if L == "scannetv2" else (12, 16)
    ds = _dataset(L, input_size=size, target_size=size)
    s, n = ds[0], native[L][1]
    assert list(s.keys()) == list(n.keys())
    oh, ow = n["images"][0].shape[-2:]
    scale = np.array([[size[1] / ow] * 3, [size[0] / oh] * 3, [1.0] * 3], np.float32)
    for j in range(3):
        np.testing.assert_array_equal(s["images"][j], _resize(n["images"][j], *size, 1, True))
        np.testing.assert_array_equal(s["intrinsics"][j], n["intrinsics"][j] * scale)
        np.testing.assert_array_equal(s["extrinsics"][j], n["extrinsics"][j])
        for k in ("cam_coord", "world_coord", "mask"):
            np.testing.assert_array_equal(s[k][j], _resize(n[k][j], *size, 0, False))
            assert s[k][j].dtype == np.float32 and s[k][j].shape[-2:] == size


def test_tum_reader_against_scipy(tmp_path):
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(3)
    q = rng.normal(size=(20, 4)) * rng.uniform(0.5, 2.0, (20, 1))                              # (x, y, z, w), not unit length
    t = rng.normal(size=(20, 3))
    with open(tmp_path / "gt.txt", "w") as f:
        f.write("# ground truth\n#timestamp tx ty tz qx qy qz qw\n\n")
        for i in range(20):
            f.write(" ".join(repr(float(v)) for v in [100.0 + i, *t[i], *q[i]]) + "\n")
    stamps, T = rgbd.read_tum_trajectory(str(tmp_path / "gt.txt"))
    assert T.shape == (20, 4, 4) and T.dtype == np.float64 and np.array_equal(stamps, 100.0 + np.arange(20))
    assert np.abs(T[:, :3, :3] - Rotation.from_quat(q).as_matrix()).max() <= 1e-12
    assert np.array_equal(T[:, :3, 3], t) and np.array_equal(T[:, 3], np.tile([0, 0, 0, 1.0], (20, 1)))
    with open(tmp_path / "bad.txt", "w") as f:
        f.write("1 2 3\n")
    with pytest.raises(ValueError, match="8 numbers"):
        rgbd.read_tum_trajectory(str(tmp_path / "bad.txt"))


def test_7scenes_nan_pose_drops_the_three_files_together(tmp_path):
    src = os.path.join(SCENES, "7scenes", SCENE["7scenes"])
    dst = tmp_path / "chess" / "seq-03"
    shutil.copytree(src, dst)
    pose = np.genfromtxt(dst / "frame-000002.pose.txt")
    pose[1, 3] = np.nan
    np.savetxt(dst / "frame-000002.pose.txt", pose)
    seq = rgbd.RGBDSequence(str(tmp_path), SCENE["7scenes"], rgbd.SevenScenesLayout(), **CLIP)
    full = rgbd.RGBDSequence(os.path.join(SCENES, "7scenes"), SCENE["7scenes"], rgbd.SevenScenesLayout(), **CLIP)
    keep = [0, 1, 3, 4]
    assert seq.rgb_paths == [f"frame-{i:06d}.color.png" for i in keep] and seq.depth_paths == [f"frame-{i:06d}.depth.proj.png" for i in keep]
    assert len(seq.extrinsics) == len(seq.intrinsics) == 4 and np.isfinite(seq.extrinsics).all()
    np.testing.assert_array_equal(seq.extrinsics, full.extrinsics[keep])
    assert list(seq.clips.values()) == [[0, 1, 2], [3, 3, 3]]


def test_scene_list_errors(tmp_path):
    root = os.path.join(SCENES, "7scenes")
    with pytest.raises(FileNotFoundError, match="scenes=.*split_file|split_file.*scenes="):
        rgbd.sevenScenesDataset(root)
    with pytest.raises(ValueError, match="nested"):
        rgbd.sevenScenesDataset(root, scenes="all")
    with pytest.raises(FileNotFoundError):
        rgbd.sevenScenesDataset(root, split_file=str(tmp_path / "missing.txt"))
    with pytest.raises(ValueError, match="prep"):
        rgbd.sevenScenesDataset(root, scenes=[SCENE["7scenes"]], prep="gpu")
    with open(tmp_path / "test.txt", "w") as f:
        f.write(SCENE["7scenes"] + "\n\n")
    assert len(rgbd.sevenScenesDataset(root, split_file=str(tmp_path / "test.txt"), **CLIP)) == 2


def test_prepare_gt_label_without_normals(native):
    s = native["7scenes"][1]
    gt = prepare_gt_label(s)
    assert set(gt) == {"gt_world_pts", "gt_masks", "gt_poses", "gt_depths", "gt_rgbs"}
    assert gt["gt_depths"].shape == (3, 24, 32) and gt["gt_masks"].dtype.is_floating_point is False
    np.testing.assert_array_equal(gt["gt_depths"].numpy(), -np.stack(s["cam_coord"])[:, 2])
    syn = SyntheticGeometryDataset(clip_length=3, clip_overlap=0, input_size=(16, 24), num_frames=3)[0]
    gs = prepare_gt_label(syn)
    assert list(gs) == ["gt_world_pts", "gt_masks", "gt_poses", "gt_depths", "gt_rgbs", "gt_normals"]
    np.testing.assert_array_equal(gs["gt_normals"].numpy(), np.stack(syn["cam_normal"]).transpose(0, 2, 3, 1))


class _Stub:
    """pred = 2 gt + 0.5, zero normals; counts its calls."""
    calls = 0

    def forward(self, data):
        import torch
        type(self).calls += 1
        d = np.stack([-np.asarray(c)[2] for c in data["cam_coord"]], 0)
        return {"pred_depths": torch.from_numpy(2.0 * d + 0.5).float(), "pred_normals": torch.zeros(d.shape + (3,))}


def _cfg(L, **kw):
    return dict({"dataset": rgbd.LAYOUTS[L].__name__, "root": os.path.join(SCENES, L),
                 "scenes": [SCENE[L]], "h": 12, "w": 16, "clip_length": 3, "clip_overlap": 0, "split": "test", "model_name": "DepthCrafter",
                 "model_params": {}, "eval_depth": {"metric_names": ["Abs Rel", "delta < 1.25"], "depth_alignment": "lstsq"}}, **kw)


def test_evaluate_with_eval_normal_raises_before_the_model_runs(tmp_path):
    class Stub(_Stub):
        calls = 0
    cfg = _cfg("7scenes", eval_normal={"metric_names": ["normal mean"]})
    with pytest.raises(ValueError, match=r"7scenes.*cam_normal"):
        evaluate(cfg, model=Stub(), save_dir=str(tmp_path), verbose=False)
    assert Stub.calls == 0


def test_evaluate_end_to_end_on_7scenes(tmp_path):
    rows, _ = evaluate(_cfg("7scenes"), model=_Stub(), save_dir=str(tmp_path), verbose=False)
    assert [r["seq_name"] for r in rows] == ["000_chess_seq-03", "001_chess_seq-03"]
    for r in rows:
        print(r)
        assert r["Abs Rel"] < 1e-5
    with open(tmp_path / "metrics.csv") as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip()]
    assert sum("chess_seq-03" in ln for ln in lines) == 2


def test_the_reference_names_resolve():
    for name, base in (("sevenScenesDataset", "7scenes"), ("bonnDataset", "bonn"), ("neuralRGBDDataset", "neuralRGBD"), ("replicaDataset", "replica"),
                       ("ScannetV2Dataset", "scannetv2")):
        cls = import_class_from_module("unigeo_amd.harness", name)
        assert issubclass(cls, rgbd.RGBDClipDataset) and cls.layout.base_dataset == base
