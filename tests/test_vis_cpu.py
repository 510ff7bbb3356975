"""CPU: the host mirror of the visualisation panels (unigeo_amd/harness/vis.py) against the reference's own panels
(tests/golden/vis_golden.npz, written by tests/golden/make_vis_golden.py from the reference's save_depth_normal_maps), and the harness loop
honouring ``vis_depth``.  Bytes are compared for equality: every step of the composition is one float32 operation."""
import os

import numpy as np
import pytest
import torch

from unigeo_amd.harness import SPECTRAL_R_LUT, SyntheticGeometryDataset, colorbar_strip, colorize, evaluate, panels_u8, save_depth_normal_maps
from unigeo_amd.harness import vis

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "vis_golden.npz"), allow_pickle=False)
T, H, W = G["depth"].shape


def test_fixture_holds_what_the_tests_assume():
    d, n, u8 = G["depth"], G["normals"], G["rgbs_u8"]
    assert (T, H, W) == (3, 20, 28) and d.dtype == n.dtype == G["rgbs"].dtype == G["cbar"].dtype == np.float32
    assert G["vmin"] == d.min() == np.float32(0.9) and G["vmax"] == d.max() == np.float32(10.0)
    assert len(np.unique(u8)) == 256
    comps = set(np.unique(n[0, 1, :6]).tolist())
    assert comps == {-1.0, 0.0, 1.0}
    u = (d - G["vmin"]) / np.float32(G["vmax"] - G["vmin"]) * np.float32(256)
    on_edge = (u == np.floor(u)) & (u > 0) & (u < 256)
    assert on_edge.sum() >= 5                                                      # depths whose u * 256 is an integer exactly
    Wc = G["cbar"].shape[1]
    assert G["cbar"].shape == (H, Wc, 3) and Wc == int(0.25 * H)
    assert G["panels_rgb"].shape == (T, H, 3 * W + 5 + Wc, 3) and G["panels_norgb"].shape == (T, H, 2 * W + 5 + Wc, 3)
    assert G["panels_rgb"].dtype == np.uint8


@pytest.mark.parametrize("with_rgb", [True, False])
def test_host_mirror_equals_the_reference_panels(with_rgb):
    got = panels_u8(G["depth"], G["normals"], G["vmin"], G["vmax"], G["lut"], rgbs=G["rgbs"] if with_rgb else None, cbar=G["cbar"])
    want = G["panels_rgb" if with_rgb else "panels_norgb"]
    assert got.dtype == np.uint8 and got.shape == want.shape
    print("differing bytes:", int((got != want).sum()))
    assert np.array_equal(got, want)


def test_host_mirror_reproduces_the_rgb_truncation():
    """byte k went through fl32(k / 255) * 255 and a truncation: the mirror returns what the reference returned (k or k - 1), it does not
    repair the round trip"""
    got = panels_u8(G["depth"], G["normals"], G["vmin"], G["vmax"], G["lut"], rgbs=G["rgbs"])[:, :, :W]
    assert np.array_equal(got, G["panels_rgb"][:, :, :W])
    diff = G["rgbs_u8"].astype(int) - got.astype(int)
    assert set(np.unique(diff).tolist()) <= {0, 1}


def test_host_range_and_torch_inputs():
    assert vis.depth_range(G["depth"]) == (G["vmin"], G["vmax"])
    d = G["depth"].copy(); d[0, 0, 0] = np.nan; d[1, 1, 1] = np.nan
    lo, hi = vis.depth_range(d)
    assert lo == np.delete(G["depth"].reshape(-1), [0, H * W + W + 1]).min() and hi == G["vmax"]
    assert vis.depth_range(np.full((2, 3), np.nan, np.float32)) == (0.0, 0.0) and vis.depth_range(np.zeros((0,), np.float32)) == (0.0, 0.0)
    t = torch.from_numpy
    a = panels_u8(t(G["depth"]), t(G["normals"]), G["vmin"], G["vmax"], t(G["lut"]), rgbs=t(G["rgbs"]), cbar=t(G["cbar"]))
    assert np.array_equal(a, G["panels_rgb"])


def test_shipped_table_is_the_fixtures_and_matplotlibs():
    assert SPECTRAL_R_LUT.shape == (256, 3) and SPECTRAL_R_LUT.dtype == np.float32
    assert np.array_equal(SPECTRAL_R_LUT, G["lut"])
    matplotlib = pytest.importorskip("matplotlib")
    assert np.array_equal(SPECTRAL_R_LUT, matplotlib.colormaps["Spectral_r"](np.arange(256))[:, :3].astype(np.float32))


def test_degenerate_range_and_nan_depth_are_black():
    d = np.full((1, 4, 6), 2.5, np.float32)
    assert not colorize(d, 2.5, 2.5, G["lut"]).any()                               # vmax == vmin: 0 / 0
    p = panels_u8(d, np.zeros((1, 4, 6, 3), np.float32), 2.5, 2.5, G["lut"])
    assert p.shape == (1, 4, 12, 3) and (p[:, :, :6] == 127).all() and not p[:, :, 6:].any()      # n = 0 -> trunc(0.5 * 255)
    d = G["depth"].copy(); d[1, 3, 4] = np.nan
    c = colorize(d, G["vmin"], G["vmax"], G["lut"])
    assert not c[1, 3, 4].any()
    d[1, 3, 4] = G["depth"][1, 3, 4]
    assert np.array_equal(np.delete(c.reshape(-1, 3), H * W + 3 * W + 4, 0), np.delete(colorize(d, G["vmin"], G["vmax"], G["lut"]).reshape(-1, 3), H * W + 3 * W + 4, 0))
    lut8 = vis.unit_to_u8(G["lut"])
    assert np.array_equal(colorize(np.array([G["vmin"], G["vmax"], -5.0, 50.0], np.float32), G["vmin"], G["vmax"], G["lut"]), lut8[[0, 255, 0, 255]])


def test_byte_cast_saturates():
    assert vis.unit_to_u8(np.array([-1.0, 0.0, 0.5, 1.0, 2.0, np.nan, np.inf, -np.inf], np.float32)).tolist() == [0, 0, 127, 255, 255, 0, 255, 0]


@pytest.mark.parametrize("h", [20, 64, 384])
def test_colorbar_strip_shape_and_range(h):
    pytest.importorskip("matplotlib")
    s = colorbar_strip(h, 0.9, 10.0)
    assert s.shape == (h, int(0.25 * h), 3) and s.dtype == np.float32
    assert s.min() >= 0.0 and s.max() <= 1.0 and s.max() > 0.9 and s.std() > 0.01
    assert colorbar_strip(h, 0.0, 0.0).shape == s.shape                            # a constant clip (StableNormal's zero depth) still renders


def test_area_resize_is_a_block_mean_at_integer_ratios_and_keeps_the_mean_otherwise():
    rng = np.random.default_rng(0)
    im = rng.uniform(size=(12, 8, 3)).astype(np.float32)
    np.testing.assert_allclose(vis.area_resize(im, 3, 4), im.reshape(3, 4, 4, 2, 3).mean(axis=(1, 3)), rtol=1e-6)
    np.testing.assert_allclose(vis.area_resize(im, 5, 3).mean(axis=(0, 1)), im.mean(axis=(0, 1)), rtol=1e-5)
    assert np.array_equal(vis.area_resize(im, 12, 8), im)


class _StubModel:
    """pred = the ground-truth depth and normals (OpenGL camera coordinates as the plugins return them)"""

    def forward(self, data):
        d = np.stack([-np.asarray(c)[2] for c in data["cam_coord"]], 0)
        n = np.stack([np.asarray(c).transpose(1, 2, 0) for c in data["cam_normal"]], 0)
        return {"pred_depths": torch.from_numpy(d).float(), "pred_normals": torch.from_numpy(np.ascontiguousarray(n)).float()}


def _cfg(**extra):
    return {"dataset": "SyntheticGeometryDataset", "root": "unused", "h": 64, "w": 64, "clip_length": 3, "clip_overlap": 1,
            "eval_depth": {"metric_names": ["Abs Rel", "delta < 1.25"]}, "eval_normal": {"metric_names": ["normal mean"]}, **extra}


def test_evaluate_writes_one_readable_image_per_frame_and_leaves_the_rows_alone(tmp_path):
    from PIL import Image
    ds = SyntheticGeometryDataset(clip_length=3, clip_overlap=1, input_size=(64, 64), num_frames=5)
    plain, _ = evaluate(_cfg(), dataset=ds, model=_StubModel(), save_dir=str(tmp_path / "plain"), verbose=False)
    rows, _ = evaluate(_cfg(vis_depth=True), dataset=ds, model=_StubModel(), save_dir=str(tmp_path / "vis"), verbose=False)
    assert rows == plain and len(rows) >= 2
    assert sorted(os.listdir(tmp_path / "plain")) == ["metrics.csv"]               # without the key no directory is made
    assert (tmp_path / "plain" / "metrics.csv").read_text() == (tmp_path / "vis" / "metrics.csv").read_text()
    strip = colorbar_strip(64, 0.0, 1.0)
    Wp = 3 * 64 + (5 + strip.shape[1] if strip is not None else 0)
    for r in rows:
        files = sorted(os.listdir(tmp_path / "vis" / f"depth_{r['seq_name']}"))
        assert [os.path.splitext(f)[0] for f in files] == [f"frame_{i:04d}" for i in range(3)]
        for f in files:
            with Image.open(tmp_path / "vis" / f"depth_{r['seq_name']}" / f) as im:
                im.load()
                assert im.size == (Wp, 64) and im.mode == "RGB"


def test_save_depth_normal_maps_returns_the_panels_it_wrote(tmp_path):
    from PIL import Image
    got = save_depth_normal_maps(torch.from_numpy(G["depth"]), torch.from_numpy(G["normals"]), str(tmp_path), rgbs=[torch.from_numpy(r) for r in G["rgbs"]])
    strip = colorbar_strip(H, G["vmin"], G["vmax"])
    assert np.array_equal(got, panels_u8(G["depth"], G["normals"], G["vmin"], G["vmax"], SPECTRAL_R_LUT, rgbs=G["rgbs"], cbar=strip))
    assert np.array_equal(got[:, :, :3 * W], G["panels_rgb"][:, :, :3 * W])        # everything left of the freshly rendered colour bar
    files = sorted(os.listdir(tmp_path))
    assert len(files) == T
    if files[0].endswith(".png"):                                                  # lossless: the file holds the panel
        assert np.array_equal(np.asarray(Image.open(tmp_path / files[0]).convert("RGB")), got[0])
    with pytest.raises(ValueError, match="engine"):
        save_depth_normal_maps(None, None, str(tmp_path))
