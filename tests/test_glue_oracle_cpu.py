"""CPU: the references of tests/glue_oracle.py against the project's oracle, and the proof that the cases and bounds of tests/test_glue_gpu.py can
tell a wrong kernel from a right one: restatements with one planted defect each must miss a case's bound by 10x or more."""
import inspect

import numpy as np
import pytest
import torch

import glue_oracle as G
from glue_oracle import CLIP_CASES, F32, h16

SMALL = [c for c in CLIP_CASES if c[4] < 224]


def _floor(video, S, ref64):
    """max |float32 oracle resize - float64 restatement| on one input."""
    from oracle.clip import resize_with_antialiasing
    o = resize_with_antialiasing(torch.from_numpy(video).permute(0, 3, 1, 2).contiguous(), (S, S)).permute(0, 2, 3, 1).numpy()
    return float(np.abs(o.astype(np.float64) - ref64).max())


def test_tap_counts_and_taps_match_the_oracle():
    from oracle.clip import antialias_taps
    for cid, T, H, W, S, P, Kpad, inet, (ky, kx) in CLIP_CASES:
        for src, k in ((H, ky), (W, kx)):
            ks, g = G.antialias_taps(src, S)
            ko, go = antialias_taps(src, S)
            assert ks == ko == k, (cid, src, ks, ko, k)
            np.testing.assert_allclose(g, go.numpy(), rtol=0, atol=3e-7)
    assert G.antialias_taps(28, 28)[1].tolist() == [0.0, 1.0, 0.0]
    assert G.antialias_taps(168, 28)[0] == 11 and G.antialias_taps(200, 28)[0] > 9      # the sizes the launcher must refuse


@pytest.mark.parametrize("case", CLIP_CASES, ids=[c[0] for c in CLIP_CASES])
def test_resize_restatement_matches_the_oracle(case):
    """float64 restatement vs oracle.clip.resize_with_antialiasing in float32.  Bound: the oracle's float32 source coordinate is off by up to one
    float32 spacing of the largest coordinate, 2^-23 * max(H, W) / 2, times the steepest slope of the cubic interpolant (1.5 x the value range);
    plus 64 float32 roundings of the two filters."""
    cid, T, H, W, S, P, Kpad, inet, _ = case
    T = min(T, 2)
    v = G.clip_case_input(np.random.default_rng(1), T, H, W)
    ref = G.resize_antialias(v, S)
    amp = float(v.max() - v.min())
    bound = 2.0 ** -24 * max(H, W) * 1.5 * amp + 64 * 2.0 ** -24 * amp
    fl = _floor(v, S, ref)
    assert fl <= bound, (cid, fl, bound)


def test_patch_matrix_matches_clip_and_dino_preprocess():
    from oracle.clip import clip_preprocess
    from oracle.stablenormal import dino_preprocess
    rng = np.random.default_rng(2)
    for S, H, W, inet, fn in ((224, 48, 80, False, clip_preprocess), (42, 64, 100, True, lambda x: dino_preprocess(x, 42))):
        v = G.clip_case_input(rng, 2, H, W)
        pv = fn(torch.from_numpy(v).permute(0, 3, 1, 2).contiguous())                    # [T,3,S,S]
        npp = S // 14
        want = pv.reshape(2, 3, npp, 14, npp, 14).permute(0, 2, 4, 1, 3, 5).reshape(2 * npp * npp, 588).numpy()   # the Conv2d patch embedding's K order
        got = G.clip_patchify(v, S, 14, 600, inet, fill=-7.0)
        assert (got[:, 588:] == -7.0).all()
        assert np.abs(got[:, :588] - want).max() < 2e-4 / 0.22


def _clip_case_data(case):
    cid, T, H, W, S, P, Kpad, inet, _ = case
    v = G.clip_case_input(np.random.default_rng(3), T, H, W)
    ref = G.clip_patchify(v, S, P, Kpad, inet)
    slack = G.clip_slack(_floor(v, S, G.resize_antialias(v, S)), S, P, Kpad, inet)
    return v, ref, slack


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_clip_bound_holds_for_a_float32_evaluation(case):
    """The GPU bound is attainable: the restatement evaluated in float32 and rounded to fp16 passes it."""
    cid, T, H, W, S, P, Kpad, inet, _ = case
    v, ref, slack = _clip_case_data(case)
    got = h16(G.clip_patchify(v, S, P, Kpad, inet, dtype=np.float32))
    assert G.f16_excess(got, ref, slack) <= 0.5


def test_scale_one_is_the_normalised_input():
    cid, T, H, W, S, P, Kpad, inet, _ = CLIP_CASES[0]
    v = G.clip_case_input(np.random.default_rng(3), T, H, W)
    mean, std = np.asarray(G.CLIP_MEAN, F32).astype(np.float64), np.asarray(G.CLIP_STD, F32).astype(np.float64)
    want = G.patch_matrix(((v.astype(np.float64) + 1) * 0.5 - mean) / std, P, Kpad, 0.0)
    assert np.abs(G.clip_patchify(v, S, P, Kpad) - want).max() < 1e-14


@pytest.mark.parametrize("defect", ["clamp", "taps", "half_pixel", "norm_swap", "transpose"])
def test_clip_planted_defects_miss_the_bound_tenfold(defect):
    worst = 0.0
    for case in SMALL:
        cid, T, H, W, S, P, Kpad, inet, _ = case
        v, ref, slack = _clip_case_data(case)
        bad = h16(G.clip_patchify(v, S, P, Kpad, inet, dtype=np.float32, defect=defect))
        worst = max(worst, G.bound_ratio(bad, ref, slack))
    assert worst >= 10.0, (defect, worst)


# ---------------------------------------------------------------------------------------------------- input preparation, sampler
def test_prep_video_matches_the_pipeline_in_half():
    rng = np.random.default_rng(4)
    frames = rng.uniform(0, 1, (2, 5, 7, 3)).astype(F32); noise = rng.standard_normal((2, 3, 5, 7)).astype(F32)
    for aug in (0.0, 0.02):
        src, vin = G.prep_video(frames, noise, aug)
        video = torch.from_numpy(frames).permute(0, 3, 1, 2).half() * 2.0 - 1.0                      # oracle/pipeline.py:51-52
        assert (src.reshape(2, 5, 7, 3) == video.permute(0, 2, 3, 1).float().numpy()).all()
        aug_v = (video + aug * torch.from_numpy(noise).half()).permute(0, 2, 3, 1).float().numpy()     # :62
        assert G.ulps16_apart(vin[:, :3].reshape(2, 5, 7, 3), aug_v) <= 1.0      # the host library may round the scalar 0.02 to fp16 first
        assert (vin[:, 3:] == 0).all()


def _sched():
    from oracle.scheduler import EulerKarrasVPred
    sch = EulerKarrasVPred(); sch.set_timesteps(5)
    return sch


def test_sampler_restatements_match_the_scheduler_in_half():
    sch = _sched(); rng = np.random.default_rng(5)
    noise = rng.standard_normal((3, 4, 5, 7)).astype(F32)
    want = (torch.from_numpy(noise).half() * sch.init_noise_sigma).permute(0, 2, 3, 1).reshape(-1, 4).float().numpy()      # oracle/pipeline.py:75
    assert (G.init_latents(noise, np.float32(sch.init_noise_sigma)) == want).all()
    for i in range(5):
        s = float(sch.sigmas[i])
        lat = h16(rng.standard_normal((105, 4)) * s); cond = h16(rng.standard_normal((105, 4)))
        den = np.sqrt(F32(s) * F32(s) + F32(1))
        ref = G.unet_input64(lat, cond, den, guided=True)
        ora = sch.scale_model_input(torch.from_numpy(lat).half(), i).float().numpy()
        assert G.f16_excess(ora, ref[:105, :4], 2.0 ** -23 * np.abs(ref[:105, :4])) <= 0.5
        assert (ref[:105, 4:] == cond).all() and (ref[105:, 4:] == 0).all() and (ref[105:, :4] == ref[:105, :4]).all()


@pytest.mark.parametrize("g", [1.5, 7.0])
def test_guided_v_matches_the_cfg_oracle(g):
    from cfg_oracle import GuidedUNet
    rng = np.random.default_rng(6)
    vc, vu = h16(rng.standard_normal((1, 3, 4, 5, 7))), h16(rng.standard_normal((1, 3, 4, 5, 7)))
    fake = lambda x, t, emb, added: torch.cat([torch.from_numpy(vu).half(), torch.from_numpy(vc).half()], 0)      # [unconditional, conditional]
    x = torch.zeros(1, 3, 8, 5, 7).half()
    want = GuidedUNet(fake, g)(x, None, torch.zeros(1, 3, 4).half(), torch.zeros(1, 3).half()).float().numpy()
    assert (G.guided_v(vc, vu, g) == want).all()


# ---------------------------------------------------------------------------------------------------- latent sliding windows
@pytest.mark.parametrize("overlap", [1, 2, 3, 5])
def test_window_formulas_match_the_pipeline(overlap):
    sch = _sched(); rng = np.random.default_rng(7)
    prev = torch.from_numpy(rng.standard_normal((1, overlap, 4, 5, 7))); cur = torch.from_numpy(rng.standard_normal((1, overlap, 4, 5, 7)) * 700)
    want = prev + cur / sch.init_noise_sigma * sch.sigmas[0].double()                                  # oracle/pipeline.py:96
    coef = F32(sch.sigmas[0].item()) / np.sqrt(F32(sch.sigmas[0].item()) ** 2 + F32(1))
    got = G.renoise64(prev.numpy().reshape(overlap, -1), cur.numpy().reshape(overlap, -1), coef)
    np.testing.assert_allclose(got, want.numpy().reshape(overlap, -1), rtol=0, atol=4 * 2.0 ** -24 * 700 * 5)
    weights = torch.linspace(0, 1, overlap, dtype=torch.float64).view(1, overlap, 1, 1, 1)            # :87
    fade = cur * weights + prev * (1 - weights)                                                        # :103
    got = G.crossfade64(cur.numpy().reshape(overlap, -1), prev.numpy().reshape(overlap, -1))
    np.testing.assert_allclose(got, fade.numpy().reshape(overlap, -1), rtol=0, atol=1e-12 * 700)
    if overlap == 1:
        assert (got == prev.numpy().reshape(1, -1)).all()


def test_crossfade_planted_weights_miss_the_bound_tenfold():
    rng = np.random.default_rng(8)
    worst = 0.0
    for overlap in (1, 2, 3, 5):
        cur, prev = h16(rng.standard_normal((overlap, 140))), h16(rng.standard_normal((overlap, 140)))
        ref = G.crossfade64(cur, prev)
        bad = h16(G.crossfade64(cur, prev, defect="weights"))
        worst = max(worst, G.bound_ratio(bad, ref, 2.0 ** -22 * (np.abs(cur) + np.abs(prev))))
        assert G.f16_excess(h16(ref), ref, 0.0) <= 0.5
    assert worst >= 10.0, worst


# ---------------------------------------------------------------------------------------------------- decoder tail, post-processing
@pytest.mark.parametrize("T", [1, 2, 5])
def test_time_conv_restatement_and_case(T):
    x, w, b = G.time_conv_case(np.random.default_rng(9), T)
    acc = G.time_conv_acc64(x, w, b)
    xt = torch.from_numpy(x[:, :, :3].astype(np.float64)).permute(2, 0, 1)[None, :, :, :, None]        # [1, C, T, HW, 1]
    want = torch.nn.functional.conv3d(xt, torch.from_numpy(w.astype(np.float64))[:, :, :, None, None], torch.from_numpy(b.astype(np.float64)),
                                      padding=(1, 0, 0))[0, :, :, :, 0].permute(1, 2, 0).reshape(-1, 3)
    np.testing.assert_allclose(acc, want.numpy(), rtol=0, atol=1e-13)
    np.testing.assert_array_equal(G.time_conv_frames64(acc), (want / 2 + 0.5).clamp(0, 1).numpy())    # oracle/pipeline.py:115
    assert np.abs(acc).max() < 4.0 and acc.max() > 1.0 and acc.min() < -1.0
    x2 = x.copy(); x2[:, :, 3:] = -3.0
    assert (G.time_conv_acc64(x2, w, b) == acc).all()


def test_time_conv_reversed_taps_miss_the_bound_tenfold():
    worst = 0.0
    for T in (1, 2, 5):
        x, w, b = G.time_conv_case(np.random.default_rng(9), T)
        acc = G.time_conv_acc64(x, w, b)
        bad = G.time_conv_frames64(h16(G.time_conv_acc64(x, w, b, defect="reversed")))
        worst = max(worst, float((np.abs(bad - G.time_conv_frames64(acc)) / (0.25 * G.ulp16(acc) + 1e-6)).max()))
    assert worst >= 10.0, worst


def test_depth_post_matches_the_wrapper_post_processing():
    from oracle.pipeline import depth_from_frames
    rng = np.random.default_rng(10)
    for off in (0.0, -0.7):
        fr = (rng.uniform(0, 1, (2, 6, 25, 3)) + off).astype(F32)
        depth, disp, mm = G.depth_post32(fr.reshape(-1, 3))
        want = np.stack(depth_from_frames(fr))
        assert want.dtype == np.float32 and (depth.reshape(2, 6, 25) == want).all()
        assert (depth == F32(1.0) / (disp + F32(0.1))).all() and disp.min() == 0.0 and disp.max() == 1.0


# ---------------------------------------------------------------------------------------------------- StableNormal glue
@pytest.mark.parametrize("h,w,g", [(12, 20, 16), (7, 9, 3), (16, 16, 16)])
def test_grid_gather_matches_the_controlnet(h, w, g):
    import oracle.stablenormal as sn
    src = inspect.getsource(sn.ControlNet.forward)
    assert "iy = (torch.arange(h) * g) // h" in src and "ix = (torch.arange(w) * g) // w" in src and "f[:, :, iy][:, :, :, ix]" in src
    rng = np.random.default_rng(11)
    x, grid = h16(rng.standard_normal((2, h, w, 16))), h16(rng.standard_normal((2, g, g, 16)))
    f = torch.from_numpy(grid).permute(0, 3, 1, 2)
    iy = (torch.arange(h) * g) // h
    ix = (torch.arange(w) * g) // w
    add = f[:, :, iy][:, :, :, ix]                                                                    # oracle/stablenormal.py, ControlNet.forward
    want = (torch.from_numpy(x).permute(0, 3, 1, 2).half() + add.half()).permute(0, 2, 3, 1).reshape(-1, 16).float().numpy()
    assert (G.add_grid_nearest(x, grid) == want).all()


def test_clip_assemble_matches_the_embedding_module():
    from oracle.clip import CLIPConfig, _Emb
    rng = np.random.default_rng(12)
    T, npp, d = 3, 4, 24
    emb = _Emb(CLIPConfig(hidden_size=d, image_size=28, patch_size=14))
    patches, cls, pos = h16(rng.standard_normal((T * npp, d))), h16(rng.standard_normal(d)), h16(rng.standard_normal((npp + 1, d)))
    with torch.no_grad():
        emb.class_embedding.copy_(torch.from_numpy(cls)); emb.position_embedding.weight.copy_(torch.from_numpy(pos))
        class Projected(torch.nn.Module):                                 # stands for the patch projection: [T, d, 2, 2]
            def forward(self, x):
                return torch.from_numpy(patches).reshape(T, 2, 2, d).permute(0, 3, 1, 2)
        emb.patch_embedding = Projected()
        want = emb(torch.zeros(T, 3, 28, 28)).reshape(T * (npp + 1), d).numpy()
    assert (G.clip_assemble(patches, cls, pos, T) == h16(want)).all()


def test_sn_normals_restatement():
    dec = np.array([[2.0, -3.0, 0.5, 9, 9], [0, 0, 0, 9, 9], [0.6, 0.0, -0.8, 9, 9]])
    out = G.sn_normals64(dec)
    np.testing.assert_allclose(out[0], np.array([1, -1, 0.5]) / 1.5, rtol=0, atol=1e-15)
    assert (out[1] == 0).all()
    np.testing.assert_allclose(out[2], [0.6, 0, -0.8], rtol=0, atol=1e-15)
