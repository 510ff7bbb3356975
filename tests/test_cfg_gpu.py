"""Classifier-free guidance on the MI355X (tiny full-topology configuration, whose 128-channel levels take the C % 128 paths): the batched
two-video UNet pass against the oracle, no leakage between the two videos, the guided pipeline (plain and windowed) against the guided
oracle (tests/cfg_oracle.py; restated, unpinned), guidance switched off again, fp8 linears under guidance and the plugin kwarg.
Tolerances are the ones the unguided tests of tests/test_stages_gpu.py use for the same stages."""
import numpy as np
import pytest
import torch

from util import assert_abs, assert_close, h16, report
from oracle_build import oracle_clip, oracle_unet, oracle_vae

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    from unigeo_amd import weights as W
    from unigeo_amd.pipeline import DepthCrafterPipelineHIP
    u, v, c = W.tiny_cfgs()
    su, sv, sc = (W.random_state(W.unet_manifest(u), 1), W.random_state(W.vae_manifest(v), 2),
                  W.random_state(W.clip_manifest(c), 3))
    pipe = DepthCrafterPipelineHIP.from_state(su, sv, sc, cfgs=(u, v, c), workspace_bytes=3 << 30)
    yield dict(pipe=pipe, eng=pipe.engine, cfgs=(u, v, c), unet=oracle_unet(u, su), vae=oracle_vae(v, sv), clip=oracle_clip(c, sc))
    pipe.engine.set_guidance(1.0)
    pipe.engine.close()


def _oracle_unet(tiny, x, emb, tstep):
    with torch.no_grad():
        return tiny["unet"](torch.from_numpy(x)[None], torch.tensor(tstep), torch.from_numpy(emb)[None],
                            torch.tensor([[7.0, 127.0, 0.02]]))[0].numpy()


# Larger latents make the convolutions write GroupNorm partial sums in their epilogues (stat_alloc: M >= 8192, and a tile whose statistics block
# divides the frame): at 96 x 128 latents (T = 5) every temporal GroupNorm of levels 0 and 1 reads them - from the spatial convolution launched once
# over both videos (its slice per video) and from the temporal convolution launched once per video (its block offset per video).
SIZES = [(5, 8, 16), (5, 96, 128)]


@pytest.mark.parametrize("T,h,w", SIZES)
def test_unet_pair_matches_the_oracle_per_video(tiny, T, h, w):
    """The guided pass's two halves: (conditioned, zero-conditioned) inputs in ONE batched UNet pass, each half against the oracle UNet."""
    rng = np.random.default_rng(11)
    u = tiny["cfgs"][0]
    xc = h16(rng.standard_normal((T, u.in_channels, h, w)))
    xu = xc.copy(); xu[:, 4:] = 0.0
    emb = h16(rng.standard_normal((T, u.cross_attention_dim)))
    zero = np.zeros_like(emb)
    tstep = 0.25 * np.log(3.7)
    got_c, got_u = tiny["eng"].unet_forward_pair(xc, emb, xu, zero, tstep)
    assert_close(got_c, _oracle_unet(tiny, xc, emb, tstep), 4.5e-3, "UNet pair forward, conditional half")
    assert_close(got_u, _oracle_unet(tiny, xu, zero, tstep), 4.5e-3, "UNet pair forward, unconditional half")


@pytest.mark.parametrize("T,h,w", SIZES)
def test_unet_pair_no_leakage_between_videos(tiny, T, h, w):
    """Same M, same tile plan in both runs: a bit of difference in the fixed video would be a temporal operator or a statistic crossing the
    video boundary.  At 96 x 128 latents the per-video temporal GroupNorms of levels 0 and 1 take their statistics from the convolutions'
    epilogue partial sums (checked through the shape-keyed profile: ':ep' = statistics from the producer's epilogue), so the per-video
    slicing of those partial sums is what is tested there."""
    rng = np.random.default_rng(12)
    u = tiny["cfgs"][0]
    a = h16(rng.standard_normal((T, u.in_channels, h, w)))
    ea = h16(rng.standard_normal((T, u.cross_attention_dim)))
    b1, eb1 = h16(rng.standard_normal(a.shape)), h16(rng.standard_normal(ea.shape))
    b2, eb2 = h16(rng.standard_normal(a.shape) * 4.0 + 3.0), h16(-3.0 * rng.standard_normal(ea.shape))
    tstep = 0.25 * np.log(11.0)
    eng = tiny["eng"]
    eng.profile_begin(shapes=True)
    try:
        a1, o1 = eng.unet_forward_pair(a, ea, b1, eb1, tstep)
    finally:
        prof = eng.profile_end()
    if h * w >= 8192:      # every per-video temporal GroupNorm of levels 0 and 1 (both videos' launches) reads epilogue partial sums
        temporal = {k: v["calls"] for k, v in prof.items() if k.startswith("groupnorm:") and ("t:" in k or k.endswith("t"))}
        for hw in (h * w, h * w // 4):
            lvl = {k: n for k, n in temporal.items() if k.startswith(f"groupnorm:T{T}xHW{hw}xC")}
            assert lvl and all(k.endswith("t:ep") for k in lvl) and sum(lvl.values()) % 2 == 0, temporal
    a2, o2 = eng.unet_forward_pair(a, ea, b2, eb2, tstep)
    assert np.abs(o1 - o2).max() > 1e-2                       # the second video really changed
    assert np.array_equal(a1, a2)
    ob1, ra1 = eng.unet_forward_pair(b1, eb1, a, ea, tstep)    # reverse direction: the fixed video second
    ob2, ra2 = eng.unet_forward_pair(b2, eb2, a, ea, tstep)
    assert np.array_equal(ra1, ra2)


def _frames(T, seed):
    from unigeo_amd.pipeline import make_noise
    rng = np.random.default_rng(seed)
    frames = (rng.uniform(0, 255, (T, 64, 64, 3)).astype(np.uint8)).astype(np.float32) / 255.0
    nl, na = make_noise(T, 64, 64, seed=seed)
    return frames, nl, na


def test_guided_pipeline_matches_the_guided_oracle_and_switches_off(tiny):
    from cfg_oracle import run_pipeline_cfg
    pipe, eng = tiny["pipe"], tiny["eng"]
    T = 3
    frames, nl, na = _frames(T, 21)
    fresh = pipe(frames, num_inference_steps=2, window_size=T, noise_latents=nl, noise_aug=na).frames[0]
    got = pipe(frames, num_inference_steps=2, guidance_scale=1.2, window_size=T, noise_latents=nl, noise_aug=na).frames[0]
    ref = run_pipeline_cfg(tiny["unet"], tiny["vae"], tiny["clip"], frames, torch.from_numpy(nl), torch.from_numpy(na), 2, 1.2)
    assert got.shape == ref.shape == (T, 64, 64, 3)
    assert_abs(got, ref, 1e-2, "tiny guided pipeline g=1.2, 2 steps (frames in [0,1])")
    assert np.abs(got - fresh).max() > 1e-4
    # lanes (independent encode / decode chunks on more streams) keep the guided result bit for bit
    eng.set_concurrency(2)
    try:
        lanes = pipe(frames, num_inference_steps=2, guidance_scale=1.2, window_size=T, noise_latents=nl, noise_aug=na).frames[0]
    finally:
        eng.set_concurrency(1)
    assert np.array_equal(lanes, got)
    # co-scheduled mode (tile planning and the fused feed-forward's row split change, so bit identity is not expected) stays on the oracle
    eng.set_coscheduled(True)
    try:
        cos = pipe(frames, num_inference_steps=2, guidance_scale=1.2, window_size=T, noise_latents=nl, noise_aug=na).frames[0]
    finally:
        eng.set_coscheduled(False)
    assert_abs(cos, ref, 1e-2, "tiny guided pipeline g=1.2, co-scheduled context")
    # the parity trace records the latents after each guided step
    eng.set_inputs(frames, nl, na)
    eng.set_guidance(1.2)
    tr = eng.run_traced(2)
    assert tr.shape == (2, T, 4, 8, 8) and np.isfinite(tr).all()
    assert np.array_equal(eng.get_outputs(frames=True, depth=False)[0], got)
    # guidance off again: the unguided path, bit-identical to the fresh run
    eng.set_guidance(1.0)
    eng.set_inputs(frames, nl, na)
    eng.run(2, 8)
    assert np.array_equal(eng.get_outputs(frames=True, depth=False)[0], fresh)
    again = pipe(frames, num_inference_steps=2, guidance_scale=1.0, window_size=T, noise_latents=nl, noise_aug=na).frames[0]
    assert np.array_equal(again, fresh)


def test_guided_latent_sliding_windows(tiny):
    from cfg_oracle import run_pipeline_cfg_windows
    T, window, overlap, g = 10, 6, 2, 1.5
    frames, nl, na = _frames(T, 22)
    got = tiny["pipe"](frames, num_inference_steps=2, guidance_scale=g, window_size=window, overlap=overlap, noise_latents=nl,
                       noise_aug=na).frames[0]
    ref = run_pipeline_cfg_windows(tiny["unet"], tiny["vae"], tiny["clip"], frames, torch.from_numpy(nl), torch.from_numpy(na), 2, g,
                                   window=window, overlap=overlap)
    assert got.shape == ref.shape
    assert_abs(got, ref, 1.4e-2, f"guided latent sliding windows T={T} window={window} overlap={overlap} g={g}")


def test_guided_pipeline_with_fp8_linears(tiny):
    pipe, eng = tiny["pipe"], tiny["eng"]
    T = 3
    frames, nl, na = _frames(T, 23)
    f16 = pipe(frames, num_inference_steps=2, guidance_scale=1.2, window_size=T, noise_latents=nl, noise_aug=na).frames[0]
    eng.set_fp8_linears(True)
    try:
        f8 = pipe(frames, num_inference_steps=2, guidance_scale=1.2, window_size=T, noise_latents=nl, noise_aug=na).frames[0]
    finally:
        eng.set_fp8_linears(False)
    assert np.isfinite(f8).all() and f8.min() >= 0.0 and f8.max() <= 1.0
    emean = report("tiny guided pipeline g=1.2: fp8-linear frames vs fp16-path frames, mean abs", float(np.abs(f8 - f16).mean()))
    assert emean <= 2e-2


def test_plugin_guidance_kwarg():
    from unigeo_amd.model import DepthCrafter
    from unigeo_amd.synthetic import synthetic_clip
    m = DepthCrafter(synthetic_weights=True, tiny=True, guidance_scale=1.2, num_inference_steps=2, workspace_bytes=3 << 30)
    try:
        data = synthetic_clip(3, 64, 64, seed=4)
        data["_index"] = 3
        g = m.forward(data)
        m.guidance_scale = 1.0
        p = m.forward(data)
    finally:
        m.pipeline.engine.close()
    for out in (g, p):
        assert torch.isfinite(out["pred_depths"]).all() and torch.isfinite(out["pred_normals"]).all()
    assert not torch.equal(g["pred_depths"], p["pred_depths"])
