"""Stage-level parity through the C ABI: CLIP tower, VAE encode/decode, one UNet forward and the full
denoise pipeline of the HIP engine against the torch-CPU fp32 oracle, on a tiny configuration with the
full topology (every block type, skip-concats, up/down-sampling, spatial + temporal attention) that the
oracle finishes in seconds.

Tolerances (written per test): the engine stores every activation in fp16 (fp32 accumulate); the oracle is
fp32 throughout.  Every bound below is <= ~2x the error MEASURED on MI355X for that case (the measured values are
printed as PARITY lines and committed under profiles/r02_parity_measured.jsonl): 1.1e-3 - 2.2e-3 of the output scale
for a stage, 3e-3 - 7.6e-3 absolute on decoded frames in [0,1] for a whole pipeline.  The kernels are deterministic, so the
measured value is reproduced bit for bit from run to run and box to box.  north_star's 1e-3 is vs an fp16 *reference*
(same storage roundings); see DESIGN.md "Numerics".
"""
import numpy as np
import pytest
import torch

from util import assert_abs, assert_close, fp16_storage, h16, rel_err, report
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
    yield dict(pipe=pipe, eng=pipe.engine, cfgs=(u, v, c), unet=oracle_unet(u, su), vae=oracle_vae(v, sv),
               clip=oracle_clip(c, sc))
    pipe.engine.close()


def test_clip_embed(tiny):
    from oracle.clip import clip_preprocess
    rng = np.random.default_rng(0)
    frames = h16(rng.uniform(0, 1, (3, 64, 128, 3)))
    got = tiny["eng"].clip_embed(frames)
    with torch.no_grad():
        v = torch.from_numpy(frames).permute(0, 3, 1, 2) * 2.0 - 1.0
        ref = tiny["clip"](clip_preprocess(v)).numpy()
    assert_close(got, ref, 2.5e-3, "CLIP image embedding")


def test_clip_embed_heads_of_80_fused_and_four_launch():
    """The tiny tower has two heads of 32; this one has the real tower's head dim - hidden 160 = 2 heads of 80, 2 layers, S = 257 tokens, 2 frames - so
    that flash_attn_dh_kernel<80> runs inside clip_embed, and with UG_CLIP_UNFUSED (read per call) the four-launch path it replaced.  Both against the
    oracle's tower at test_clip_embed's bound, and against each other."""
    import os
    from oracle.clip import clip_preprocess
    from unigeo_amd import weights as W
    from unigeo_amd._lib import Engine
    c = W.CLIPCfg(hidden_size=160, intermediate_size=320, num_hidden_layers=2, num_attention_heads=2, image_size=224, patch_size=14, projection_dim=48)
    sc = W.random_state(W.clip_manifest(c), 5)
    frames = h16(np.random.default_rng(5).uniform(0, 1, (2, 64, 96, 3)))
    with torch.no_grad():
        ref = oracle_clip(c, sc)(clip_preprocess(torch.from_numpy(frames).permute(0, 3, 1, 2) * 2.0 - 1.0)).numpy()
    eng = Engine(0, workspace_bytes=1 << 30, persist_bytes=256 << 20)
    try:
        eng.load_state("clip.", sc); eng.bind_clip(c)
        assert "UG_CLIP_UNFUSED" not in os.environ
        fused = eng.clip_embed(frames)
        os.environ["UG_CLIP_UNFUSED"] = "1"
        try:
            unfused = eng.clip_embed(frames)
        finally:
            del os.environ["UG_CLIP_UNFUSED"]
        assert np.array_equal(eng.clip_embed(frames), fused)      # the variable is read per call, and the kernels are deterministic
    finally:
        eng.close()
    assert_close(fused, ref, 2.5e-3, "CLIP image embedding, 2 heads of 80, fused attention")
    assert_close(unfused, ref, 2.5e-3, "CLIP image embedding, 2 heads of 80, four-launch attention")
    assert_close(fused, unfused, 2.5e-3, "CLIP image embedding, 2 heads of 80, fused vs four-launch attention")
    assert not np.array_equal(fused, unfused)      # really two paths


def test_vae_encode(tiny):
    """Default = the reference's float32 encoder (force_upcast): fp32-grade arithmetic on fp16 hi/lo activation pairs
    (kernels/wide.hip); the output is the pipeline's fp16 latent, so the floor is one fp16 rounding (2^-11 = 4.9e-4)."""
    rng = np.random.default_rng(1)
    video = h16(rng.uniform(-1, 1, (2, 64, 64, 3)))
    with torch.no_grad():
        ref = tiny["vae"].encode_mode(torch.from_numpy(video).permute(0, 3, 1, 2)).numpy()
    got = tiny["eng"].vae_encode(video)
    assert_close(got, ref, 6e-4, "tiny VAE encode, float32-grade (posterior mode, fp16 output)")
    tiny["eng"].set_vae_encode_fp32(False)
    try:
        got16 = tiny["eng"].vae_encode(video)
    finally:
        tiny["eng"].set_vae_encode_fp32(True)
    assert_close(got16, ref, 4e-3, "tiny VAE encode, fp16 storage (posterior mode)")


@pytest.mark.parametrize("T", [1, 3])
def test_vae_decode(tiny, T):
    rng = np.random.default_rng(2)
    z = h16(rng.standard_normal((T, 4, 8, 8)) * 2)
    got = tiny["eng"].vae_decode(z)
    with torch.no_grad():
        fr = tiny["vae"].decode(torch.from_numpy(z), T)
        ref = (fr / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).numpy()
    # frames live in [0,1]: bound the absolute error
    assert_abs(got, ref, 5e-3, f"tiny VAE decode T={T} (frames in [0,1])")


@pytest.mark.parametrize("T,h,w", [(3, 8, 8), (5, 8, 16)])
def test_unet_forward(tiny, T, h, w):
    rng = np.random.default_rng(3)
    u = tiny["cfgs"][0]
    x = h16(rng.standard_normal((T, u.in_channels, h, w)))
    emb = h16(rng.standard_normal((T, u.cross_attention_dim)))
    tstep = 0.25 * np.log(3.7)
    got = tiny["eng"].unet_forward(x, tstep, emb)
    with torch.no_grad():
        ref = tiny["unet"](torch.from_numpy(x)[None], torch.tensor(tstep), torch.from_numpy(emb)[None],
                           torch.tensor([[7.0, 127.0, 0.02]]))[0].numpy()
    assert_close(got, ref, 4.5e-3, "UNet forward")


def test_pipeline_end_to_end(tiny):
    from oracle.pipeline import depth_from_frames, run_pipeline
    from unigeo_amd.pipeline import make_noise
    rng = np.random.default_rng(4)
    T, H, W = 3, 64, 64
    frames = (rng.uniform(0, 255, (T, H, W, 3)).astype(np.uint8)).astype(np.float32) / 255.0
    nl, na = make_noise(T, H, W, seed=7)
    res = tiny["pipe"](frames, height=H, width=W, num_inference_steps=2, window_size=T, noise_latents=nl, noise_aug=na)
    ref, st = run_pipeline(tiny["unet"], tiny["vae"], tiny["clip"], frames, torch.from_numpy(nl), torch.from_numpy(na),
                           steps=2, return_stages=True)
    got = res.frames[0]
    assert got.shape == ref.shape == (T, H, W, 3)
    assert np.isfinite(got).all()
    assert_abs(got, ref, 1e-2, "tiny pipeline end to end, 2 steps (frames in [0,1])")
    # wrapper post-processing (channel mean, clip-global min-max, 1/(x+0.1)) done on device
    dref = np.stack(depth_from_frames(got), 0)
    assert_close(res.depth, dref, 1e-5, "on-device depth post-processing")


def test_unet_fp16_accuracy_matches_a_torch_fp16_run(tiny):
    """The north-star tolerance (1e-3) is stated against an fp16 *reference* run.  That run cannot be produced here, but
    its noise floor can: the same network evaluated by torch in fp16 deviates from the fp32 oracle by e16.  The HIP
    engine (fp16 storage, fp32 accumulation everywhere) must be at least as close to the fp32 truth."""
    import copy
    rng = np.random.default_rng(11)
    u = tiny["cfgs"][0]
    T, h, w = 4, 8, 8
    x = h16(rng.standard_normal((T, u.in_channels, h, w)))
    emb = h16(rng.standard_normal((T, u.cross_attention_dim)))
    ts = 0.25 * np.log(12.0)
    ids = torch.tensor([[7.0, 127.0, 0.02]])
    with torch.no_grad():
        ref = tiny["unet"](torch.from_numpy(x)[None], torch.tensor(ts), torch.from_numpy(emb)[None], ids)[0].numpy()
        m16 = copy.deepcopy(tiny["unet"]).half()
        t16 = m16(torch.from_numpy(x)[None].half(), torch.tensor(ts), torch.from_numpy(emb)[None].half(), ids.half())[0].float().numpy()
        with fp16_storage(tiny["unet"]):
            em = tiny["unet"](torch.from_numpy(x)[None], torch.tensor(ts), torch.from_numpy(emb)[None], ids)[0].numpy()
    got = tiny["eng"].unet_forward(x, ts, emb)
    e_hip, e16 = rel_err(got, ref), rel_err(t16, ref)
    report("tiny UNet: |HIP - fp32|", e_hip); report("tiny UNet: |torch fp16 - fp32|", e16)
    # the quantity north_star bounds, measured directly: HIP against an fp16 run of the same network (two fp16 runs differ from each other by
    # about sqrt(2) x their distance from the fp32 result), and the fp16-storage emulation used at full size against the real .half() run
    report("tiny UNet: |HIP - torch fp16| / max", rel_err(got, t16))
    report("tiny UNet: |fp16-storage emulation - fp32|", rel_err(em, ref)); report("tiny UNet: |HIP - fp16-storage emulation| / max", rel_err(got, em))
    assert e_hip <= 1.25 * e16 + 2e-4, (e_hip, e16)
    assert rel_err(got, t16) <= 2.0 * e16 + 2e-4


def test_vae_decode_fp16_accuracy_matches_a_torch_fp16_run(tiny):
    import copy
    rng = np.random.default_rng(12)
    z = h16(rng.standard_normal((3, 4, 8, 8)) * 2)
    with torch.no_grad():
        ref = tiny["vae"].decode(torch.from_numpy(z), 3).numpy()
        t16 = copy.deepcopy(tiny["vae"]).half().decode(torch.from_numpy(z).half(), 3).float().numpy()
    got = tiny["eng"].vae_decode(z)                      # [T,H,W,3] in [0,1]
    ref01 = np.clip(ref / 2 + 0.5, 0, 1).transpose(0, 2, 3, 1)
    t01 = np.clip(t16 / 2 + 0.5, 0, 1).transpose(0, 2, 3, 1)
    e_hip, e16 = np.abs(got - ref01).max(), np.abs(t01 - ref01).max()
    report("tiny VAE decode: |HIP - fp32|", e_hip); report("tiny VAE decode: |torch fp16 - fp32|", e16)
    report("tiny VAE decode: |HIP - torch fp16| (frames in [0,1])", np.abs(got - t01).max())
    assert e_hip <= 1.25 * e16 + 5e-4, (e_hip, e16)


@pytest.mark.parametrize("T,H,W,steps,chunk", [(1, 64, 64, 1, 8), (5, 64, 128, 2, 2), (4, 128, 64, 3, 3)])
def test_pipeline_edge_cases(tiny, T, H, W, steps, chunk):
    """single frame, chunked encode/decode (temporal layers only see the chunk, as in the reference), non-square."""
    from oracle.pipeline import run_pipeline
    from unigeo_amd.pipeline import make_noise
    rng = np.random.default_rng(T * 100 + H)
    frames = (rng.uniform(0, 255, (T, H, W, 3)).astype(np.uint8)).astype(np.float32) / 255.0
    nl, na = make_noise(T, H, W, seed=T)
    res = tiny["pipe"](frames, num_inference_steps=steps, window_size=T, decode_chunk_size=chunk, noise_latents=nl, noise_aug=na)
    ref = run_pipeline(tiny["unet"], tiny["vae"], tiny["clip"], frames, torch.from_numpy(nl), torch.from_numpy(na),
                       steps=steps, chunk=chunk)
    got = res.frames[0]
    assert got.shape == ref.shape
    assert_abs(got, ref, 1.2e-2, f"tiny pipeline edge case T={T} {H}x{W} steps={steps} chunk={chunk}")


def test_frame_count_limits(tiny):
    """A 64-frame clip and a 100-frame clip (3- / 4-block temporal-attention tiles; the limit of one denoising window is 128 frames,
    upstream DepthCrafter's default window is 110) run and match the oracle; 129 frames, an empty clip and a ragged noise tensor are
    refused with a message instead of being truncated or padded."""
    from oracle.pipeline import run_pipeline
    from unigeo_amd.pipeline import make_noise
    T, H, W = 64, 64, 64
    rng = np.random.default_rng(64)
    frames = rng.uniform(0, 1, (T, H, W, 3)).astype(np.float32)
    nl, na = make_noise(T, H, W, seed=1)
    res = tiny["pipe"](frames, num_inference_steps=1, window_size=T, noise_latents=nl, noise_aug=na)
    ref = run_pipeline(tiny["unet"], tiny["vae"], tiny["clip"], frames, torch.from_numpy(nl), torch.from_numpy(na), steps=1, chunk=8)
    assert_abs(res.frames[0], ref, 1.5e-2, "tiny pipeline, 64 frames")
    T2 = 100
    f2 = rng.uniform(0, 1, (T2, H, W, 3)).astype(np.float32)
    nl3, na3 = make_noise(T2, H, W, seed=2)
    res2 = tiny["pipe"](f2, num_inference_steps=1, window_size=T2, noise_latents=nl3, noise_aug=na3)
    ref2 = run_pipeline(tiny["unet"], tiny["vae"], tiny["clip"], f2, torch.from_numpy(nl3), torch.from_numpy(na3), steps=1, chunk=8)
    assert_abs(res2.frames[0], ref2, 1.5e-2, "tiny pipeline, 100 frames")
    big = rng.uniform(0, 1, (129, H, W, 3)).astype(np.float32)
    nl2, na2 = make_noise(129, H, W, seed=1)
    with pytest.raises((RuntimeError, ValueError, NotImplementedError)):
        tiny["pipe"](big, num_inference_steps=1, window_size=129, noise_latents=nl2, noise_aug=na2)
    with pytest.raises((RuntimeError, ValueError)):
        tiny["pipe"](frames[:0], num_inference_steps=1, window_size=1, noise_latents=nl[:, :0], noise_aug=na[:0])
    with pytest.raises((RuntimeError, ValueError)):
        tiny["pipe"](frames, num_inference_steps=1, window_size=T, noise_latents=nl[:, :10], noise_aug=na)


@pytest.mark.parametrize("T,window,overlap,steps", [(10, 6, 2, 2), (9, 4, 1, 2), (7, 6, 0, 1), (11, 5, 3, 2)])
def test_latent_sliding_windows(tiny, T, window, overlap, steps):
    """Long-video mode (upstream DepthCrafter's latent sliding windows, off on the reference path; restated, unpinned): HIP vs the
    oracle's restatement on ragged window tails; window >= T must be the plain path bit for bit."""
    from oracle.pipeline import run_pipeline
    from unigeo_amd.pipeline import make_noise
    H, W = 64, 64
    rng = np.random.default_rng(T * 10 + window)
    frames = rng.uniform(0, 1, (T, H, W, 3)).astype(np.float32)
    nl, na = make_noise(T, H, W, seed=3)
    res = tiny["pipe"](frames, num_inference_steps=steps, window_size=window, overlap=overlap, noise_latents=nl, noise_aug=na)
    ref = run_pipeline(tiny["unet"], tiny["vae"], tiny["clip"], frames, torch.from_numpy(nl), torch.from_numpy(na), steps=steps, chunk=8,
                       window=window, overlap=overlap)
    assert res.frames[0].shape == ref.shape
    assert_abs(res.frames[0], ref, 1.4e-2, f"latent sliding windows T={T} window={window} overlap={overlap}")
    plain = tiny["pipe"](frames, num_inference_steps=steps, window_size=T, noise_latents=nl, noise_aug=na).frames[0]
    same = tiny["pipe"](frames, num_inference_steps=steps, window_size=T + 5, overlap=overlap, noise_latents=nl, noise_aug=na).frames[0]
    assert np.array_equal(plain, same)
    assert np.abs(plain - res.frames[0]).max() > 1e-4       # the windowed result really is a different computation


def test_full_architecture_unet_and_vae_decoder_small_clip():
    """The REAL architecture (1.52 B-parameter SVD UNet: 320/640/1280/1280 channels, 5/10/20/20 heads, 1024-d cross attention; the
    97.7 M-parameter temporal VAE) with seeded random weights on a clip small enough for the CPU oracle (3 frames, 8x16 latents):
    every full-size channel count / head count / group size goes through the HIP engine and is compared with the fp32 oracle."""
    from unigeo_amd import weights as W
    from unigeo_amd.pipeline import DepthCrafterPipelineHIP
    u, v, c = W.UNetCfg(), W.VAECfg(), W.tiny_cfgs()[2]          # full UNet + VAE; the CLIP tower is pinned elsewhere
    su, sv, sc = (W.random_state(W.unet_manifest(u), 11), W.random_state(W.vae_manifest(v), 12), W.random_state(W.clip_manifest(c), 13))
    pipe = DepthCrafterPipelineHIP.from_state(su, sv, sc, cfgs=(u, v, c), workspace_bytes=8 << 30, persist_bytes=8 << 30)
    try:
        rng = np.random.default_rng(5)
        T, h, w = 3, 8, 16
        x = h16(rng.standard_normal((T, u.in_channels, h, w)))
        emb = h16(rng.standard_normal((T, u.cross_attention_dim)))
        tstep = 0.25 * np.log(11.0)
        got = pipe.engine.unet_forward(x, tstep, emb)
        unet = oracle_unet(u, su)
        with torch.no_grad():
            ref = unet(torch.from_numpy(x)[None], torch.tensor(tstep), torch.from_numpy(emb)[None], torch.tensor([[7.0, 127.0, 0.02]]))[0].numpy()
            with fp16_storage(unet):     # fp16 run of the same network (emulated: fp16 tensors, fp32 accumulation) - the reference north_star's 1e-3 is stated against
                ref16 = unet(torch.from_numpy(x)[None], torch.tensor(tstep), torch.from_numpy(emb)[None], torch.tensor([[7.0, 127.0, 0.02]]))[0].numpy()
        del unet
        assert_close(got, ref, 3.5e-3, "full-architecture UNet forward")
        report("full-architecture UNet: |fp16-storage oracle - fp32 oracle| / max", rel_err(ref16, ref))
        report("full-architecture UNet: |HIP - fp16-storage oracle| / max (the quantity north_star's 1e-3 bounds)", rel_err(got, ref16))
        z = h16(rng.standard_normal((2, 4, 8, 8)) * 2)
        gotv = pipe.engine.vae_decode(z)
        vae = oracle_vae(v, sv)
        with torch.no_grad():
            fr = vae.decode(torch.from_numpy(z), 2)
            refv = (fr / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).numpy()
            with fp16_storage(vae):
                refv16 = (vae.decode(torch.from_numpy(z), 2) / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).numpy()
        assert_abs(gotv, refv, 4.5e-3, "full-architecture VAE decode (frames in [0,1])")
        report("full-architecture VAE decode: |fp16-storage oracle - fp32 oracle| (frames in [0,1])", np.abs(refv16 - refv).max())
        report("full-architecture VAE decode: |HIP - fp16-storage oracle| (frames in [0,1])", np.abs(gotv - refv16).max())
    finally:
        pipe.engine.close()


def test_full_architecture_clip_and_vae_encoder_small_clip():
    """CLIP ViT-H/14 (632 M parameters, 32 layers, 16 heads of 80) and the full VAE encoder with seeded random weights: HIP vs the oracle.
    The CLIP oracle itself is pinned against transformers.CLIPVisionModelWithProjection (tests/test_oracle_structure.py), so this ties the
    HIP tower to the real implementation at full size."""
    from oracle.clip import clip_preprocess
    from unigeo_amd import weights as W
    from unigeo_amd.pipeline import DepthCrafterPipelineHIP
    u, v, c = W.tiny_cfgs()[0], W.VAECfg(), W.CLIPCfg()
    su, sv, sc = (W.random_state(W.unet_manifest(u), 21), W.random_state(W.vae_manifest(v), 22), W.random_state(W.clip_manifest(c), 23))
    pipe = DepthCrafterPipelineHIP.from_state(su, sv, sc, cfgs=(u, v, c), workspace_bytes=8 << 30, persist_bytes=4 << 30)
    try:
        rng = np.random.default_rng(6)
        frames = h16(rng.uniform(0, 1, (2, 64, 128, 3)))
        got = pipe.engine.clip_embed(frames)
        clip = oracle_clip(c, sc)
        with torch.no_grad():
            ref = clip(clip_preprocess(torch.from_numpy(frames).permute(0, 3, 1, 2) * 2.0 - 1.0)).numpy()
        del clip
        assert got.shape == ref.shape == (2, 1024)
        assert_close(got, ref, 2.5e-3, "full-architecture CLIP image embedding")
        video = h16(rng.uniform(-1, 1, (2, 64, 64, 3)))
        gote = pipe.engine.vae_encode(video)
        vae = oracle_vae(v, sv)
        with torch.no_grad():
            refe = vae.encode_mode(torch.from_numpy(video).permute(0, 3, 1, 2)).numpy()
        assert_close(gote, refe, 1e-3, "full-architecture VAE encode, float32-grade (posterior mode, fp16 output)")
        pipe.engine.set_vae_encode_fp32(False)
        gote16 = pipe.engine.vae_encode(video)
        pipe.engine.set_vae_encode_fp32(True)
        assert_close(gote16, refe, 3e-3, "full-architecture VAE encode, fp16 storage")
        # full frame size of BASELINE configs[1] (one 384x512 frame: S = 3072 mid-block attention, 196608-pixel level 0)
        yy, xx = np.mgrid[0:384, 0:512].astype(np.float32)
        big = h16(np.stack([np.sin(xx / 31.0 + c) * np.cos(yy / 23.0) * 0.8 + 0.1 * rng.standard_normal((384, 512)) for c in range(3)], -1)[None])
        gotb = pipe.engine.vae_encode(big)
        with torch.no_grad():
            refb = vae.encode_mode(torch.from_numpy(big).permute(0, 3, 1, 2)).numpy()
        assert_close(gotb, refb, 1e-3, "full-size (384x512) full-architecture VAE encode, float32-grade")
        # the engine's output IS the pipeline's fp16 latent: what is left after subtracting the unavoidable half-ulp of that final
        # fp16 rounding is the error of the float32-grade interior - a few 1e-6 of the output scale, i.e. fp32 round-off
        half_ulp = np.spacing(np.abs(refb).astype(np.float16)).astype(np.float32) / 2
        interior = float(np.maximum(np.abs(gotb - refb) - half_ulp, 0).max() / np.abs(refb).max())
        report("full-size VAE encode, float32-grade: error beyond the final fp16 rounding / max|ref|", interior)
        report("full-size VAE encode, float32-grade: fraction of latents != fp16(oracle)", float((gotb != refb.astype(np.float16).astype(np.float32)).mean()))
        assert interior < 2e-5, interior
    finally:
        pipe.engine.close()


def test_full_architecture_pipeline_end_to_end():
    """The whole hot path - CLIP embed, noise-augmented VAE encode, 2 Karras-Euler steps of the 1.52 B-parameter UNet, temporal VAE
    decode, depth post-processing - at the real architecture sizes (seeded random weights) on a 2-frame 64x64 clip, against the oracle's
    run of the same pipeline with the same noise.  Frames live in [0,1]: the bound is absolute."""
    from oracle.pipeline import run_pipeline
    from unigeo_amd import weights as W
    from unigeo_amd.pipeline import DepthCrafterPipelineHIP, make_noise
    u, v, c = W.UNetCfg(), W.VAECfg(), W.CLIPCfg()
    su, sv, sc = (W.random_state(W.unet_manifest(u), 31), W.random_state(W.vae_manifest(v), 32), W.random_state(W.clip_manifest(c), 33))
    pipe = DepthCrafterPipelineHIP.from_state(su, sv, sc, cfgs=(u, v, c), workspace_bytes=8 << 30)
    try:
        T, H, Wd = 2, 64, 64
        rng = np.random.default_rng(9)
        frames = (rng.uniform(0, 255, (T, H, Wd, 3)).astype(np.uint8)).astype(np.float32) / 255.0
        nl, na = make_noise(T, H, Wd, seed=4)
        res = pipe(frames, num_inference_steps=2, window_size=T, noise_latents=nl, noise_aug=na)
        ref = run_pipeline(oracle_unet(u, su), oracle_vae(v, sv), oracle_clip(c, sc), frames, torch.from_numpy(nl), torch.from_numpy(na),
                           steps=2, chunk=8)
        assert res.frames[0].shape == ref.shape
        assert_abs(res.frames[0], ref, 6.5e-3, "full-architecture pipeline, 2 frames 64x64, 2 steps (frames in [0,1])")
    finally:
        pipe.engine.close()
