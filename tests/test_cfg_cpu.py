"""Classifier-free guidance, CPU side: the library exports the new entry points and the headers declare them, the guided oracle's
restatement reduces to the unguided oracle at guidance_scale = 1, and the pipeline's argument checks (stub engine, no GPU)."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ug_dc_set_guidance", "ug_unet_forward_pair")


def _declared(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return set(re.findall(r"\b(ug_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))


def test_guidance_entry_points_are_exported_and_declared():
    from unigeo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load_library()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS, s
    assert "ug_dc_set_guidance" in _declared("unigeo_hip.h")            # product boundary: the pipeline call's guidance_scale
    assert "ug_unet_forward_pair" in _declared("unigeo_hip_test.h")     # test entry point


@pytest.fixture(scope="module")
def tiny_oracle():
    from oracle_build import oracle_clip, oracle_unet, oracle_vae
    from unigeo_amd import weights as W
    u, v, c = W.tiny_cfgs()
    return (oracle_unet(u, W.random_state(W.unet_manifest(u), 1)), oracle_vae(v, W.random_state(W.vae_manifest(v), 2)),
            oracle_clip(c, W.random_state(W.clip_manifest(c), 3)))


def _clip(T, seed):
    from unigeo_amd.pipeline import make_noise
    rng = np.random.default_rng(seed)
    frames = rng.uniform(0, 1, (T, 64, 64, 3)).astype(np.float32)
    nl, na = make_noise(T, 64, 64, seed=seed)
    return frames, torch.from_numpy(nl), torch.from_numpy(na)


def test_guided_oracle_at_scale_one_is_the_unguided_oracle(tiny_oracle):
    from cfg_oracle import run_pipeline_cfg, run_pipeline_cfg_windows
    from oracle.pipeline import run_pipeline
    un, va, cl = tiny_oracle
    frames, nl, na = _clip(3, 5)
    ref = run_pipeline(un, va, cl, frames, nl, na, steps=2)
    assert np.array_equal(run_pipeline_cfg(un, va, cl, frames, nl, na, 2, 1.0), ref)
    assert np.array_equal(run_pipeline_cfg(un, va, cl, frames, nl, na, 2, 0.5), ref)       # <= 1: no guidance
    g = run_pipeline_cfg(un, va, cl, frames, nl, na, 2, 1.5)
    assert np.isfinite(g).all() and np.abs(g - ref).max() > 1e-4                            # > 1: a different computation
    frames, nl, na = _clip(7, 6)
    refw = run_pipeline(un, va, cl, frames, nl, na, steps=1, window=4, overlap=1)
    assert np.array_equal(run_pipeline_cfg_windows(un, va, cl, frames, nl, na, 1, 1.0, window=4, overlap=1), refw)


def test_guided_unet_is_the_combination_of_two_separate_passes(tiny_oracle):
    """The batched oracle evaluation equals v_u + g (v_c - v_u) of two separate UNet calls (the oracle UNet keeps batch items apart)."""
    from cfg_oracle import GuidedUNet
    un = tiny_oracle[0]
    rng = np.random.default_rng(8)
    x = torch.from_numpy(rng.standard_normal((1, 3, 8, 8, 8)).astype(np.float32))
    emb = torch.from_numpy(rng.standard_normal((1, 3, un.cfg.cross_attention_dim)).astype(np.float32))
    added = torch.tensor([[7.0, 127.0, 0.02]])
    t = torch.tensor(0.25 * np.log(3.7))
    with torch.no_grad():
        got = GuidedUNet(un, 1.3)(x, t, emb, added)
        vc = un(x, t, emb, added)
        xu = x.clone(); xu[:, :, 4:] = 0
        vu = un(xu, t, torch.zeros_like(emb), added)
    torch.testing.assert_close(got, vu + 1.3 * (vc - vu), rtol=1e-4, atol=1e-4)


class _StubEngine:
    def __init__(self):
        self.guidance, self.calls = [], 0

    def set_inputs(self, video, nl, na, K):
        self._T, self._H, self._W = video.shape[:3]

    def set_guidance(self, g):
        self.guidance.append(g)

    def run(self, steps, chunk, with_normals=False, window=0, overlap=0):
        self.calls += 1

    def get_outputs(self, frames=True, depth=True, normals=False):
        T, H, W = self._T, self._H, self._W
        return np.zeros((T, H, W, 3), np.float32), np.zeros((T, H, W), np.float32), None


def test_pipeline_guidance_argument_checks():
    from unigeo_amd.pipeline import DepthCrafterPipelineHIP, make_noise
    eng = _StubEngine()
    pipe = DepthCrafterPipelineHIP(eng, None, None, None)
    frames = np.zeros((2, 64, 64, 3), np.float32)
    nl, na = make_noise(2, 64, 64, 0)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            pipe(frames, num_inference_steps=1, guidance_scale=bad, window_size=2, noise_latents=nl, noise_aug=na)
    assert eng.calls == 0
    for g in (1.2, 1.0, 0.5, 3.0):      # set per call: a call with 1.0 after one with 1.2 is unguided again
        pipe(frames, num_inference_steps=1, guidance_scale=g, window_size=2, noise_latents=nl, noise_aug=na)
    assert eng.guidance == [1.2, 1.0, 0.5, 3.0] and eng.calls == 4
    pipe(frames, num_inference_steps=1, window_size=2, noise_latents=nl, noise_aug=na)
    assert eng.guidance[-1] == 1.0                                   # default: the reference's 1.0


def test_plugin_passes_guidance_scale_through():
    from unigeo_amd.model.depthcrafter import DepthCrafter
    seen = []
    p = DepthCrafter.__new__(DepthCrafter)
    p.num_inference_steps, p.seed, p._calls, p.device, p.guidance_scale = 1, 0, 0, "cpu", 1.2

    def pipeline(frames, **kw):
        seen.append(kw["guidance_scale"])
        T, H, W = frames.shape[:3]
        return SimpleNamespace(depth=np.ones((T, H, W), np.float32), normals=np.zeros((T, H, W, 3), np.float32))
    p.pipeline = pipeline
    from unigeo_amd.synthetic import synthetic_clip
    p.forward(synthetic_clip(2, 64, 64, seed=1))
    assert seen == [1.2]
