"""Oracle for classifier-free guidance (test helper): upstream DepthCrafter's guided pipeline call, restated - UNPINNED (the upstream code
is not vendored), following diffusers' ``do_classifier_free_guidance = guidance_scale > 1``:

  * the negative image embeddings are ``zeros_like(image_embeddings)``, the negative conditioning latents ``zeros_like(video_latents)``;
  * each Euler step runs the UNet on the batch [unconditional, conditional] - the same scaled latents twice, the same timestep and
    added_time_ids - and steps on ``v_u + g * (v_c - v_u)``;
  * everything else (noise, CLIP / VAE encode, scheduler, latent sliding windows, decode) is the unguided call of oracle/pipeline.py.

It is composed from the oracle's own pieces: ``GuidedUNet`` wraps ``oracle.svd_unet.UNetSpatioTemporal`` (which takes a batch dimension) as
the ``unet`` callable that ``oracle.pipeline.run_pipeline`` drives - in the plain loop and inside every window of the window loop - so the
scheduler (``oracle.scheduler.EulerKarrasVPred``) and the window bookkeeping are the oracle's, not a copy."""
import torch

from oracle.pipeline import run_pipeline


class GuidedUNet:
    """unet(x, t, emb, added) with x = cat[scale_in(latents), cond_latents] along channels ([B,T,8,h,w]); guidance_scale <= 1 is the
    plain call (no guidance), > 1 the guided combination of one batched pass over [unconditional, conditional]."""

    def __init__(self, unet, guidance_scale):
        self.unet, self.g = unet, float(guidance_scale)

    def __call__(self, x, t, emb, added):
        if self.g <= 1.0:
            return self.unet(x, t, emb, added)
        xu = x.clone()
        xu[:, :, 4:] = 0                                             # zero conditioning latents
        v = self.unet(torch.cat([xu, x], 0), t, torch.cat([torch.zeros_like(emb), emb], 0), torch.cat([added, added], 0))
        vu, vc = v.chunk(2)
        return vu + self.g * (vc - vu)


def run_pipeline_cfg(unet, vae, clip, frames_thwc, noise_latents, noise_aug, steps, guidance_scale, **kw):
    """oracle.pipeline.run_pipeline with classifier-free guidance; kw: chunk, window, overlap, return_stages ... as there."""
    return run_pipeline(GuidedUNet(unet, guidance_scale), vae, clip, frames_thwc, noise_latents, noise_aug, steps, **kw)


def run_pipeline_cfg_windows(unet, vae, clip, frames_thwc, noise_latents, noise_aug, steps, guidance_scale, window, overlap, chunk=8):
    """The windowed variant: upstream DepthCrafter's latent sliding windows (the window loop of oracle/pipeline.py) with the guided UNet
    evaluation inside every window."""
    return run_pipeline_cfg(unet, vae, clip, frames_thwc, noise_latents, noise_aug, steps, guidance_scale, chunk=chunk, window=window,
                            overlap=overlap)
