"""`guidance_rescale` (diffusers 0.27 `rescale_noise_cfg`; Lin et al., "Common Diffusion Noise Schedules and Sample Steps are
Flawed", section 3.4), restated in float64 independently of powerpaint_amd/guidance.py and csrc/guidance.hip, and the oracle
side of the pipeline tests: the denoising loops of tests/pag_cases.py with the rescale behind their guidance combine.  Shared by
tests/test_guidance_rescale.py (CPU), tests/test_guidance_rescale_kernel_gpu.py and tests/test_guidance_rescale_gpu.py.

The rule (the specification), called by the library `if do_classifier_free_guidance and guidance_rescale > 0`:
    std_text  = noise_pred_text.std(dim=[1..], keepdim=True)            per sample, torch.std: unbiased
    std_cfg   = noise_cfg.std(dim=[1..], keepdim=True)
    noise_cfg = phi * noise_cfg * (std_text / std_cfg) + (1 - phi) * noise_cfg
noise_cfg = e_u + g (e_c - e_u), with PAG e_u + g (e_c - e_u) + s_i (e_c - e_p); noise_pred_text = e_c.  Only the ratio of the two
deviations enters: the n - 1 of the unbiased estimate cancels and sums of squared deviations (SSD) are enough.
"""
import contextlib

import numpy as np
import torch

import pag_cases as PC


def combine_f64(e, segs, g, s):
    """e: [segs][B][per] -> the guided prediction [B][per], float64 (segs 2: CFG; segs 3: PAG's three-way combine)."""
    e = np.asarray(e, dtype=np.float64)
    m = e[0] + np.float64(g) * (e[1] - e[0])
    if segs == 3:
        m = m + np.float64(s) * (e[1] - e[2])
    return m


def ssd_f64(x):
    """[B][per] -> [B][1]: the sum of squared deviations from each sample's own mean."""
    x = np.asarray(x, dtype=np.float64)
    return ((x - x.mean(axis=1, keepdims=True)) ** 2).sum(axis=1, keepdims=True)


def ratio_f64(e, segs, g, s):
    """r_b = std(e_c[b]) / std(m[b]) = sqrt(SSD(e_c[b]) / SSD(m[b])), [B][1]."""
    e = np.asarray(e, dtype=np.float64)
    return np.sqrt(ssd_f64(e[1]) / ssd_f64(combine_f64(e, segs, g, s)))


def rescale_f64(e, segs, g, s, phi):
    """e: [segs][B][per] -> what the step launch takes in place of the guided prediction, [B][per] float64."""
    m = combine_f64(e, segs, g, s)
    return m * (np.float64(phi) * ratio_f64(e, segs, g, s) + (1.0 - np.float64(phi)))


def rescale_tensor(noise_cfg, noise_pred_text, phi):
    """The same rule on torch tensors [B, ...], computed in float64 and returned in the input's dtype (the oracle loops)."""
    B = noise_cfg.shape[0]
    m, c = noise_cfg.double().reshape(B, -1), noise_pred_text.double().reshape(B, -1)
    ssd = lambda x: ((x - x.mean(dim=1, keepdim=True)) ** 2).sum(dim=1, keepdim=True)      # noqa: E731
    f = phi * torch.sqrt(ssd(c) / ssd(m)) + (1.0 - phi)
    return (m * f).reshape(noise_cfg.shape).to(noise_cfg.dtype)


# ------------------------------------------------------------------------------------------------ the oracle loops
@contextlib.contextmanager
def rescaled_guidance(phi):
    """Inside: the loops of tests/pag_cases.py rescale their guided prediction (their `_guided`) against the conditional one,
    where CFG is on and phi > 0 -- the library's own condition."""
    plain = PC._guided

    def guided(noise_pred, cfg, g, s):
        m = plain(noise_pred, cfg, g, s)
        if not cfg or not phi > 0.0:
            return m
        return rescale_tensor(m, noise_pred.chunk(3)[1], phi)

    PC._guided = guided
    try:
        yield
    finally:
        PC._guided = plain


def loop_v2_rescale(unet, brushnet, scheduler, latents, conditioning_latents, prompt_embeds, prompt_embedsU, steps,
                    guidance_scale, guidance_rescale, pag_names=(), pag_scale=0.0, generator=None):
    """PC.loop_v2_pag with the rescale.  pag_names = () and pag_scale = 0: the third segment is a second conditional one and
    the combine is plain CFG."""
    with rescaled_guidance(float(guidance_rescale)):
        return PC.loop_v2_pag(unet, brushnet, scheduler, list(pag_names), latents, conditioning_latents, prompt_embeds,
                              prompt_embedsU, steps, guidance_scale, pag_scale, generator=generator)


def loop_v1_rescale(unet, scheduler, latents, mask, masked_image_latents, prompt_embeds, steps, guidance_scale,
                    guidance_rescale, pag_names=(), pag_scale=0.0, **kw):
    """PC.loop_v1_pag with the rescale (optionally a ControlNet callable, optionally the 4-channel blend)."""
    with rescaled_guidance(float(guidance_rescale)):
        return PC.loop_v1_pag(unet, scheduler, list(pag_names), latents, mask, masked_image_latents, prompt_embeds, steps,
                              guidance_scale, pag_scale, **kw)
