"""`guidance_rescale` on the HIP path: diffusers' `rescale_noise_cfg` (0.27; Lin et al., "Common Diffusion Noise Schedules and
Sample Steps are Flawed", section 3.4).

With classifier-free guidance on, the guided prediction of every sample is pulled back to the standard deviation of that
sample's conditional prediction:

    noise_cfg <- phi * noise_cfg * (std(e_c) / std(noise_cfg)) + (1 - phi) * noise_cfg         (phi = guidance_rescale)

pp_cfg_rescale does it in one launch in front of the scheduler's step launch (csrc/guidance.hip; DESIGN.md, "guidance_rescale").
Without CFG (`guidance_scale <= 1`, or a guidance-embedded UNet with `time_cond_proj_dim`) the argument has no effect, as in
the library.  Everything in this file is host code without a device: the argument check and the rule as tensor code for a
duck-typed scheduler.
"""
import math

import torch


def check_guidance_rescale(guidance_rescale) -> float:
    """The pipelines' check: a finite number >= 0 (0 = off).  The library has no such check; a negative or non-finite phi has
    no meaning in the rule above."""
    try:
        v = float(guidance_rescale)
    except (TypeError, ValueError):
        raise ValueError(f"`guidance_rescale` has to be a number but is {type(guidance_rescale).__name__}") from None
    if not math.isfinite(v) or v < 0.0:
        raise ValueError(f"`guidance_rescale` has to be a finite number >= 0 but is {guidance_rescale}")
    return v


def rescale_noise_cfg(noise_cfg: torch.Tensor, noise_pred_text: torch.Tensor, guidance_rescale: float) -> torch.Tensor:
    """`rescale_noise_cfg` as tensor code (the loop of a duck-typed scheduler), per sample over all other dimensions."""
    dims = list(range(1, noise_pred_text.ndim))
    std_text = noise_pred_text.std(dim=dims, keepdim=True)
    std_cfg = noise_cfg.std(dim=dims, keepdim=True)
    rescaled = noise_cfg * (std_text / std_cfg)
    return guidance_rescale * rescaled + (1 - guidance_rescale) * noise_cfg
