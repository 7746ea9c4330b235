"""AsymmetricAutoencoderKL on the MI355X HIP path: the VAE with a mask-conditioned decoder (diffusers 0.27
`models/autoencoders/autoencoder_asym_kl.py`; Zhu et al., arXiv:2306.04632 -- the `asymmetric-autoencoder-kl-x-1-5` / `x-2`
checkpoints) that the reference's image-conditioned pipelines accept as `vae` and branch on when they decode
(pipeline_PowerPaint.py:194,1043-1051; pipeline_PowerPaint_ControlNet.py:1317-1325):

    vae.decode(latents / scaling_factor, return_dict=False, image=init_image, mask=mask)[0]

The network is `powerpaint_amd.vae_asym.AsymVAENet`; `load_state_dict` takes the checkpoint's key names unchanged.
"""
from types import SimpleNamespace
from typing import Optional

import torch

from .. import _lib as L
from ..vae_asym import BLOCK_DOWN, BLOCK_UP, AsymVAENet, AsymVAERuntime
from ._base import Output
from .autoencoder_kl import _KLModel

MAX_BYTES = (1 << 31) - 1      # every tensor of a launch plan stays below 2^31 bytes


class AsymmetricAutoencoderKL(_KLModel):
    def __init__(self, in_channels: int = 3, out_channels: int = 3, down_block_types=(BLOCK_DOWN,),
                 down_block_out_channels=(64,), layers_per_down_block: int = 1, up_block_types=(BLOCK_UP,),
                 up_block_out_channels=(64,), layers_per_up_block: int = 1, act_fn: str = "silu", latent_channels: int = 4,
                 norm_num_groups: int = 32, sample_size: int = 32, scaling_factor: float = 0.18215, device="cuda",
                 dtype: torch.dtype = torch.bfloat16, **unused):
        name = "AsymmetricAutoencoderKL"
        bad = [t for t in down_block_types if t != BLOCK_DOWN] + [t for t in up_block_types if t != BLOCK_UP]
        if bad:
            raise L.PPError(f"{name}: block type {bad[0]!r} is not built (only {BLOCK_DOWN} / {BLOCK_UP}, the SD-1.5 layout)")
        if act_fn != "silu":
            raise L.PPError(f"{name}: act_fn={act_fn!r} is not built (only 'silu')")
        if len(down_block_types) != len(down_block_out_channels) or len(up_block_types) != len(up_block_out_channels):
            raise L.PPError(f"{name}: one block type per entry of down_block_out_channels / up_block_out_channels")
        self._device = torch.device(device)
        self.net = AsymVAENet(in_channels, out_channels, latent_channels, down_block_out_channels, layers_per_down_block,
                              up_block_out_channels, layers_per_up_block, norm_num_groups, dtype=dtype)
        why = self.net.condition_mismatch()
        if why:                                                # (diffusers: a KeyError in the first conditioned forward)
            raise L.PPError(f"{name}: {why}")
        self._dec = AsymVAERuntime(self.net, self._device, "decode")
        self._dec_cond = AsymVAERuntime(self.net, self._device, "decode_cond")
        self._enc = AsymVAERuntime(self.net, self._device, "encode")
        self._runtimes = (self._dec, self._dec_cond, self._enc)
        self._scale = 2 ** (len(up_block_out_channels) - 1)             # decoder: image side / latent side
        self._enc_scale = 2 ** (len(down_block_out_channels) - 1)      # encoder (its own block count, as in diffusers)
        # (diffusers registers block_out_channels = up_block_out_channels and force_upcast = False on top of its arguments)
        self.config = SimpleNamespace(
            in_channels=in_channels, out_channels=out_channels, down_block_types=tuple(down_block_types),
            down_block_out_channels=tuple(down_block_out_channels), layers_per_down_block=layers_per_down_block,
            up_block_types=tuple(up_block_types), up_block_out_channels=tuple(up_block_out_channels),
            layers_per_up_block=layers_per_up_block, act_fn=act_fn, latent_channels=latent_channels,
            norm_num_groups=norm_num_groups, sample_size=sample_size, scaling_factor=scaling_factor,
            block_out_channels=tuple(up_block_out_channels), force_upcast=False)

    def _max_pixels(self) -> int:
        # the widest full-resolution tensor: layer 1 of the condition encoder, 2 up[0] channels of 2 bytes
        return min(1 << 21, MAX_BYTES // (4 * self.net.up[0]))

    @torch.no_grad()
    def decode(self, z: torch.Tensor, generator=None, image: Optional[torch.Tensor] = None,
               mask: Optional[torch.Tensor] = None, return_dict: bool = True):
        """image [B | 1, out_channels, H, W] and mask [B | 1, 1, H, W] (any float values; 1 = take the decoded sample, 0 = take
        the image's features), H x W the decoded size: the conditioned decode.  With either None nothing is blended."""
        self._loaded()
        B, Cc, h, w = z.shape
        s = self._scale
        if Cc != self.config.latent_channels:
            raise ValueError(f"decode expects [B, {self.config.latent_channels}, h, w] latents, got {tuple(z.shape)}")
        cond = image is not None and mask is not None
        if cond:
            if tuple(image.shape[1:]) != (self.config.out_channels, s * h, s * w) or image.shape[0] not in (1, B):
                raise ValueError(f"decode: image must be [{B} | 1, {self.config.out_channels}, {s * h}, {s * w}] (sizes "
                                 f"divisible by {s}), got {tuple(image.shape)}")
            if tuple(mask.shape[1:]) != (1, s * h, s * w) or mask.shape[0] not in (1, B):
                raise ValueError(f"decode: mask must be [{B} | 1, 1, {s * h}, {s * w}], got {tuple(mask.shape)}")
        pick = lambda t, a, b: t if t.shape[0] == 1 else t[a:b]      # noqa: E731
        parts = []
        for a, b in self._chunks(B, s * s * h * w):
            if cond:
                out = self._dec_cond.run(z[a:b], pick(image, a, b), pick(mask, a, b))
            else:
                out = self._dec.run(z[a:b])
            parts.append(out[:, :self.config.out_channels].clone())
        img = torch.cat(parts, 0) if len(parts) > 1 else parts[0]
        return Output(sample=img) if return_dict else (img,)

    def forward(self, sample: torch.Tensor, mask: Optional[torch.Tensor] = None, sample_posterior: bool = False,
                return_dict: bool = True, generator: Optional[torch.Generator] = None):
        dist = self.encode(sample).latent_dist
        z = dist.sample(generator=generator) if sample_posterior else dist.mode()
        return self.decode(z, generator=generator, image=sample, mask=mask, return_dict=return_dict)

    __call__ = forward
