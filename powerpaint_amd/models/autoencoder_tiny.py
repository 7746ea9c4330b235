"""AutoencoderTiny (TAESD) on the MI355X HIP path: diffusers' `AutoencoderTiny` (`models/autoencoders/autoencoder_tiny.py`;
the `madebyollin/taesd` / `taesdxl` checkpoints), the small deterministic VAE that few-step and real-time setups put in
place of AutoencoderKL, and that previews decode with inside the denoising loop:

    vae.encode(x).latents                      (no posterior: nothing is sampled, no generator is touched)
    vae.decode(z, return_dict=False)[0]

The network is `powerpaint_amd.vae_tiny.TinyVAENet`; `load_state_dict` takes the checkpoint's key names unchanged.
"""
from types import SimpleNamespace
from typing import Optional

import torch

from .. import _lib as L
from ..vae_tiny import WIDTH, TinyVAENet, TinyVAERuntime
from ._base import Output, _VAEModel
from .autoencoder_kl import MAX_PIXELS


class AutoencoderTiny(_VAEModel):
    def __init__(self, in_channels: int = 3, out_channels: int = 3, encoder_block_out_channels=(64, 64, 64, 64),
                 decoder_block_out_channels=(64, 64, 64, 64), act_fn: str = "relu", upsample_fn: str = "nearest",
                 latent_channels: int = 4, upsampling_scaling_factor: int = 2, num_encoder_blocks=(1, 3, 3, 3),
                 num_decoder_blocks=(3, 3, 3, 1), latent_magnitude: int = 3, latent_shift: float = 0.5,
                 force_upcast: bool = False, scaling_factor: float = 1.0, shift_factor: float = 0.0, device="cuda",
                 dtype: torch.dtype = torch.bfloat16, **unused):
        name = "AutoencoderTiny"
        enc_w, dec_w = tuple(encoder_block_out_channels), tuple(decoder_block_out_channels)
        for key, widths in (("encoder_block_out_channels", enc_w), ("decoder_block_out_channels", dec_w)):
            if any(c != WIDTH for c in widths):
                raise L.PPError(f"{name}: {key}={widths} is not built (every width must be {WIDTH}: pp_conv3x3_c64)")
        if act_fn != "relu":
            raise L.PPError(f"{name}: act_fn={act_fn!r} is not built (only 'relu')")
        if upsample_fn != "nearest":
            raise L.PPError(f"{name}: upsample_fn={upsample_fn!r} is not built (only 'nearest')")
        if upsampling_scaling_factor != 2:
            raise L.PPError(f"{name}: upsampling_scaling_factor={upsampling_scaling_factor} is not built (only 2)")
        if len(enc_w) != len(num_encoder_blocks) or len(dec_w) != len(num_decoder_blocks):
            raise L.PPError(f"{name}: one width per entry of num_encoder_blocks={tuple(num_encoder_blocks)} / "
                            f"num_decoder_blocks={tuple(num_decoder_blocks)}")
        self._device = torch.device(device)
        self.net = TinyVAENet(in_channels, out_channels, latent_channels, tuple(num_encoder_blocks), tuple(num_decoder_blocks),
                              dtype=dtype)
        self._dec = TinyVAERuntime(self.net, self._device, "decode")
        self._enc = TinyVAERuntime(self.net, self._device, "encode")
        self._runtimes = (self._dec, self._enc)
        self._scale = 2 ** (len(dec_w) - 1)                  # decoder: image side / latent side
        # (diffusers registers block_out_channels = decoder_block_out_channels on top of its arguments: the pipelines compute
        # vae_scale_factor from it)
        self.config = SimpleNamespace(
            in_channels=in_channels, out_channels=out_channels, encoder_block_out_channels=enc_w,
            decoder_block_out_channels=dec_w, act_fn=act_fn, upsample_fn=upsample_fn, latent_channels=latent_channels,
            upsampling_scaling_factor=upsampling_scaling_factor, num_encoder_blocks=tuple(num_encoder_blocks),
            num_decoder_blocks=tuple(num_decoder_blocks), latent_magnitude=latent_magnitude, latent_shift=latent_shift,
            force_upcast=force_upcast, scaling_factor=scaling_factor, shift_factor=shift_factor, block_out_channels=dec_w)
        self.latent_magnitude, self.latent_shift = latent_magnitude, latent_shift

    def enable_tiling(self, *a, **k):
        raise L.PPError("AutoencoderTiny: enable_tiling is not built (tiles blend across seams: another result)")

    def enable_slicing(self, *a, **k):
        raise L.PPError("AutoencoderTiny: enable_slicing is not built (batches are chunked by MAX_PIXELS already)")

    def _max_pixels(self) -> int:
        return MAX_PIXELS

    # ------------------------------------------------------------------
    def scale_latents(self, x: torch.Tensor) -> torch.Tensor:
        """raw latents -> [0, 1]"""
        return x.div(2 * self.latent_magnitude).add(self.latent_shift).clamp(0, 1)

    def unscale_latents(self, x: torch.Tensor) -> torch.Tensor:
        """[0, 1] -> raw latents"""
        return x.sub(self.latent_shift).mul(2 * self.latent_magnitude)

    @torch.no_grad()
    def encode(self, x: torch.Tensor, return_dict: bool = True):
        self._loaded()
        B, Cc, H, W = x.shape
        if Cc != self.config.in_channels:
            raise ValueError(f"encode expects [B, {self.config.in_channels}, H, W] images, got {tuple(x.shape)}")
        x = x.to(self._device)
        parts = [self._enc.run(x[a:b])[:, :self.config.latent_channels].clone() for a, b in self._chunks(B, H * W)]
        lat = torch.cat(parts, 0) if len(parts) > 1 else parts[0]
        return Output(latents=lat) if return_dict else (lat,)

    @torch.no_grad()
    def decode(self, z: torch.Tensor, generator: Optional[torch.Generator] = None, return_dict: bool = True):
        self._loaded()
        B, Cc, h, w = z.shape
        if Cc != self.config.latent_channels:
            raise ValueError(f"decode expects [B, {self.config.latent_channels}, h, w] latents, got {tuple(z.shape)}")
        z = z.to(self._device)
        s = self._scale
        parts = [self._dec.run(z[a:b])[:, :self.config.out_channels].clone() for a, b in self._chunks(B, s * s * h * w)]
        img = torch.cat(parts, 0) if len(parts) > 1 else parts[0]
        return Output(sample=img) if return_dict else (img,)

    def forward(self, sample: torch.Tensor, return_dict: bool = True):
        """encode, quantise the latents to the 256 levels of a uint8 image (as diffusers does), decode."""
        enc = self.encode(sample).latents
        q = self.scale_latents(enc).mul_(255).round_().byte()
        return self.decode(self.unscale_latents(q / 255.0), return_dict=return_dict)

    __call__ = forward
