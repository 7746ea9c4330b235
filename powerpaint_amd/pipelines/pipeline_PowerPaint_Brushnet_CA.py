"""ppt-v2 (BrushNet) pipeline on the MI355X HIP path: drop-in for
/root/reference/powerpaint/pipelines/pipeline_PowerPaint_Brushnet_CA.py:1026-1497
(`StableDiffusionPowerPaintBrushNetPipeline.__call__`).

Additive keyword extension for synthetic / VAE-free operation: `conditioning_latents=` ([B or 2B, 5, h, w]:
VAE latents of the masked image * scaling_factor concatenated with the latent-resolution mask, i.e. the tensor the
reference builds at :1338-1345) and `prompt_embedsU=` / `negative_prompt_embedsU=` for the UNet's plain prompt.
"""
import inspect
from typing import Any, Callable, Dict, List, Optional, Union

import torch

from .. import _lib as L
from .. import guidance as GDM
from .. import ip_adapter as IPA
from .. import pag as PAGM
from ._base import PipelineBase, hip_mask_prep, randn_tensor, retrieve_latents
from ._loop import DenoiseLoop
from .image_processor import VaeImageProcessor


def retrieve_timesteps(scheduler, num_inference_steps=None, device=None, timesteps=None, **kwargs):
    """pipeline_PowerPaint_Brushnet_CA.py:87-128: a custom `timesteps` list goes to schedulers whose `set_timesteps`
    takes one -- of this package LCMScheduler, which validates it (descending integers below num_train_timesteps) -- and is
    a ValueError for the others, as in diffusers 0.27 (DDIM / DPM-Solver++ / PNDM / UniPC take a step count only)."""
    if timesteps is not None:
        if "timesteps" not in set(inspect.signature(scheduler.set_timesteps).parameters.keys()):
            raise ValueError(f"The current scheduler class {scheduler.__class__}'s `set_timesteps` does not support custom"
                             f" timestep schedules. Please check whether you are using the correct scheduler.")
        scheduler.set_timesteps(timesteps=timesteps, device=device, **kwargs)
        return scheduler.timesteps, len(scheduler.timesteps)
    scheduler.set_timesteps(num_inference_steps, device=device, **kwargs)
    return scheduler.timesteps, num_inference_steps


class StableDiffusionPowerPaintBrushNetPipeline(PipelineBase):
    _callback_tensor_inputs = ["latents", "prompt_embeds", "negative_prompt_embeds"]     # pipeline_PowerPaint_Brushnet_CA.py:177

    def __init__(self, vae=None, text_encoder=None, text_encoder_brushnet=None, tokenizer=None, unet=None,
                 brushnet=None, scheduler=None, safety_checker=None, feature_extractor=None, image_encoder=None,
                 requires_safety_checker: bool = False, pag_applied_layers=None):
        self.register_modules(vae=vae, text_encoder=text_encoder, text_encoder_brushnet=text_encoder_brushnet,
                              tokenizer=tokenizer, unet=unet, brushnet=brushnet, scheduler=scheduler,
                              safety_checker=safety_checker, feature_extractor=feature_extractor,
                              image_encoder=image_encoder)
        self.vae_scale_factor = 2 ** (len(vae.config.block_out_channels) - 1) if vae is not None else 8
        self.image_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor) if vae is not None else None
        self._loop = None
        self.use_graph = True
        if pag_applied_layers is not None:
            self.set_pag_applied_layers(pag_applied_layers)

    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def clip_skip(self):
        """pipeline_PowerPaint_Brushnet_CA.py:1005-1007,1227: `__call__` records its `clip_skip` argument here and, like the
        reference, does NOT pass it on to `encode_prompt` (:1268-1277) -- only a direct `encode_prompt(clip_skip=k)` call
        selects an earlier hidden state."""
        return getattr(self, "_clip_skip", None)

    @property
    def do_classifier_free_guidance(self):
        return self._guidance_scale > 1 and self.unet.config.time_cond_proj_dim is None

    def get_guidance_scale_embedding(self, w, embedding_dim=512, dtype=torch.float32):
        """pipeline_PowerPaint_Brushnet_CA.py:973-999: the sinusoidal embedding [len(w), embedding_dim] of 1000 w that a
        guidance-embedded (LCM-distilled) UNet takes as `timestep_cond` -- sines then cosines over half_dim frequencies
        exp(-k ln(10000) / (half_dim - 1)), one zero column behind them when embedding_dim is odd."""
        if w.dim() != 1:
            raise ValueError(f"w must be one-dimensional, got shape {tuple(w.shape)}")
        half_dim = embedding_dim // 2
        rate = torch.log(torch.tensor(10000.0)) / (half_dim - 1)
        freqs = torch.exp(torch.arange(half_dim, dtype=dtype) * -rate)
        arg = (w * 1000.0).to(dtype)[:, None] * freqs[None, :]
        emb = torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)
        if embedding_dim % 2 == 1:
            emb = torch.nn.functional.pad(emb, (0, 1))
        return emb

    def encode_prompt(self, prompt, device, num_images_per_prompt, do_cfg, negative_prompt=None, prompt_embeds=None,
                      negative_prompt_embeds=None, lora_scale=None, clip_skip=None):
        """pipeline_PowerPaint_Brushnet_CA.py:442-629 (plain prompt for the UNet); returns cat([neg, pos])."""
        if prompt_embeds is None:
            if self.text_encoder is None:
                raise ValueError("no text encoder registered: pass prompt_embedsU / negative_prompt_embedsU")
            if clip_skip is None:
                prompt_embeds = self._text_embeds(self.text_encoder, prompt, device)
            else:
                # :537-552 -- the hidden state `clip_skip` layers before the last, then the tower's final LayerNorm.
                # (Only a direct `encode_prompt(clip_skip=...)` call gets here: the reference's `__call__` stores its
                # `clip_skip` argument in `self._clip_skip` (:1227) and never hands it to `encode_prompt` (:1268-1277),
                # and this `__call__` does the same.)
                tok = self.tokenizer
                ids = tok(prompt, padding="max_length", max_length=tok.model_max_length, truncation=True,
                          return_tensors="pt").input_ids
                out = self.text_encoder(ids.to(device), output_hidden_states=True)
                prompt_embeds = self.text_encoder.text_model.final_layer_norm(out[-1][-(clip_skip + 1)])
        bs, seq, _ = prompt_embeds.shape
        prompt_embeds = prompt_embeds.to(device).repeat(1, num_images_per_prompt, 1).view(bs * num_images_per_prompt, seq, -1)
        if do_cfg:
            if negative_prompt_embeds is None:
                if self.text_encoder is None:
                    raise ValueError("classifier-free guidance needs negative_prompt_embedsU")
                neg = negative_prompt if negative_prompt is not None else [""] * bs
                if isinstance(neg, str):
                    neg = [neg] * bs
                negative_prompt_embeds = self._text_embeds(self.text_encoder, neg, device)
            negative_prompt_embeds = negative_prompt_embeds.to(device).repeat(1, num_images_per_prompt, 1).view(
                bs * num_images_per_prompt, seq, -1)
            prompt_embeds = torch.cat([negative_prompt_embeds, prompt_embeds])
        return prompt_embeds

    # ------------------------------------------------------------------ IP-Adapter (DESIGN.md "IP-Adapter")
    def load_ip_adapter(self, pretrained_model_name_or_path_or_dict, subfolder=None, weight_name=None,
                        image_encoder_folder=None, **kwargs):
        """diffusers' `IPAdapterMixin.load_ip_adapter` for local files and state dicts (nothing is downloaded): a dict
        {"image_proj": {...}, "ip_adapter": {...}}, a .bin holding one, a .safetensors with `image_proj.` / `ip_adapter.` key
        prefixes, a folder plus `weight_name` (and `subfolder`) -- or a list of those for several adapters (`subfolder` /
        `weight_name` then a value or one per adapter).  Base adapters (Linear + LayerNorm projection of the pooled image
        embeds, [B, n, D] per call) and Plus adapters (the Resampler over the tower's `hidden_states[-2]`, [B, n, S, E] per
        call, 16 tokens per image) load, alone or mixed in one list; FaceID and full-face files are refused by name
        (powerpaint_amd.ip_adapter.check_ip_adapter, which also states the index order of the cross-attentions).
        `image_encoder_folder` (default None: no image encoder is loaded) names the CLIP vision tower's folder as diffusers
        resolves it -- a name without "/" lies under `subfolder` of the model path, anything else is relative to the model
        path -- and needs a local-path source: the HIP `CLIPVisionModelWithProjection` is loaded from it into
        `pipe.image_encoder` unless one is registered already, and a default `CLIPImageProcessor` becomes
        `pipe.feature_extractor` unless one is.  With a state-dict source there is no path to resolve it against (diffusers
        raises there too).  Without it, register a duck-typed `image_encoder` and `feature_extractor` yourself, or pass
        `ip_adapter_image_embeds`."""
        if kwargs.get("ip_adapter_masks") is not None:
            raise L.PPError("load_ip_adapter takes no ip_adapter_masks (diffusers' does not either): hand them to the call, "
                            "pipe(..., cross_attention_kwargs={\"ip_adapter_masks\": IPAdapterMaskProcessor().preprocess(...)})")
        srcs = pretrained_model_name_or_path_or_dict
        srcs = list(srcs) if isinstance(srcs, (list, tuple)) else [srcs]
        if image_encoder_folder is not None:
            import os
            src = srcs[0]
            if isinstance(src, dict) or not os.path.isdir(str(src)):
                raise L.PPError("load_ip_adapter: image_encoder_folder needs a local model folder to be resolved against; a state "
                                "dict or a file has none: pass image_encoder_folder=None and register pipe.image_encoder / "
                                "pipe.feature_extractor yourself")
            sub = subfolder[0] if isinstance(subfolder, (list, tuple)) else subfolder
            folder = str(image_encoder_folder)
            folder = os.path.join(str(src), sub or "", folder) if folder.count("/") == 0 else os.path.join(str(src), folder)
            if not os.path.isdir(folder):
                raise L.PPError(f"load_ip_adapter: image_encoder_folder {folder} does not exist (nothing is downloaded)")
            encoder_folder = folder
        else:
            encoder_folder = None

        def per(v, what):
            v = list(v) if isinstance(v, (list, tuple)) else [v] * len(srcs)
            if len(v) != len(srcs):
                raise ValueError(f"`{what}` must have the same length as the number of adapters ({len(srcs)})")
            return v

        sds = [IPA.read_ip_adapter(s_, sf, wn) for s_, sf, wn in zip(srcs, per(subfolder, "subfolder"),
                                                                     per(weight_name, "weight_name"))]
        self.unet._load_ip_adapter_weights(sds)
        if encoder_folder is not None:
            if self.image_encoder is None:
                from ..models import CLIPVisionModelWithProjection
                enc = CLIPVisionModelWithProjection.from_pretrained(encoder_folder, device=self.unet.device)
                self.image_encoder = self._modules["image_encoder"] = enc
            if self.feature_extractor is None:
                from .image_processor import CLIPImageProcessor
                self.feature_extractor = self._modules["feature_extractor"] = CLIPImageProcessor()

    def set_ip_adapter_scale(self, scale):
        self.unet.set_ip_adapter_scale(scale)

    def unload_ip_adapter(self):
        """diffusers' `unload_ip_adapter`: the UNet of before `load_ip_adapter` (the image encoder and feature
        extractor stay registered, whether `load_ip_adapter` loaded them or the caller brought them)."""
        self.unet._unload_ip_adapter()

    def encode_image(self, image, device, num_images_per_prompt, output_hidden_states=None):
        """pipeline_PowerPaint_Brushnet_CA.py:632-654 through the registered (duck-typed) `image_encoder` /
        `feature_extractor`; the unconditional embeds of a base adapter are zeros.  output_hidden_states (IP-Adapter Plus,
        :639-648): the encoder's `hidden_states[-2]` [B, S, E] of the image and of the ZERO image (its hidden states, not
        zeros); each is copied by `repeat_interleave` before the next encoder call (the HIP tower's hidden states live in
        buffers it writes again).  Hidden states serve a Plus adapter only: while none is loaded the request is refused, as an
        image prompt without an adapter is -- never a tensor that nothing on the HIP path would take."""
        if self.image_encoder is None:
            raise ValueError("`ip_adapter_image` needs an `image_encoder` registered on the pipeline (none is): load one with "
                             "load_ip_adapter(<folder>, image_encoder_folder=...), register a "
                             "powerpaint_amd.models.CLIPVisionModelWithProjection, or pass `ip_adapter_image_embeds`")
        if output_hidden_states:
            layers = getattr(getattr(self.unet, "encoder_hid_proj", None), "image_projection_layers", None) or ()
            if not any(isinstance(m, IPA.IPAdapterPlusImageProjection) for m in layers):
                raise L.PPError("encode_image(output_hidden_states=True) serves IP-Adapter Plus, and no Plus adapter is loaded "
                                "(load_ip_adapter with a Plus file first; a base adapter takes the pooled image_embeds)")
        dtype = next(self.image_encoder.parameters()).dtype
        if not isinstance(image, torch.Tensor):
            if self.feature_extractor is None:
                raise ValueError("`ip_adapter_image` that is not a tensor needs a `feature_extractor` registered on the pipeline")
            image = self.feature_extractor(image, return_tensors="pt").pixel_values
        image = image.to(device=device, dtype=dtype)
        if output_hidden_states:
            hs = self.image_encoder(image, output_hidden_states=True).hidden_states[-2]
            hs = hs.repeat_interleave(num_images_per_prompt, dim=0)
            uncond = self.image_encoder(torch.zeros_like(image), output_hidden_states=True).hidden_states[-2]
            uncond = uncond.repeat_interleave(num_images_per_prompt, dim=0)
            return hs, uncond
        image_embeds = self.image_encoder(image).image_embeds
        image_embeds = image_embeds.repeat_interleave(num_images_per_prompt, dim=0)
        return image_embeds, torch.zeros_like(image_embeds)

    def prepare_ip_adapter_image_embeds(self, ip_adapter_image, ip_adapter_image_embeds, device, num_images_per_prompt,
                                        do_classifier_free_guidance):
        """pipeline_PowerPaint_Brushnet_CA.py:657-706: one [B, n, D] (base) or [B, n, S, E] (Plus) tensor per adapter, under CFG the negative embeds in the
        first half of the batch (precomputed embeds carry them there already and are `chunk(2)`ed for the repeat)."""
        layers = getattr(getattr(self.unet, "encoder_hid_proj", None), "image_projection_layers", None)
        if layers is None:
            raise ValueError("an IP-Adapter image prompt was given but no IP-Adapter is loaded: call `load_ip_adapter` first "
                             "(the prompt is never silently dropped)")
        out = []
        if ip_adapter_image_embeds is None:
            if not isinstance(ip_adapter_image, list):
                ip_adapter_image = [ip_adapter_image]
            if len(ip_adapter_image) != len(layers):
                raise ValueError(f"`ip_adapter_image` must have same length as the number of IP Adapters. Got "
                                 f"{len(ip_adapter_image)} images and {len(layers)} IP Adapters.")
            for img, layer in zip(ip_adapter_image, layers):
                pos, neg = self.encode_image(img, device, 1, not isinstance(layer, IPA.ImageProjection))
                pos = torch.stack([pos] * num_images_per_prompt, dim=0)
                neg = torch.stack([neg] * num_images_per_prompt, dim=0)
                out.append(torch.cat([neg, pos]).to(device) if do_classifier_free_guidance else pos)
        else:
            for e in ip_adapter_image_embeds:
                ones = [1] * (e.dim() - 1)
                if do_classifier_free_guidance:
                    neg, pos = e.chunk(2)
                    e = torch.cat([neg.repeat(num_images_per_prompt, *ones), pos.repeat(num_images_per_prompt, *ones)])
                else:
                    e = e.repeat(num_images_per_prompt, *ones)
                out.append(e)
        return out

    def check_inputs(self, ip_adapter_image=None, ip_adapter_image_embeds=None, guidance_rescale=0.0):
        """What this `__call__` checks before anything runs: the IP-Adapter branches of the reference's `check_inputs`, and
        `guidance_rescale` (no counterpart there): a finite number >= 0."""
        self._check_ip_inputs(ip_adapter_image, ip_adapter_image_embeds)
        GDM.check_guidance_rescale(guidance_rescale)

    @staticmethod
    def _check_ip_inputs(ip_adapter_image, ip_adapter_image_embeds):
        """The IP-Adapter branches of `check_inputs`, pipeline_PowerPaint_Brushnet_CA.py:853-866."""
        if ip_adapter_image is not None and ip_adapter_image_embeds is not None:
            raise ValueError("Provide either `ip_adapter_image` or `ip_adapter_image_embeds`. Cannot leave both "
                             "`ip_adapter_image` and `ip_adapter_image_embeds` defined.")
        if ip_adapter_image_embeds is not None:
            if not isinstance(ip_adapter_image_embeds, list):
                raise ValueError(f"`ip_adapter_image_embeds` has to be of type `list` but is {type(ip_adapter_image_embeds)}")
            elif ip_adapter_image_embeds[0].ndim not in [3, 4]:
                raise ValueError(f"`ip_adapter_image_embeds` has to be a list of 3D or 4D tensors but is "
                                 f"{ip_adapter_image_embeds[0].ndim}D")

    @torch.no_grad()
    def __call__(self, promptA: Union[str, List[str]] = None, promptB: Union[str, List[str]] = None,
                 promptU: Union[str, List[str]] = None, tradoff: float = 1.0, tradoff_nag: float = 1.0, image=None,
                 mask=None, height: Optional[int] = None, width: Optional[int] = None, num_inference_steps: int = 50,
                 timesteps: List[int] = None, guidance_scale: float = 7.5, negative_promptA=None,
                 negative_promptB=None, negative_promptU=None, num_images_per_prompt: Optional[int] = 1,
                 eta: float = 0.0, generator=None, latents: Optional[torch.FloatTensor] = None,
                 prompt_embeds: Optional[torch.FloatTensor] = None,
                 negative_prompt_embeds: Optional[torch.FloatTensor] = None, ip_adapter_image=None,
                 ip_adapter_image_embeds=None, output_type: Optional[str] = "pil", return_dict: bool = True,
                 cross_attention_kwargs: Optional[Dict[str, Any]] = None,
                 brushnet_conditioning_scale: Union[float, List[float]] = 1.0, guess_mode: bool = False,
                 control_guidance_start: Union[float, List[float]] = 0.0,
                 control_guidance_end: Union[float, List[float]] = 1.0, clip_skip: Optional[int] = None,
                 callback_on_step_end: Optional[Callable[[int, int, Dict], None]] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"],
                 conditioning_latents: Optional[torch.FloatTensor] = None,
                 prompt_embedsU: Optional[torch.FloatTensor] = None,
                 negative_prompt_embedsU: Optional[torch.FloatTensor] = None, pag_scale: float = 0.0,
                 pag_adaptive_scale: float = 0.0, guidance_rescale: float = 0.0, **kwargs):
        callback = kwargs.pop("callback", None)
        callback_steps = kwargs.pop("callback_steps", 1)
        self.check_inputs(ip_adapter_image, ip_adapter_image_embeds, guidance_rescale)
        # `cross_attention_kwargs` reaches the UNet only (:1430-1441): its `ip_adapter_masks` confine each adapter's image
        # prompt to a region (checked here, before anything runs; never dropped)
        ip_adapter_masks = (cross_attention_kwargs or {}).get("ip_adapter_masks")
        if ip_adapter_masks is not None:
            self.unet._check_ip_masks(ip_adapter_masks)
            if ip_adapter_image is None and ip_adapter_image_embeds is None:
                raise ValueError("`ip_adapter_masks` confine an image prompt: pass `ip_adapter_image` or "
                                 "`ip_adapter_image_embeds` with them")
        if isinstance(control_guidance_start, list):
            control_guidance_start = control_guidance_start[0]
        if isinstance(control_guidance_end, list):
            control_guidance_end = control_guidance_end[0]
        if isinstance(brushnet_conditioning_scale, list):
            brushnet_conditioning_scale = brushnet_conditioning_scale[0]
        prompt = promptA
        if prompt is not None and prompt_embeds is not None:
            raise ValueError("Cannot forward both `prompt` and `prompt_embeds`.")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`.")
        self._guidance_scale = guidance_scale
        self._clip_skip = clip_skip                      # (:1227; recorded, not applied -- see the property)
        if prompt is not None and isinstance(prompt, str):
            batch_size = 1
        elif prompt is not None and isinstance(prompt, list):
            batch_size = len(prompt)
        else:
            batch_size = prompt_embeds.shape[0]
        device = self._execution_device
        do_cfg = self.do_classifier_free_guidance
        lora_scale = self._merge_lora(cross_attention_kwargs)       # adapters folded into the weights before the loop
        prompt_embeds = self._encode_prompt(promptA, promptB, tradoff, device, num_images_per_prompt, do_cfg,
                                            negative_promptA, negative_promptB, tradoff_nag,
                                            prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds,
                                            text_encoder=self.text_encoder_brushnet)
        prompt_embedsU = self.encode_prompt(promptU, device, num_images_per_prompt, do_cfg, negative_promptU,
                                            prompt_embeds=prompt_embedsU, negative_prompt_embeds=negative_prompt_embedsU,
                                            lora_scale=lora_scale)
        # :1279-1290 -- the image prompt (per call: no memo covers it); :1363-1366 -- for the UNet only
        added_cond_kwargs = None
        if ip_adapter_image is not None or ip_adapter_image_embeds is not None:
            added_cond_kwargs = {"image_embeds": self.prepare_ip_adapter_image_embeds(
                ip_adapter_image, ip_adapter_image_embeds, device, batch_size * num_images_per_prompt, do_cfg)}
        nb = batch_size * num_images_per_prompt
        # 4./6.1 conditioning latents: [VAE latents of the masked image | latent-resolution keep-mask]
        if conditioning_latents is None:
            ip = getattr(self, "image_processor", None)
            if ip is None or self.vae is None:
                raise ValueError("no VAE / image processor registered: pass conditioning_latents")
            img = ip.preprocess(image, height=height, width=width).to(device=device, dtype=torch.float32)
            msk = ip.preprocess(mask, height=height, width=width).to(device=device, dtype=torch.float32)
            img = img.repeat_interleave(nb // img.shape[0], dim=0)
            msk = msk.repeat_interleave(nb // msk.shape[0], dim=0)
            if do_cfg and not guess_mode:   # prepare_image (:949-950) duplicates BEFORE the VAE: the two CFG halves get
                img, msk = torch.cat([img] * 2), torch.cat([msk] * 2)   # their own posterior samples (the RNG advances 2x)
            B0, C0, H0, W0 = msk.shape
            original_mask = hip_mask_prep(3, msk, None, (B0, 1, H0, W0), B0, C0, H0, W0)   # (mask.sum(1) < 0)  :1312
            height, width = img.shape[-2:]
            # 6. latents are drawn BEFORE the conditioning posterior is sampled (:1323 precedes :1338)
            if latents is None:
                vs = getattr(self, "vae_scale_factor", 8)
                latents = randn_tensor((nb, self.unet.config.in_channels, height // vs, width // vs), generator=generator,
                                       device=device, dtype=self._noise_dtype(prompt_embeds))
            cl = retrieve_latents(self.vae.encode(img.to(next(iter(self.vae.parameters())).dtype))) * \
                self.vae.config.scaling_factor                                               # :1338-1341
            hl, wl = cl.shape[-2:]
            ml = hip_mask_prep(2, original_mask, None, (B0, 1, hl, wl), B0, 1, H0, W0, hl, wl)  # nearest  :1342-1344
            conditioning_latents = torch.cat([cl.float(), ml], 1)                            # :1345
        conditioning_latents = conditioning_latents.to(device)
        # (an un-duplicated tensor stays so: the loop copies it to both CFG halves itself, without comparing them)
        if do_cfg and guess_mode and conditioning_latents.shape[0] != nb:
            raise ValueError("guess_mode runs BrushNet on the conditional half only: conditioning_latents must have "
                             f"batch {nb}, got {conditioning_latents.shape[0]}")
        h, w = conditioning_latents.shape[-2:]
        timesteps, num_inference_steps = retrieve_timesteps(self.scheduler, num_inference_steps, device, timesteps)
        self._num_timesteps = len(timesteps)
        shape = (nb, self.unet.config.in_channels, h, w)
        if latents is None:
            latents = randn_tensor(shape, generator=generator, device=device, dtype=self._noise_dtype(prompt_embeds))
        latents = latents.to(device=device, dtype=torch.float32) * self.scheduler.init_noise_sigma
        # 6.5 (:1351-1357) a guidance-embedded UNet: the guidance scale enters through the time embedding, not through CFG.
        # Built on the host and rounded to the dtype the reference's latents have (`.to(dtype=latents.dtype)`)
        timestep_cond = None
        if self.unet.config.time_cond_proj_dim is not None:
            gs = torch.tensor(self.guidance_scale - 1).repeat(nb)
            timestep_cond = self.get_guidance_scale_embedding(gs, embedding_dim=self.unet.config.time_cond_proj_dim).to(
                dtype=self._noise_dtype(prompt_embeds))
        n = len(timesteps)
        keep = [1.0 - float(i / n < control_guidance_start or (i + 1) / n > control_guidance_end) for i in range(n)]
        scales = [brushnet_conditioning_scale * k for k in keep]                              # :1370-1376,1405-1409
        if self._loop is None or self._loop.scheduler is not self.scheduler or self._loop.unet is not self.unet or \
                self._loop.side is not self.brushnet:        # (a replaced component must not keep driving the old one)
            self._loop = DenoiseLoop(self.unet, self.scheduler, side=self.brushnet, side_kind="brushnet")
        self._loop.bind(shape, do_cfg, guidance_scale, prompt_embedsU, prompt_embeds_side=prompt_embeds,
                        side_static_inputs=[(conditioning_latents, self.unet.config.in_channels)],
                        side_scale=scales[0], guess_mode=guess_mode, eta=eta, generator=generator,
                        noise_dtype=self._noise_dtype(prompt_embeds), timestep_cond=timestep_cond,
                        added_cond_kwargs=added_cond_kwargs, ip_adapter_masks=ip_adapter_masks, pag_scale=pag_scale,
                        pag_adaptive_scale=pag_adaptive_scale, guidance_rescale=guidance_rescale)
        cb = None
        bad = [k for k in callback_on_step_end_tensor_inputs if k not in self._callback_tensor_inputs]
        if bad:                                                                              # check_inputs, :775-780
            raise ValueError(f"`callback_on_step_end_tensor_inputs` has to be in {self._callback_tensor_inputs}, but "
                             f"found {bad}")
        if callback is not None or callback_on_step_end is not None:
            state = {"prompt_embeds": prompt_embeds, "negative_prompt_embeds": negative_prompt_embeds}

            def cb(i, t, lat):
                if callback_on_step_end is not None:
                    # :1451-1459 -- the callback sees the tensors it asked for and may hand back replacements:
                    #   latents         the loop owns `lat`: new values are copied into it (the next replay reads it);
                    #   prompt_embeds   in the reference's loop that name is BrushNet's context (`encoder_hidden_states=
                    #                   prompt_embeds`, :1411-1419): the side network's hoisted cross-attention K / V^T are
                    #                   recomputed in place (same arena addresses -> the captured step graph stays valid);
                    #   negative_prompt_embeds   rebinds a local the reference never reads again: recorded only.
                    kwargs = {k: (lat if k == "latents" else state[k]) for k in callback_on_step_end_tensor_inputs}
                    ret = callback_on_step_end(self, i, t, kwargs)
                    if isinstance(ret, dict):
                        new = ret.pop("latents", lat)
                        if new is not lat:
                            lat.copy_(new.to(lat.device, lat.dtype))
                        pe = ret.pop("prompt_embeds", state["prompt_embeds"])
                        if pe is not state["prompt_embeds"]:
                            if tuple(pe.shape) != tuple(state["prompt_embeds"].shape):
                                raise ValueError(f"callback_on_step_end returned prompt_embeds of shape {tuple(pe.shape)}, "
                                                 f"the loop was built for {tuple(state['prompt_embeds'].shape)}")
                            state["prompt_embeds"] = pe
                            side_rt = self._loop.side_rt
                            ctx = pe.chunk(2)[1] if (guess_mode and do_cfg and pe.shape[0] == 2 * nb) else pe
                            if pag_scale > 0:                   # (the side network runs [.., cond, cond])
                                ctx = PAGM.layout(ctx, nb, do_cfg)
                            side_rt.set_context(ctx.to(device), force=True)
                        state["negative_prompt_embeds"] = ret.pop("negative_prompt_embeds", state["negative_prompt_embeds"])
                if callback is not None and self._legacy_callback_row(i, n, num_inference_steps) and \
                        i % callback_steps == 0:
                    callback(i // getattr(self.scheduler, "order", 1), t, lat)                   # :1462-1466
        out = self._loop.run(latents, n, use_graph=self.use_graph, callback=cb, timesteps=timesteps,
                             scale_schedule=scales)
        return self._finish(out.clone(), output_type, return_dict, prompt_embeds.dtype, generator)
