"""Shared host plumbing of the three PowerPaint pipelines (everything either side of the denoising loop).

Restates, for the parts the hot path needs, the helpers of
/root/reference/powerpaint/pipelines/pipeline_PowerPaint.py (check_inputs 553-602, _encode_prompt 317-518,
prepare_latents 604-655, prepare_mask_latents 671-710, get_timesteps 713-720, prepare_mask_and_masked_image 39-153).
VAE / CLIP / tokenizer are duck-typed collaborators passed in by the caller (out of scope of this build,
SURVEY.md section 8f); every entry point also accepts ready-made latents / embeddings so the loop can be driven
without them.
"""
import inspect
from types import SimpleNamespace
from typing import List, Optional, Union

import numpy as np
import torch

from .. import _lib as L
from ..loaders import PipelinePretrainedMixin


class StableDiffusionPipelineOutput(SimpleNamespace):
    def __getitem__(self, i):
        return (self.images, self.nsfw_content_detected)[i]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def hip_mask_prep(mode: int, a: torch.Tensor, b: Optional[torch.Tensor], out_shape, batch, c, h, w, ho=0, wo=0):
    """Bit-exact mask ops on the device (pp_mask_prep)."""
    a = a.contiguous().float()
    out = torch.empty(out_shape, dtype=torch.float32, device=a.device)
    bp = b.contiguous().float() if b is not None else None
    L.check(L.lib().pp_mask_prep(mode, a.data_ptr(), bp.data_ptr() if bp is not None else None, out.data_ptr(), batch,
                                 c, h, w, ho, wo, _stream()), "pp_mask_prep")
    return out


def prepare_mask_and_masked_image(image, mask, height, width, device, return_image: bool = False):
    """pipeline_PowerPaint.py:39-153.  Tensor and PIL/ndarray inputs; binarisation and masking run in the HIP kernel."""
    if image is None:
        raise ValueError("`image` input cannot be undefined.")
    if mask is None:
        raise ValueError("`mask_image` input cannot be undefined.")
    if isinstance(image, torch.Tensor):
        if not isinstance(mask, torch.Tensor):
            raise TypeError(f"`image` is a torch.Tensor but `mask` (type: {type(mask)} is not")
        if image.ndim == 3:
            assert image.shape[0] == 3, "Image outside a batch should be of shape (3, H, W)"
            image = image.unsqueeze(0)
        if mask.ndim == 2:
            mask = mask.unsqueeze(0).unsqueeze(0)
        if mask.ndim == 3:
            mask = mask.unsqueeze(0) if mask.shape[0] == 1 else mask.unsqueeze(1)
        assert image.ndim == 4 and mask.ndim == 4, "Image and Mask must have 4 dimensions"
        assert image.shape[-2:] == mask.shape[-2:], "Image and Mask must have the same spatial dimensions"
        assert image.shape[0] == mask.shape[0], "Image and Mask must have the same batch size"
        if image.min() < -1 or image.max() > 1:
            raise ValueError("Image should be in [-1, 1] range")
        if mask.min() < 0 or mask.max() > 1:
            raise ValueError("Mask should be in [0, 1] range")
        image = image.to(device=device, dtype=torch.float32)
        mask = mask.to(device=device, dtype=torch.float32)
    elif isinstance(mask, torch.Tensor):
        raise TypeError(f"`mask` is a torch.Tensor but `image` (type: {type(image)} is not")
    else:
        import PIL.Image
        if isinstance(image, (PIL.Image.Image, np.ndarray)):
            image = [image]
        if isinstance(image, list) and isinstance(image[0], PIL.Image.Image):
            image = [i.resize((width, height), resample=PIL.Image.LANCZOS) for i in image]
            image = np.concatenate([np.array(i.convert("RGB"))[None, :] for i in image], axis=0)
        elif isinstance(image, list) and isinstance(image[0], np.ndarray):
            image = np.concatenate([i[None, :] for i in image], axis=0)
        image = torch.from_numpy(image.transpose(0, 3, 1, 2)).to(dtype=torch.float32) / 127.5 - 1.0
        if isinstance(mask, (PIL.Image.Image, np.ndarray)):
            mask = [mask]
        if isinstance(mask, list) and isinstance(mask[0], PIL.Image.Image):
            mask = [i.resize((width, height), resample=PIL.Image.LANCZOS) for i in mask]
            mask = np.concatenate([np.array(m.convert("L"))[None, None, :] for m in mask], axis=0)
            mask = mask.astype(np.float32) / 255.0
        elif isinstance(mask, list) and isinstance(mask[0], np.ndarray):
            mask = np.concatenate([m[None, None, :] for m in mask], axis=0)
        image = image.to(device)
        mask = torch.from_numpy(np.ascontiguousarray(mask)).to(device=device, dtype=torch.float32)
    B, _, H, W = image.shape
    mask = hip_mask_prep(0, mask, None, mask.shape, mask.shape[0], 1, H, W)               # binarise  (:143-144)
    masked_image = hip_mask_prep(1, image, mask, image.shape, B, image.shape[1], H, W)    # image*(mask<0.5) (:147)
    if return_image:
        return mask, masked_image, image
    return mask, masked_image


class PipelineBase(PipelinePretrainedMixin):
    """Minimal DiffusionPipeline stand-in: component registry, device, progress bar, scheduler kwargs probing."""

    def register_modules(self, **mods):
        self._modules = mods
        for k, v in mods.items():
            setattr(self, k, v)

    @property
    def _execution_device(self):
        return self.unet.device

    @property
    def device(self):
        return self.unet.device

    def to(self, *a, **k):
        """Forwards the request to every component that has a `.to` (int arguments = cuda indices): the packed HIP
        networks are no-ops for their own device / dtype and REFUSE a different one (models/_base.py), so
        `pipe.to(torch.float16)` on a bf16 pipeline raises instead of being silently ignored."""
        a = tuple(torch.device("cuda", v) if isinstance(v, int) and not isinstance(v, bool) else v for v in a)
        if isinstance(k.get("device"), int):
            k = dict(k, device=torch.device("cuda", k["device"]))
        mods = [(name, m) for name, m in getattr(self, "_modules", {}).items()
                if m is not None and hasattr(m, "to") and name != "scheduler"]
        # the packed HIP networks only VALIDATE the request (and may refuse it): ask them before any nn.Module is converted,
        # so that a refused `pipe.to(torch.float16)` leaves the pipeline as it was
        mods.sort(key=lambda nm: isinstance(nm[1], torch.nn.Module))
        for name, m in mods:
            r = m.to(*a, **k)
            if isinstance(m, torch.nn.Module) and r is not None:
                setattr(self, name, r)
                self._modules[name] = r
        return self

    def progress_bar(self, iterable=None, total=None):
        try:
            from tqdm.auto import tqdm
            cfg = getattr(self, "_progress_bar_config", {"disable": True})
            return tqdm(iterable, total=total, **cfg)
        except Exception:  # pragma: no cover
            class _N:
                def __enter__(s): return s
                def __exit__(s, *a): return False
                def update(s, *a): pass
            return _N()

    def set_progress_bar_config(self, **kw):
        self._progress_bar_config = kw

    # Memory-saving switches of DiffusionPipeline that app.py flips (`enable_model_cpu_offload()`, app.py:199) or users
    # habitually call.  With 288 GB of HBM and static arenas there is nothing to offload or slice: accepted, no effect.
    def enable_model_cpu_offload(self, gpu_id=0, device="cuda"):
        return None

    def enable_sequential_cpu_offload(self, gpu_id=0, device="cuda"):
        return None

    def maybe_free_model_hooks(self):
        return None

    def enable_attention_slicing(self, slice_size="auto"):
        return None

    def disable_attention_slicing(self):
        return None

    def enable_vae_slicing(self):
        return None

    def disable_vae_slicing(self):
        return None

    def enable_vae_tiling(self):
        return None

    def disable_vae_tiling(self):
        return None

    def enable_xformers_memory_efficient_attention(self, attention_op=None):
        return None

    def disable_xformers_memory_efficient_attention(self):
        return None

    # ---- LoRA adapters (the reference's pipelines inherit LoraLoaderMixin, pipeline_PowerPaint_Brushnet_CA.py:147-148).
    # Every active adapter is always MERGED into the packed weights (models/unet_2d_condition.py, models/clip_text.py); the
    # call's `cross_attention_kwargs["scale"]` is folded in before the loop starts.  UNet keys go to `unet`, text-encoder keys
    # to `text_encoder` only (`text_encoder_brushnet`, BrushNet, ControlNet and VAE take no adapters).
    def _lora_components(self):
        out = [("unet", self.unet)] if hasattr(self.unet, "merge_adapters") else []     # (duck-typed networks take none)
        te = getattr(self, "text_encoder", None)
        if te is not None and hasattr(te, "load_lora_adapter"):
            out.append(("text_encoder", te))
        return out

    def load_lora_weights(self, pretrained_model_name_or_path_or_dict, weight_name=None, adapter_name=None, **kwargs):
        from ..lora import read_lora, text_targets, unet_targets
        comps = dict(self._lora_components())
        if "unet" not in comps:
            raise L.PPError(f"{type(self.unet).__name__} takes no LoRA adapters")
        ad = read_lora(pretrained_model_name_or_path_or_dict, weight_name, unet_targets(self.unet.net),
                       text_targets(comps["text_encoder"]) if "text_encoder" in comps else {})
        names = self.__dict__.setdefault("_lora_names", {})
        if adapter_name is None:
            i = 0
            while f"default_{i}" in names:
                i += 1
            adapter_name = f"default_{i}"
        if adapter_name in names:
            raise ValueError(f"Adapter name {adapter_name} already in use in the pipeline")
        if ad.text_encoder and "text_encoder" not in comps:
            raise L.PPError(f"the adapter has text-encoder keys (e.g. {next(iter(ad.text_encoder))!r}) but the pipeline has "
                            f"no text encoder that takes adapters")
        parts, done = [c for c, fac in ad.components().items() if fac], []
        try:
            for c in parts:
                comps[c].load_lora_adapter(ad, adapter_name)
                done.append(c)
        except Exception:
            for c in done:                      # all components or none: no half-loaded name stays behind
                comps[c].delete_adapters(adapter_name)
            raise
        names[adapter_name] = parts
        return self

    def set_adapters(self, adapter_names, adapter_weights=None):
        adapter_names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        if adapter_weights is None or not isinstance(adapter_weights, (list, tuple)):
            adapter_weights = [adapter_weights] * len(adapter_names)
        if len(adapter_weights) != len(adapter_names):
            raise ValueError(f"Length of adapter names {len(adapter_names)} is not equal to the length of the weights "
                             f"{len(adapter_weights)}")
        names = self.__dict__.get("_lora_names", {})
        for n in adapter_names:
            if n not in names:
                raise ValueError(f"Adapter {n!r} is not loaded (loaded: {sorted(names)})")
        for c, m in self._lora_components():
            pairs = [(n, w) for n, w in zip(adapter_names, adapter_weights) if c in names[n]]
            m.set_adapters([n for n, _ in pairs], [w for _, w in pairs])

    def get_active_adapters(self):
        out = []
        for _, m in self._lora_components():
            out += [n for n in m.active_adapters() if n not in out]
        return out

    def get_list_adapters(self):
        out = {}
        for n, cs in self.__dict__.get("_lora_names", {}).items():
            for c in cs:
                out.setdefault(c, []).append(n)
        return out

    def delete_adapters(self, adapter_names):
        adapter_names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        names = self.__dict__.get("_lora_names", {})
        comps = dict(self._lora_components())
        for n in adapter_names:
            if n not in names:
                raise ValueError(f"Adapter {n!r} is not loaded")
            for c in names.pop(n):
                comps[c].delete_adapters(n)
        self.__dict__.pop("_prompt_memo", None)

    def unload_lora_weights(self):
        self.delete_adapters(list(self.__dict__.get("_lora_names", {})))
        self.unfuse_lora()
        self._merge_lora(None)

    def fuse_lora(self, fuse_unet=True, fuse_text_encoder=True, lora_scale: float = 1.0, **kwargs):
        """Kept for source compatibility: every adapter is merged anyway; this only fixes the scale (a later
        `cross_attention_kwargs["scale"]` then has no effect, as after diffusers' fuse_lora)."""
        self._lora_fused = float(lora_scale)
        for _, m in self._lora_components():
            m.__dict__["lora_scale_fixed"] = self._lora_fused      # (holds for direct calls of the models too)
        self._merge_lora(None)

    def unfuse_lora(self, **kwargs):
        self.__dict__.pop("_lora_fused", None)
        for _, m in self._lora_components():
            m.__dict__.pop("lora_scale_fixed", None)

    def _merge_lora(self, cross_attention_kwargs):
        """Bring unet / text encoder to the call's LoRA scale and return it (a no-op for a model without adapters)."""
        s = self.__dict__.get("_lora_fused")
        if s is None:
            s = (cross_attention_kwargs or {}).get("scale", 1.0)
        for c, m in self._lora_components():
            changed = m.merge_adapters(s)
            if c == "text_encoder" and changed:
                self.__dict__.pop("_prompt_memo", None)        # embeddings of the previous weights
        return s

    def set_pag_applied_layers(self, layers="mid"):
        """diffusers' `pag_applied_layers` (PAGMixin): a string or a list of strings, each searched as a regular expression
        in the names of the UNet's self-attention modules (`mid_block.attentions.0.transformer_blocks.0.attn1`, ...).  The
        selection takes effect in calls with `pag_scale > 0`.  An entry that selects nothing raises ValueError at once."""
        self.unet.set_pag_applied_layers(layers)
        return self

    def _refuse_ip_adapter_masks(self, cross_attention_kwargs):
        """A pipeline without an IP-Adapter path: `cross_attention_kwargs["ip_adapter_masks"]` is refused, never dropped."""
        if (cross_attention_kwargs or {}).get("ip_adapter_masks") is not None:
            raise ValueError(f"{type(self).__name__} has no IP-Adapter path: `ip_adapter_masks` would confine an image prompt "
                             f"that this pipeline never applies (StableDiffusionPowerPaintBrushNetPipeline takes them, after "
                             f"`load_ip_adapter`)")

    def prepare_extra_step_kwargs(self, generator, eta):
        """pipeline_PowerPaint.py:536-551."""
        kw = {}
        params = set(inspect.signature(self.scheduler.step).parameters.keys())
        if "eta" in params:
            kw["eta"] = eta
        if "generator" in params:
            kw["generator"] = generator
        return kw

    @staticmethod
    def _noise_dtype(prompt_embeds):
        """The reference draws the initial noise in prompt_embeds.dtype (prepare_latents(..., prompt_embeds.dtype, ...),
        pipeline_PowerPaint.py:930-940) and only then runs the loop; the HIP loop keeps latents in fp32, so the draw
        happens in the reference's dtype (same generator state, same rounded values) and is widened afterwards."""
        dt = getattr(prompt_embeds, "dtype", torch.float32)
        return dt if dt in (torch.float16, torch.bfloat16, torch.float32) else torch.float32

    def _legacy_callback_row(self, i, rows, num_inference_steps) -> bool:
        """Does the legacy `callback` fire after row `i` of `rows`?  pipeline_PowerPaint.py:986,1038: with a scheduler of
        `order` 2 (Heun, DPM2, DPM2 ancestral: two network evaluations per step) only after a step's second evaluation and
        after the last row, `num_warmup_steps = rows - num_inference_steps * order`.  (`callback_on_step_end` of the BrushNet
        pipeline fires after every row, as in the reference's loop.)"""
        order = getattr(self.scheduler, "order", 1)
        if order == 1:
            return True
        return i == rows - 1 or ((i + 1) > rows - num_inference_steps * order and (i + 1) % order == 0)

    def get_timesteps(self, num_inference_steps, strength, device):
        """pipeline_PowerPaint.py:713-720.  The schedulers of this package additionally learn where the loop enters
        (`set_begin_index`): their per-step tables are indexed by a device-side step counter, not by timestep lookup."""
        init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
        t_start = max(num_inference_steps - init_timestep, 0)
        timesteps = self.scheduler.timesteps[t_start * self.scheduler.order:]
        if t_start and getattr(self.scheduler, "kind", -1) >= 0:
            self.scheduler.set_begin_index(t_start * self.scheduler.order)
        return timesteps, num_inference_steps - t_start

    def _initial_latents(self, shape, strength, timesteps, latents, init_image, generator, device, noise_dtype,
                         return_image_latents=False, return_all=False):
        """prepare_latents (pipeline_PowerPaint.py:604-655): pure noise * init_noise_sigma at strength 1 (or when the
        caller hands `latents`, which the reference then treats as the noise whatever the strength), otherwise the
        VAE latents of the init image noised to the first timestep of the shortened schedule.  Draw order as in the
        reference: the init image's posterior sample BEFORE the noise.  `return_image_latents` (a 4-channel UNet,
        :927-928): the init image is encoded in every case.  return_all -> (latents, noise, image_latents | None)."""
        image_latents = None
        if return_image_latents or (latents is None and strength != 1.0):
            if init_image is None:
                raise ValueError("Since strength < 1. initial latents are to be initialised as a combination of Image + "
                                 "Noise.However, either the image or the noise timestep has not been provided.")
            image_latents = self._vae_encode(init_image.to(device=device, dtype=noise_dtype), generator)
        if latents is not None:
            noise = latents.to(device=device)
            out = noise.to(torch.float32) * self.scheduler.init_noise_sigma
        else:
            noise = randn_tensor(shape, generator=generator, device=device, dtype=noise_dtype)
            if strength == 1.0:
                out = noise.to(torch.float32) * self.scheduler.init_noise_sigma
            else:
                t0 = timesteps[:1].repeat(shape[0])
                out = self.scheduler.add_noise(image_latents.to(noise.dtype), noise, t0).to(torch.float32)
        return (out, noise, image_latents) if return_all else out

    # ---- text: promptA/promptB blended by `tradoff` (pipeline_PowerPaint.py:317-518)
    def _text_embeds(self, text_encoder, prompt: Union[str, List[str]], device):
        tok = self.tokenizer
        ids = tok(prompt, padding="max_length", max_length=tok.model_max_length, truncation=True,
                  return_tensors="pt").input_ids
        out = text_encoder(ids.to(device))
        return out[0]

    def _encode_prompt(self, promptA, promptB, t, device, num_images_per_prompt, do_classifier_free_guidance,
                       negative_promptA=None, negative_promptB=None, t_nag=None, prompt_embeds=None,
                       negative_prompt_embeds=None, lora_scale=None, text_encoder=None):
        text_encoder = text_encoder or getattr(self, "text_encoder", None)
        if lora_scale is not None and text_encoder is getattr(self, "text_encoder", None) and \
                hasattr(text_encoder, "merge_adapters") and text_encoder.merge_adapters(lora_scale):
            self.__dict__.pop("_prompt_memo", None)
        # A call that passes the SAME embedding tensors as the previous one (unchanged storage and version counter) gets the
        # same result OBJECT: the networks then recognise their context and skip the per-prompt set-up (hoisted cross-attention
        # K / V, the folded projections: ~2 ms per call) instead of redoing it for an identical tensor.
        memo_key = None
        if prompt_embeds is not None and torch.is_tensor(prompt_embeds) and \
                (negative_prompt_embeds is None or torch.is_tensor(negative_prompt_embeds)) and \
                (not do_classifier_free_guidance or negative_prompt_embeds is not None):
            ident = lambda t: None if t is None else (id(t), t.data_ptr(), t._version, tuple(t.shape), t.dtype, str(t.device))  # noqa: E731
            memo_key = (ident(prompt_embeds), ident(negative_prompt_embeds), str(device), num_images_per_prompt,
                        bool(do_classifier_free_guidance))
            memo = self.__dict__.setdefault("_prompt_memo", {})
            if memo_key in memo:
                return memo[memo_key][0]
            src_keep = (prompt_embeds, negative_prompt_embeds)     # (an identity only holds while the tensors live)
        if prompt_embeds is None:
            if text_encoder is None or getattr(self, "tokenizer", None) is None:
                raise ValueError("no text encoder / tokenizer registered: pass prompt_embeds (and negative_prompt_embeds)")
            eA = self._text_embeds(text_encoder, promptA, device)
            eB = self._text_embeds(text_encoder, promptB, device)
            prompt_embeds = eA * t + (1 - t) * eB                                          # :423
        bs = prompt_embeds.shape[0]
        prompt_embeds = prompt_embeds.to(device=device)
        _, seq, _ = prompt_embeds.shape
        prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt, 1).view(bs * num_images_per_prompt, seq, -1)
        if do_classifier_free_guidance:
            if negative_prompt_embeds is None:
                if text_encoder is None:
                    raise ValueError("classifier-free guidance needs negative_prompt_embeds when no text encoder is set")
                # pipeline_PowerPaint.py:441-460: `negative_prompt` IS negative_promptA -- when it is None BOTH
                # unconditional prompts are "" (a lone negative_promptB is ignored), a str is used as given, a list must
                # match the prompt's type and batch size
                if negative_promptA is None:
                    nA = nB = [""] * bs
                elif promptA is not None and type(promptA) is not type(negative_promptA):
                    raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got "
                                    f"{type(negative_promptA)} != {type(promptA)}.")
                elif isinstance(negative_promptA, str):
                    nA, nB = [negative_promptA], [negative_promptB]
                elif bs != len(negative_promptA):
                    raise ValueError(f"`negative_prompt`: {negative_promptA} has batch size {len(negative_promptA)}, but "
                                     f"`prompt`: {promptA} has batch size {bs}. Please make sure that passed "
                                     "`negative_prompt` matches the batch size of `prompt`.")
                else:
                    nA, nB = negative_promptA, negative_promptB
                eA = self._text_embeds(text_encoder, nA, device)
                eB = self._text_embeds(text_encoder, nB, device)
                negative_prompt_embeds = eA * t_nag + (1 - t_nag) * eB                     # :499
            negative_prompt_embeds = negative_prompt_embeds.to(device=device)
            seq = negative_prompt_embeds.shape[1]
            negative_prompt_embeds = negative_prompt_embeds.repeat(1, num_images_per_prompt, 1).view(
                bs * num_images_per_prompt, seq, -1)
            prompt_embeds = torch.cat([negative_prompt_embeds, prompt_embeds])             # :516  [uncond, cond]
        if memo_key is not None:
            memo = self.__dict__.setdefault("_prompt_memo", {})
            while len(memo) >= 4:                                  # (a few live entries: ppt-v2 encodes two prompt pairs per call)
                memo.pop(next(iter(memo)))
            memo[memo_key] = (prompt_embeds, src_keep)
        return prompt_embeds

    def _vae_encode(self, image, generator):
        vae = getattr(self, "vae", None)
        if vae is None:
            raise ValueError("no VAE registered: pass the latent-space inputs directly")
        if isinstance(generator, list):
            lat = torch.cat([retrieve_latents(vae.encode(image[i:i + 1]), generator[i])
                             for i in range(image.shape[0])], dim=0)
        else:
            lat = retrieve_latents(vae.encode(image), generator)
        return vae.config.scaling_factor * lat

    def _decode_condition(self, init_image, mask, generator, device, dtype):
        """The `condition_kwargs` of the reference's decode (pipeline_PowerPaint.py:1043-1049, pipeline_PowerPaint_ControlNet.py:
        1317-1324): with an AsymmetricAutoencoderKL as `vae`, the preprocessed init image and the preprocessed mask go to
        `decode`.  The reference also calls `_encode_vae_image(init_image, generator)` there and drops the result; all that call
        leaves behind is the generator, advanced by the posterior's noise draw -- the draw is made (same shape, the dtype of this
        VAE's moments, same per-item order for a list of generators) and discarded, the encoder does not run.  `dtype`: that of
        the masked-image latents, which the reference casts both tensors to.  {} for every other VAE."""
        from ..models.autoencoder_asym_kl import AsymmetricAutoencoderKL
        vae = getattr(self, "vae", None)
        if not isinstance(vae, AsymmetricAutoencoderKL) or init_image is None or mask is None:
            return {}
        dt = next(iter(vae.parameters())).dtype
        init_image = init_image.to(device=device, dtype=dtype)
        n, f = init_image.shape[0], vae._enc_scale
        lat = (1, vae.config.latent_channels, init_image.shape[2] // f, init_image.shape[3] // f)
        if isinstance(generator, list):
            for i in range(n):
                randn_tensor(lat, generator=generator[i], device=device, dtype=dt)
        else:
            randn_tensor((n,) + lat[1:], generator=generator, device=device, dtype=dt)
        return {"image": init_image.clone(), "mask": mask.clone().to(device=device, dtype=dtype)}

    def _finish(self, latents, output_type, return_dict, prompt_dtype, generator=None, condition=None):
        """condition: callable -> the keyword arguments `vae.decode` gets on top (evaluated only when an image is decoded)."""
        if output_type != "latent":
            vae = getattr(self, "vae", None)
            if vae is None:
                raise ValueError('no VAE registered: use output_type="latent"')
            image = vae.decode(latents.to(next(iter(vae.parameters())).dtype) / vae.config.scaling_factor,
                               return_dict=False, **(condition() if condition is not None else {}))[0]
            ip = getattr(self, "image_processor", None)
            if ip is not None:
                image = ip.postprocess(image, output_type=output_type, do_denormalize=[True] * image.shape[0])
                loop = getattr(self, "_loop", None)
                if loop is not None and output_type in ("pil", "np"):     # (the images are on the host: the device is idle anyway)
                    loop.flush_faults()
        else:
            image = latents
        if not return_dict:
            return (image, None)
        return StableDiffusionPipelineOutput(images=image, nsfw_content_detected=None)


def randn_tensor(shape, generator=None, device=None, dtype=torch.float32):
    """diffusers.utils.torch_utils.randn_tensor: CPU generator -> sample on CPU then move."""
    gdev = generator.device.type if isinstance(generator, torch.Generator) else None
    if isinstance(generator, list):
        shape1 = (1,) + tuple(shape[1:])
        return torch.cat([randn_tensor(shape1, g, device, dtype) for g in generator], dim=0)
    if gdev == "cpu" or generator is None and (device is None or torch.device(device).type == "cpu"):
        return torch.randn(shape, generator=generator, dtype=dtype).to(device)
    return torch.randn(shape, generator=generator, device=device, dtype=dtype)


def retrieve_latents(encoder_output, generator=None):
    """diffusers' `retrieve_latents` (sample mode): a posterior (`latent_dist`, AutoencoderKL / AsymmetricAutoencoderKL) is
    sampled with `generator`; a deterministic encoder's `latents` (AutoencoderTiny) are taken as they are and the generator
    is not touched."""
    if hasattr(encoder_output, "latent_dist"):
        return encoder_output.latent_dist.sample(generator=generator)
    if hasattr(encoder_output, "latents"):
        return encoder_output.latents
    raise AttributeError("vae.encode(...) returned neither `latent_dist` nor `latents`")
