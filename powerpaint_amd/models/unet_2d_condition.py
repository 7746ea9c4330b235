"""UNet2DConditionModel on the MI355X HIP path.

Drop-in for the call surface of /root/reference/powerpaint/models/unet_2d_condition.py:1040-1058 (the fork, incl.
`down_block_add_samples` / `mid_block_add_sample` / `up_block_add_samples`) and of the stock diffusers class the
v1 / ControlNet pipelines import (/root/reference/powerpaint/pipelines/pipeline_PowerPaint.py:27,1009-1015;
pipeline_PowerPaint_ControlNet.py:1707-1715: `down_block_additional_residuals`, `mid_block_additional_residual`).
"""
from types import SimpleNamespace
from typing import Any, Dict, List, Optional, Tuple, Union

import torch

from .. import _lib as L
from .. import ip_adapter as IPA
from .. import pag as PAGM
from ..lora import AdapterSet, LoraAdapter, unet_targets
from ._base import SD15_DOWN, SD15_UP, Output, _HipModel


class UNet2DConditionModel(_HipModel):
    kind = "unet"

    def __init__(self, sample_size: Optional[int] = 64, in_channels: int = 4, out_channels: int = 4,
                 down_block_types=SD15_DOWN, up_block_types=SD15_UP, block_out_channels=(320, 640, 1280, 1280),
                 layers_per_block: int = 2, norm_num_groups: int = 32, norm_eps: float = 1e-5,
                 cross_attention_dim: int = 768, attention_head_dim: int = 8, device="cuda",
                 dtype=torch.bfloat16, time_cond_proj_dim: Optional[int] = None, **unused):
        self._extra_config = unused         # validated in the base constructor (check_fixed_config)
        super().__init__(in_channels, block_out_channels, layers_per_block, attention_head_dim, cross_attention_dim,
                         norm_num_groups, norm_eps, down_block_types, up_block_types, device, dtype,
                         out_channels=out_channels, time_cond_proj_dim=time_cond_proj_dim)
        self.config = SimpleNamespace(
            sample_size=sample_size, in_channels=in_channels, out_channels=out_channels,
            down_block_types=tuple(down_block_types), up_block_types=tuple(up_block_types),
            block_out_channels=tuple(block_out_channels), layers_per_block=layers_per_block,
            norm_num_groups=norm_num_groups, norm_eps=norm_eps, cross_attention_dim=cross_attention_dim,
            attention_head_dim=attention_head_dim, time_cond_proj_dim=time_cond_proj_dim, addition_embed_type=None,
            flip_sin_to_cos=True, freq_shift=0, act_fn="silu", only_cross_attention=False,
            use_linear_projection=False, class_embed_type=None, num_class_embeds=None, upcast_attention=False,
            resnet_time_scale_shift="default", mid_block_scale_factor=1, downsample_padding=1,
            num_attention_heads=None, projection_class_embeddings_input_dim=None, encoder_hid_dim=None,
            encoder_hid_dim_type=None, addition_time_embed_dim=None, transformer_layers_per_block=1)
        self.encoder_hid_proj = None        # (IP-Adapters loaded: MultiIPAdapterImageProjection, as in diffusers)

    # ------------------------------------------------------------------ LoRA adapters (DESIGN.md "LoRA adapters")
    # Adapters are MERGED into the packed parameter buffer in place (SDNet.repack -> pp_lora_merge): the launch plans, the
    # captured graphs and the step cost stay what they are without adapters.  Kept from the first adapter on, and only for the
    # modules adapters touch: an fp32 device copy of the source weights and a byte snapshot of the packed entries that get
    # overwritten; both go when the active set becomes empty.
    def load_state_dict(self, sd, strict: bool = True, keep_state_dict: bool = False, materialize: bool = True):
        """keep_state_dict=True keeps `sd` (as BrushNetModel.from_unet needs it, and as from_pretrained does): the fp32
        source of an adapter merge is read from it, at the time of the first merge."""
        super().load_state_dict(sd, strict, keep_state_dict, materialize)
        self._lora_forget()
        # (a fresh packed buffer: IP-Adapter entries, which live behind the network's own, are gone with the old one)
        self.encoder_hid_proj, self.config.encoder_hid_dim_type = None, None
        return self

    def _lora_set(self) -> AdapterSet:
        if "_adapters" not in self.__dict__:
            self._adapters = AdapterSet()
            self._lora_forget()
        return self._adapters

    def _lora_forget(self):
        """The packed buffer holds the plain weights (again): drop what was derived for merging."""
        self._lora_src, self._lora_snap, self._lora_dirty, self._lora_state = {}, {}, [], None
        self._lora_dev = {}

    def load_lora_adapter(self, adapter, adapter_name: str = "default"):
        """adapter: a `powerpaint_amd.lora.LoraAdapter` (its `unet` part is taken) or {module: (down, up, alpha)}."""
        fac = adapter.unet if isinstance(adapter, LoraAdapter) else dict(adapter)
        targets = unet_targets(self.net)
        for m, (down, up, alpha) in fac.items():
            if m not in targets:
                raise L.PPError(f"LoRA module {m!r} matches no target module of the unet")
            shp, r = targets[m], down.shape[0]
            if tuple(down.shape[1:]) != tuple(shp[1:]) or up.reshape(up.shape[0], -1).shape != (shp[0], r):
                raise L.PPError(f"LoRA module {m!r}: factors down {tuple(down.shape)} / up {tuple(up.shape)} do not fit "
                                f"{m}.weight {shp}")
            if not 1 <= r <= L.PP_LORA_MAX_RANK:
                raise L.PPError(f"LoRA module {m!r}: rank {r} is outside 1..{L.PP_LORA_MAX_RANK}")
        self._lora_set().add(adapter_name, fac)
        return self

    def set_adapters(self, adapter_names, weights=None):
        self._lora_set().set(adapter_names, weights)
        return self

    def delete_adapters(self, adapter_names):
        ads = self._lora_set()
        ads.delete(adapter_names)
        if not ads.active:
            self.merge_adapters(1.0)          # the last one left: back to the plain weights now, copies freed
        return self

    def active_adapters(self):
        return list(self._lora_set().active)

    def list_adapters(self):
        return list(self._lora_set().loaded)

    def _lora_source(self, keys):
        sd = self._sd
        for k in keys:
            if k not in self._lora_src:
                if sd is None or k not in sd or sd[k].device.type == "meta":
                    raise L.PPError(f"{type(self).__name__}: merging an adapter needs the fp32 source weights ({k!r}), but "
                                    f"the model keeps no state dict: load it with from_pretrained or with "
                                    f"load_state_dict(sd, keep_state_dict=True) (a buffer filled through param_buffer() has "
                                    f"no source)")
                self._lora_src[k] = sd[k].to(device=self._device, dtype=torch.float32).contiguous()
        return self._lora_src

    def merge_adapters(self, scale: float = 1.0):
        """Bring the packed weights to `W + sum_a w_a * scale * (alpha_a / r_a) U_a D_a` over the active adapters; nothing
        happens when they are there already (same adapters, weights and scale)."""
        ads = self.__dict__.get("_adapters")
        if ads is None or (not ads.loaded and self._lora_state is None):
            return self
        if getattr(self, "lora_scale_fixed", None) is not None:      # (pipeline.fuse_lora: later scales have no effect)
            scale = self.lora_scale_fixed
        state = ads.state(scale)
        if state == self._lora_state:
            return self
        net, pk = self.net, self.net.params
        merged = {}
        for stale in [k for k in self._lora_dev if k not in {(n, ads.gen[n]) for n in ads.loaded}]:
            del self._lora_dev[stale]
        for name, w in ads.active.items():
            dev = self._lora_dev.get((name, ads.gen[name]))
            if dev is None:
                dev = self._lora_dev[(name, ads.gen[name])] = {
                    m: (up.reshape(up.shape[0], -1).to(device=self._device, dtype=torch.float32).contiguous(),
                        down.reshape(down.shape[0], -1).to(device=self._device, dtype=torch.float32).contiguous(),
                        float(alpha) / down.shape[0]) for m, (down, up, alpha) in ads.loaded[name].items()}
            for m, (up, down, a_over_r) in dev.items():
                merged.setdefault(m, []).append((up, down, w * float(scale) * a_over_r))
        recipes = net.recipes_of(merged) if merged else []
        names = [r.name for r in recipes]
        entries = lambda r: [e for e in (r.name, r.colsum, r.bias) if e]      # noqa: E731
        source = None
        if recipes:                         # (before anything is touched: a model without a kept state dict refuses here)
            keys = set()
            for r in recipes:
                keys |= {m + ".weight" for m in r.sources()}
                if r.gamma:
                    keys |= {r.gamma + ".weight", r.gamma + ".bias"}
                if r.badd:
                    keys.add(r.badd)
                if r.compose:
                    keys.add(r.compose + ".bias")
            source = self._lora_source(sorted(keys))
        # entries that leave the merge go back to their snapshot; entries that enter it are snapshot first
        for r in self._lora_dirty:
            if r.name not in names:
                for e in entries(r):
                    pk.tensor(e).copy_(self._lora_snap[e])
        for r in recipes:
            for e in entries(r):
                if e not in self._lora_snap:
                    self._lora_snap[e] = pk.tensor(e).clone()
        if recipes:
            net.repack(list(merged), merged, source, torch.cuda.current_stream(self._device).cuda_stream)
        self._lora_dirty = recipes
        self._lora_state = state
        if state is None:
            self._lora_forget()
        self.params_changed()
        return self

    # ------------------------------------------------------------------ IP-Adapter (DESIGN.md "IP-Adapter")
    def _load_ip_adapter_weights(self, state_dicts):
        """diffusers' `UNet2DConditionLoadersMixin._load_ip_adapter_weights`: state_dicts = one {"image_proj", "ip_adapter"}
        dict, or a list of them (several adapters, each with its own image embeds and scale at call time).  Replaces whatever
        adapters were loaded.  Everything is validated before anything changes: a refused file leaves the model as it was.
        The weights go into the packed parameter buffer (SDNet.set_ip_adapters); the plans are rebuilt on the next call,
        without the fused cross-attention forms and the CFG twin prefix (every attn2 runs to_q -> attention ->
        pp_ip_attn_add per adapter -> to_out).  Base and Plus (Resampler) files load, mixed freely; `encoder_hid_proj` shows an
        ImageProjection or an IPAdapterPlusImageProjection per adapter.  Scales start at 1.0, as in diffusers."""
        if isinstance(state_dicts, dict):
            state_dicts = [state_dicts]
        if not state_dicts:
            raise L.PPError("_load_ip_adapter_weights: no adapter given (unload with _unload_ip_adapter)")
        ads = [IPA.check_ip_adapter(self.net, IPA.read_ip_adapter(sd), f"IP-Adapter {i}") for i, sd in enumerate(state_dicts)]
        self.net.set_ip_adapters(ads)
        self.encoder_hid_proj = IPA.MultiIPAdapterImageProjection([IPA.projection_module(a, self.net.ctx_dim) for a in ads])
        self.config.encoder_hid_dim_type = "ip_image_proj"
        self.rt.key = None
        self.rt.set_ip_scales([1.0] * len(ads))
        self.params_changed()
        return self

    def _unload_ip_adapter(self):
        """Back to the UNet that never had an adapter: its packed entries, its plans (launch for launch), its config."""
        if self.net.ip:
            self.net.set_ip_adapters([])
            self.rt.key = None
            self.params_changed()
        self.encoder_hid_proj, self.config.encoder_hid_dim_type = None, None
        return self

    def set_ip_adapter_scale(self, scale):
        """A float for all adapters or one value per adapter (by-value kernel arguments: captured graphs are re-captured)."""
        if not self.net.ip:
            raise L.PPError("set_ip_adapter_scale: no IP-Adapter is loaded")
        self.rt.set_ip_scales(IPA.scales_list(scale, len(self.net.ip)))
        return self

    def _ip_image_embeds(self, added_cond_kwargs, B: int):
        """`added_cond_kwargs["image_embeds"]` of a UNet with IP-Adapters (unet_2d_condition.py:1030-1037 of the reference):
        a list with one tensor per adapter, [B, n, D] for a base adapter and [B, n, S, E] for a Plus adapter (each refuses the
        other's rank by name).  Without adapters the key is refused, never ignored."""
        if not self.net.ip:
            if added_cond_kwargs and "image_embeds" in added_cond_kwargs:
                raise L.PPError("added_cond_kwargs['image_embeds'] given but no IP-Adapter is loaded (load_ip_adapter first)")
            return None
        if not added_cond_kwargs or "image_embeds" not in added_cond_kwargs:
            raise ValueError(f"{self.__class__} has the config param `encoder_hid_dim_type` set to 'ip_image_proj' which requires "
                             f"the keyword argument `image_embeds` to be passed in  `added_conditions`")
        embeds = added_cond_kwargs["image_embeds"]
        IPA.check_image_embeds(embeds, len(self.net.ip), [len(spec) > 2 for spec in self.net.ip])
        for i, (e, spec) in enumerate(zip(embeds, self.net.ip)):
            T, D = spec[:2]
            if e.shape[0] != B or e.shape[-1] != D or (e.dim() == 4 and e.shape[2] < 1):
                raise ValueError(f"image_embeds[{i}] has shape {tuple(e.shape)}, the UNet runs batch {B} and adapter {i} takes "
                                 f"embeds of dimension {D}")
            if e.shape[1] * T > L.PP_IP_MAX_TOKENS:
                raise L.PPError(f"image_embeds[{i}]: {e.shape[1]} images of {T} tokens, at most {L.PP_IP_MAX_TOKENS} tokens "
                                f"per adapter")
        return list(embeds)

    def _check_ip_masks(self, masks):
        """`cross_attention_kwargs["ip_adapter_masks"]` of diffusers 0.27: ONE float tensor [adapters, 1, H, W] (what
        `IPAdapterMaskProcessor.preprocess` returns), shared by the batch and both CFG halves.  None passes; without a loaded
        adapter the masks are refused, as an image prompt is -- never ignored."""
        if masks is None:
            return None
        if not self.net.ip:
            raise ValueError("`ip_adapter_masks` were given but no IP-Adapter is loaded: call `load_ip_adapter` first (the masks "
                             "are never silently dropped)")
        if not isinstance(masks, torch.Tensor) or masks.ndim != 4 or not masks.is_floating_point():
            raise ValueError(" ip_adapter_mask should be a tensor with shape [num_ip_adapter, 1, height, width]."
                             " Please use `IPAdapterMaskProcessor` to preprocess your mask")
        if masks.shape[1] != 1:
            raise ValueError(f"ip_adapter_masks should be a tensor with shape [num_ip_adapter, 1, height, width], got "
                             f"{tuple(masks.shape)} (one mask per adapter: per-image masks are not implemented)")
        if len(masks) != len(self.net.ip):
            raise ValueError(f"Number of ip_adapter_masks ({len(masks)}) must match number of IP-Adapters ({len(self.net.ip)})")
        if not bool(torch.isfinite(masks).all()):
            raise ValueError("ip_adapter_masks hold non-finite values")
        return masks

    # ------------------------------------------------------------------ FreeU (DESIGN.md "FreeU")
    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """FreeU (https://arxiv.org/abs/2309.11497), the reference's `UNet2DConditionModel.enable_freeu`
        (unet_2d_condition.py:835-857): in front of every resnet of the first two up blocks the first half of the backbone
        channels is scaled by b1 / b2 and the skip tensor's four lowest frequency bins by s1 / s2 (one pp_freeu launch each).
        As in the reference's up blocks (unet_2d_blocks.py:2563-2568) the mechanism is on only while all four are truthy."""
        self._freeu = (s1, s2, b1, b2)
        return self

    def disable_freeu(self):
        """The reference's `disable_freeu` (unet_2d_condition.py:859-865): the plan and the outputs of a UNet that never had it."""
        self._freeu = (None, None, None, None)
        return self

    def _freeu_values(self):
        v = self.__dict__.get("_freeu")
        return tuple(float(x) for x in v) if v is not None and all(v) else None

    # ------------------------------------------------------------------ perturbed-attention guidance
    def pag_attn1_names(self):
        """The self-attention modules of this UNet by their diffusers names, in execution order."""
        return PAGM.attn1_names([p for p, _ in self.net._attn_specs()])

    def set_pag_applied_layers(self, layers="mid"):
        """diffusers' `pag_applied_layers` (a string or a list of strings, each a regular expression searched in the names of
        the self-attention modules; PAGMixin's rules, pag.resolve_layers).  Invalid entries raise at once.  What is stored is
        the resolved set of transformers; it takes effect in calls with `pag_scale > 0` (prepare(pag_batch=...))."""
        self._pag_layers = PAGM.resolve_prefixes(layers, [p for p, _ in self.net._attn_specs()])
        return self

    def pag_layers(self):
        """The transformers `set_pag_applied_layers` selected (default: "mid")."""
        if self.__dict__.get("_pag_layers") is None:
            self.set_pag_applied_layers("mid")
        return self._pag_layers

    # ------------------------------------------------------------------
    def _wiring(self, down_add, mid_add, up_add, ctrl_down, ctrl_mid):
        def ptrs(lst):
            # zero-copy hand-off of a side network's NHWC arena tensor -- only when it is stored in THIS network's 16-bit
            # format (a bf16 BrushNet feeding an fp16 UNet would have its bits reinterpreted); any other tensor goes
            # through `load_residual`, which converts
            return [getattr(t, "_pp_nhwc_ptr", 0) if t.dtype == self._dtype else 0 for t in lst]

        if down_add is not None and mid_add is not None and up_add is not None:
            return ("brushnet", {"down": ptrs(down_add), "mid": ptrs([mid_add]), "up": ptrs(up_add)})
        if ctrl_down is not None and ctrl_mid is not None:
            return ("controlnet", {"down": ptrs(ctrl_down), "mid": ptrs([ctrl_mid])})
        return ("plain",)

    def prepare(self, sample_shape, encoder_hidden_states, down_block_add_samples=None, mid_block_add_sample=None,
                up_block_add_samples=None, down_block_additional_residuals=None, mid_block_additional_residual=None,
                twin: bool = False, timestep_cond: Optional[torch.Tensor] = None, added_cond_kwargs=None,
                ip_adapter_masks: Optional[torch.Tensor] = None, pag_batch: int = 0):
        """Compile (or reuse) the launch plan for this shape / residual wiring and bind the inputs.  pag_batch > 0:
        perturbed-attention guidance -- the LAST pag_batch items of the batch are the perturbed segment: in the transformers
        `pag_layers()` their self-attention is the identity (one re-plan when it is switched on or off; 0: the plan of a UNet
        that never had it).  added_cond_kwargs:
        {"image_embeds": [...]} while IP-Adapters are loaded (_ip_image_embeds), copied in on every call.  ip_adapter_masks:
        `cross_attention_kwargs["ip_adapter_masks"]` (_check_ip_masks) -- masked or not is part of the plan key, the values
        are per-row weights in device memory, rewritten on every call (NetRuntime.set_ip_masks).  timestep_cond: the
        guidance embedding of a UNet with `time_cond_proj_dim` ([B or 1, d], one value over the batch; None = no term, as
        in diffusers) -- constant over a denoising call, folded into the time embedding's first bias once
        (NetRuntime.set_timestep_cond).  twin: the caller (the
        fused denoising loop) vouches that the second half of the batch is a copy of the first (`torch.cat([latents] * 2)`
        over CFG-duplicated mask / masked-image latents, pipeline_PowerPaint.py:990-996): the prompt-independent prefix of
        the forward pass then runs on one half (NetRuntime.ensure).  `forward` never sets it."""
        B, Cin, H, W = sample_shape
        if Cin != self.config.in_channels:
            raise ValueError(f"sample has {Cin} channels, unet.config.in_channels = {self.config.in_channels}")
        wiring = self._wiring(down_block_add_samples, mid_block_add_sample, up_block_add_samples,
                              down_block_additional_residuals, mid_block_additional_residual)
        ip_masks = self._check_ip_masks(ip_adapter_masks)
        ip_embeds = self._ip_image_embeds(added_cond_kwargs, B)
        self.rt.ensure(B, H, W, self._nctx(encoder_hidden_states), Cin, wiring, twin=twin, freeu=self._freeu_values(),
                       ip_n=[e.shape[1] if e.dim() == 3 else (e.shape[1], e.shape[2]) for e in ip_embeds] if ip_embeds else (),
                       ip_masked=ip_masks is not None, pag=PAGM.setting(self.pag_layers(), pag_batch) if pag_batch else None)
        if ip_embeds:
            self.rt.set_ip_embeds(ip_embeds)
        if ip_masks is not None:
            self.rt.set_ip_masks(ip_masks)
        if wiring[0] != "plain":
            groups = {"down": down_block_add_samples if wiring[0] == "brushnet" else down_block_additional_residuals,
                      "mid": [mid_block_add_sample if wiring[0] == "brushnet" else mid_block_additional_residual]}
            if wiring[0] == "brushnet":
                groups["up"] = up_block_add_samples
            for g, lst in groups.items():
                exp = len(self.rt.lay["slots"][g])
                if len(lst) != exp:
                    raise ValueError(f"{g} residual list has {len(lst)} tensors, expected {exp}")
                for i, (t, p) in enumerate(zip(lst, wiring[1][g])):
                    if not p:
                        self.rt.load_residual(g, i, t)
        self.rt.set_context(encoder_hidden_states)
        self.rt.set_timestep_cond(self._check_timestep_cond(timestep_cond, B))
        return self.rt

    def _check_timestep_cond(self, c, B):
        d = self.config.time_cond_proj_dim
        if c is None:
            return None
        if d is None:
            raise NotImplementedError("timestep_cond needs a UNet with config.time_cond_proj_dim (a guidance-embedded, "
                                      "LCM-distilled UNet); this one has none")
        if c.dim() != 2 or c.shape[1] != d or c.shape[0] not in (1, B):
            raise ValueError(f"timestep_cond must be [{B} or 1, {d}], got {tuple(c.shape)}")
        if c.shape[0] > 1 and not bool(torch.equal(c, c[:1].expand_as(c))):
            raise ValueError("timestep_cond differs over the batch: the HIP path computes ONE time embedding per step "
                             "(one guidance scale per call, as the pipelines build it)")
        return c[:1]

    @torch.no_grad()
    def forward(self, sample: torch.Tensor, timestep: Union[torch.Tensor, float, int],
                encoder_hidden_states: torch.Tensor, class_labels=None, timestep_cond=None, attention_mask=None,
                cross_attention_kwargs: Optional[Dict[str, Any]] = None, added_cond_kwargs=None,
                down_block_additional_residuals: Optional[Tuple[torch.Tensor]] = None,
                mid_block_additional_residual: Optional[torch.Tensor] = None,
                down_intrablock_additional_residuals=None, encoder_attention_mask=None, return_dict: bool = True,
                down_block_add_samples: Optional[List[torch.Tensor]] = None,
                mid_block_add_sample: Optional[torch.Tensor] = None,
                up_block_add_samples: Optional[List[torch.Tensor]] = None, **kwargs):
        for name, v in (("class_labels", class_labels), ("attention_mask", attention_mask), ("encoder_attention_mask", encoder_attention_mask),
                        ("down_intrablock_additional_residuals", down_intrablock_additional_residuals)):
            if v is not None:
                raise NotImplementedError(f"{name} is outside the PowerPaint hot path (never set by the pipelines)")
        # LoRA scale (unet_2d_condition.py:1192-1195 of the reference): folded into the packed weights before the step
        # runs; with no adapter loaded a scale is a no-op, as in the reference
        self.merge_adapters((cross_attention_kwargs or {}).get("scale", 1.0))
        rt = self.prepare(tuple(sample.shape), encoder_hidden_states, down_block_add_samples, mid_block_add_sample,
                          up_block_add_samples, down_block_additional_residuals, mid_block_additional_residual,
                          timestep_cond=timestep_cond, added_cond_kwargs=added_cond_kwargs,
                          ip_adapter_masks=(cross_attention_kwargs or {}).get("ip_adapter_masks"))
        # the reference consumes the BrushNet lists destructively (.pop(0), unet_2d_condition.py:1223,1234,1318)
        for lst in (down_block_add_samples, up_block_add_samples):
            if isinstance(lst, list):
                del lst[:]
        rt.load_input([(sample, 0)])
        rt.set_timestep(timestep)
        rt.run_step()
        out = rt.eps_tensor().to(self._dtype)
        if not return_dict:
            return (out,)
        return Output(sample=out)

    __call__ = forward
