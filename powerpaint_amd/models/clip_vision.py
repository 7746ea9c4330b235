"""CLIPVisionModelWithProjection on the MI355X HIP path: the `image_encoder` of an IP-Adapter pipeline.

Drop-in for `transformers.CLIPVisionModelWithProjection` as `encode_image` uses it (`image_encoder(pixel_values).image_embeds`,
`next(image_encoder.parameters()).dtype`).  It IS an nn.Module whose parameter tree has transformers' names --
`vision_model.embeddings.{class_embedding, patch_embedding.weight, position_embedding.weight}`, `vision_model.pre_layrnorm`
(transformers' spelling), `vision_model.encoder.layers.{i}.{self_attn.{q,k,v,out}_proj, layer_norm1, mlp.fc1, mlp.fc2,
layer_norm2}`, `vision_model.post_layernorm`, `visual_projection.weight` -- so `state_dict()`, `load_state_dict()`,
`safetensors.torch.load_model` and `.to()` work on it unchanged; the sub-modules are parameter containers only (fp32 masters).
`forward` repacks the parameters into the kernels' layout when they changed and replays `powerpaint_amd.clip_vision`'s launch
plan, in bf16 whatever the pipeline's dtype (as the text tower does).
"""
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn

from .. import _lib as L
from ..clip_vision import CLIPVisionNet, CLIPVisionRuntime
from ..loaders import PretrainedMixin
from ._base import Output
from .clip_text import _Encoder


class _VisionEmbeddings(nn.Module):
    def __init__(self, c, patch, npos):
        super().__init__()
        self.class_embedding = nn.Parameter(torch.zeros(c))
        self.patch_embedding = nn.Conv2d(3, c, kernel_size=patch, stride=patch, bias=False)
        self.position_embedding = nn.Embedding(npos, c)


class _VisionTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        npos = (cfg.image_size // cfg.patch_size) ** 2 + 1
        self.embeddings = _VisionEmbeddings(cfg.hidden_size, cfg.patch_size, npos)
        self.pre_layrnorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)
        self.encoder = _Encoder(cfg.num_hidden_layers, cfg.hidden_size, cfg.intermediate_size, cfg.layer_norm_eps)
        self.post_layernorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class CLIPVisionModelWithProjection(nn.Module, PretrainedMixin):
    def __init__(self, config=None, device="cuda", **kw):
        super().__init__()
        d = dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=16, num_channels=3,
                 image_size=224, patch_size=14, hidden_act="gelu", layer_norm_eps=1e-5, projection_dim=1024)
        if config is not None:
            d.update({k: getattr(config, k) for k in d if hasattr(config, k)})
        vc = kw.get("vision_config")                 # (a full CLIPConfig's config.json nests the tower's keys)
        if isinstance(vc, dict):
            d.update({k: vc[k] for k in d if k in vc})
        d.update({k: v for k, v in kw.items() if k in d})
        self.config = SimpleNamespace(**d)
        c = self.config
        # configs the kernels cannot run are refused by name (a swallowed key would load, run and give wrong embeddings)
        if c.hidden_act != "gelu":
            raise L.PPError(f"CLIPVisionModelWithProjection: config hidden_act={c.hidden_act!r} is not implemented on the HIP path "
                            f"(supported: 'gelu', the exact-erf GELU of the ViT-H/14 image encoder)")
        if c.num_channels != 3:
            raise L.PPError(f"CLIPVisionModelWithProjection: config num_channels={c.num_channels!r} is not implemented on the HIP "
                            f"path (supported: 3)")
        self.net = CLIPVisionNet(c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads, c.image_size,
                                 c.patch_size, c.projection_dim, c.layer_norm_eps)
        self.vision_model = _VisionTransformer(c)
        self.visual_projection = nn.Linear(c.hidden_size, c.projection_dim, bias=False)
        self._rt: Optional[CLIPVisionRuntime] = None
        self._stamp = None
        self.requires_grad_(False)
        self.to(device)

    @property
    def device(self):
        return self.visual_projection.weight.device

    @property
    def dtype(self):
        return self.visual_projection.weight.dtype

    # ---- checkpoints: transformers 4.x names (`vision_model.` prefix) and 5.x names (the tower's keys without it)
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        sd = {}
        for k, v in state_dict.items():
            if k.endswith("position_ids"):
                continue
            if not k.startswith("vision_model.") and not k.startswith("visual_projection."):
                k = "vision_model." + k
            sd[k] = v
        return super().load_state_dict(sd, strict=strict, assign=assign)

    def _params_stamp(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _ensure_packed(self):
        dev = self.device
        if dev.type != "cuda":
            raise L.PPError("CLIPVisionModelWithProjection: parameters must live on the GPU (no CPU path)")
        stamp = self._params_stamp()
        if stamp != self._stamp or self._rt is None or self._rt.device != dev:
            sd = {(n[len("vision_model."):] if n.startswith("vision_model.") else n): p for n, p in self.named_parameters()}
            self.net.pack(sd, dev)
            self._rt = CLIPVisionRuntime(self.net, dev)
            self._stamp = stamp

    @torch.no_grad()
    def forward(self, pixel_values: Optional[torch.Tensor] = None, output_attentions=None, output_hidden_states=None,
                interpolate_pos_encoding: bool = False, return_dict: Optional[bool] = True, **unused):
        if pixel_values is None:
            raise ValueError("You have to specify pixel_values")
        if output_attentions or interpolate_pos_encoding:
            raise NotImplementedError("output_attentions / interpolate_pos_encoding are not used by the pipelines")
        if pixel_values.dim() != 4 or pixel_values.shape[1] != 3:
            raise ValueError(f"pixel_values must be [B, 3, H, W], got {tuple(pixel_values.shape)}")
        self._ensure_packed()
        embeds = self._rt.run(pixel_values.to(self.device)).to(self.dtype)
        # (pre_layrnorm's output, layer 1, ..., layer N), as transformers returns them; last_hidden_state is the encoder's
        # output BEFORE post_layernorm, which transformers applies to the class token only
        hs = tuple(h.to(self.dtype) for h in self._rt.hidden_states()) if output_hidden_states else None
        last = hs[-1] if hs is not None else self._rt.hidden_states(last_only=True)[0].to(self.dtype)
        out = Output(image_embeds=embeds, last_hidden_state=last, hidden_states=hs)
        if not return_dict:
            return tuple(v for v in (out.image_embeds, out.last_hidden_state, out.hidden_states) if v is not None)
        return out
