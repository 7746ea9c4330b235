"""IP-Adapter (image prompts) for the UNet's HIP path: reading adapter files, checking them against the network, and the
host-side `ImageProjection` modules `unet.encoder_hid_proj.image_projection_layers` holds (DESIGN.md "IP-Adapter").

Follows the names of diffusers 0.27 (`IPAdapterMixin.load_ip_adapter`, `UNet2DConditionLoadersMixin._load_ip_adapter_weights`,
`ImageProjection`, `MultiIPAdapterImageProjection`, `IPAdapterAttnProcessor2_0`), which the reference's BrushNet pipeline calls
(pipeline_PowerPaint_Brushnet_CA.py:632-706).  Base adapters only: a Linear + LayerNorm image projection to T tokens and, per
cross-attention, the bias-free pair to_k_ip / to_v_ip.  Files of the other families (Plus / Resampler, FaceID) are refused by
the key that gives them away.  Nothing is ever downloaded.
"""
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib as L

IMAGE_PROJ_KEYS = ("proj.weight", "proj.bias", "norm.weight", "norm.bias")


class ImageProjection(nn.Module):
    """image_embeds [B, D] -> LayerNorm(Linear(D -> T * ctx)(image_embeds).reshape(B, T, ctx))."""

    def __init__(self, image_embed_dim: int = 768, cross_attention_dim: int = 768, num_image_text_embeds: int = 32):
        super().__init__()
        self.num_image_text_embeds = num_image_text_embeds
        self.image_embeds = nn.Linear(image_embed_dim, num_image_text_embeds * cross_attention_dim)
        self.norm = nn.LayerNorm(cross_attention_dim)

    def forward(self, image_embeds: torch.Tensor) -> torch.Tensor:
        y = self.image_embeds(image_embeds)
        return self.norm(y.reshape(image_embeds.shape[0], self.num_image_text_embeds, -1))


class MultiIPAdapterImageProjection(nn.Module):
    """One projection per adapter over a list of [B, n, D] embeds: the n images' tokens side by side, [B, n T, ctx] each.
    On the HIP path the same arithmetic runs in the UNet's setup plan (SDNet.build_setup); this module is what
    `unet.encoder_hid_proj` shows to callers (and what the pipeline's length / type checks look at)."""

    def __init__(self, layers: Sequence[nn.Module]):
        super().__init__()
        self.image_projection_layers = nn.ModuleList(layers)

    def forward(self, image_embeds: List[torch.Tensor]) -> List[torch.Tensor]:
        check_image_embeds(image_embeds, len(self.image_projection_layers))
        out = []
        for e, layer in zip(image_embeds, self.image_projection_layers):
            B, n = e.shape[0], e.shape[1]
            y = layer(e.reshape(B * n, -1))
            out.append(y.reshape(B, n * y.shape[1], -1))
        return out


def check_image_embeds(image_embeds, n_adapters: int):
    if not isinstance(image_embeds, (list, tuple)):
        raise ValueError(f"image_embeds must be a list of [B, n, D] tensors (one per IP-Adapter), got {type(image_embeds)}")
    if len(image_embeds) != n_adapters:
        raise ValueError(f"image_embeds must have the same length as the number of IP-Adapters: got {len(image_embeds)} "
                         f"tensors and {n_adapters} IP-Adapters")
    for e in image_embeds:
        if not torch.is_tensor(e) or e.dim() != 3:
            raise ValueError("every entry of image_embeds must be a 3-D tensor [B, n, D]")


def _split_prefixed(sd: Dict[str, torch.Tensor], where: str) -> Dict[str, Dict[str, torch.Tensor]]:
    out = {"image_proj": {}, "ip_adapter": {}}
    for k, v in sd.items():
        if k.startswith("image_proj."):
            out["image_proj"][k[len("image_proj."):]] = v
        elif k.startswith("ip_adapter."):
            out["ip_adapter"][k[len("ip_adapter."):]] = v
        else:
            raise L.PPError(f"{where}: key {k!r} is neither image_proj.* nor ip_adapter.*: not an IP-Adapter file")
    return out


def read_ip_adapter(src, subfolder: Optional[str] = None, weight_name: Optional[str] = None) -> Dict[str, dict]:
    """One adapter as {"image_proj": {...}, "ip_adapter": {...}}: from that dict, from a .bin holding it, or from a
    .safetensors with `image_proj.` / `ip_adapter.` key prefixes.  `src` is a dict, a file, or a folder (then
    [subfolder/]weight_name names the file).  Local paths only."""
    if isinstance(src, dict):
        if set(src) == {"image_proj", "ip_adapter"} and all(isinstance(v, dict) for v in src.values()):
            return {"image_proj": dict(src["image_proj"]), "ip_adapter": dict(src["ip_adapter"])}
        if src and all(isinstance(k, str) and torch.is_tensor(v) for k, v in src.items()):
            return _split_prefixed(src, "state dict")
        raise L.PPError("an IP-Adapter state dict is {'image_proj': {...}, 'ip_adapter': {...}} (or flat with those prefixes); "
                        f"got keys {sorted(map(str, src))[:6]}")
    path = str(src)
    if os.path.isdir(path):
        if not weight_name:
            raise L.PPError(f"{path} is a folder: name the adapter file with weight_name=")
        path = os.path.join(path, subfolder or "", weight_name)
    if not os.path.isfile(path):
        raise L.PPError(f"IP-Adapter file {path} does not exist (local paths and state dicts only: nothing is downloaded)")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return _split_prefixed(load_file(path, device="cpu"), path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise L.PPError(f"{path}: not a state dict")
    return read_ip_adapter(sd)


def check_ip_adapter(net, sd: Dict[str, dict], where: str = "IP-Adapter") -> Dict[str, object]:
    """Validate one adapter against the SDNet `net` and bring it into the form SDNet.set_ip_adapters takes.

    Index order.  The file numbers the UNet's attention processors, `"{i}.to_k_ip.weight"`, by their position in the reference
    UNet's `attn_processors` dict (unet_2d_condition.py:694): a depth-first walk over the module tree in registration order --
    `down_blocks` (:310-311), then `up_blocks` (:381), then `mid_block` (assigned after both) -- with attn1 before attn2 inside
    every transformer block.  Self-attentions carry no weights, so cross-attention k (k = 0, 1, ... over down blocks, up
    blocks, mid block) is index 2 k + 1: 1, 3, .. 11 down, 13 .. 29 up, 31 mid for SD 1.5 (SDNet.ip_attn_order)."""
    ip, ad = sd["image_proj"], sd["ip_adapter"]
    for k in ip:
        if k == "latents" or k.startswith("proj_in.") or k.startswith("layers.") or k.startswith("proj_out.") or \
                k.startswith("norm_out."):
            raise L.PPError(f"{where}: image_proj key {k!r} belongs to an IP-Adapter Plus (Resampler) file; only base adapters "
                            f"(Linear + LayerNorm image projection) run on the HIP path")
        if k.startswith("proj.0.") or k.startswith("proj.2.") or k.startswith("perceiver_resampler."):
            raise L.PPError(f"{where}: image_proj key {k!r} belongs to an IP-Adapter FaceID / full file; only base adapters run "
                            f"on the HIP path")
    for k in ad:
        if "lora" in k:
            raise L.PPError(f"{where}: ip_adapter key {k!r} belongs to an IP-Adapter FaceID file (LoRA terms); only base "
                            f"adapters run on the HIP path")
    missing = [k for k in IMAGE_PROJ_KEYS if k not in ip]
    surplus = [k for k in ip if k not in IMAGE_PROJ_KEYS]
    if missing or surplus:
        raise L.PPError(f"{where}: image_proj must hold exactly {list(IMAGE_PROJ_KEYS)}: missing {missing}, surplus {surplus}")
    ctx = net.ctx_dim
    w = ip["proj.weight"]
    if w.dim() != 2 or w.shape[0] % ctx or w.shape[0] == 0:
        raise L.PPError(f"{where}: image_proj proj.weight has shape {tuple(w.shape)}; expected [T * {ctx}][D]")
    T, D = w.shape[0] // ctx, w.shape[1]
    if T > L.PP_IP_MAX_TOKENS:
        raise L.PPError(f"{where}: image_proj proj.weight gives {T} tokens per image, the kernel takes {L.PP_IP_MAX_TOKENS}")
    for k, shp in (("proj.bias", (T * ctx,)), ("norm.weight", (ctx,)), ("norm.bias", (ctx,))):
        if tuple(ip[k].shape) != shp:
            raise L.PPError(f"{where}: image_proj {k} has shape {tuple(ip[k].shape)}, expected {shp}")
    order = net.ip_attn_order()
    width = dict(net._attn_specs())
    want = {f"{2 * k + 1}.{n}.weight": (pre, n) for k, pre in enumerate(order) for n in ("to_k_ip", "to_v_ip")}
    missing = [k for k in want if k not in ad]
    surplus = [k for k in ad if k not in want]
    if missing or surplus:
        raise L.PPError(f"{where}: ip_adapter keys do not match the UNet's {len(order)} cross-attentions: missing "
                        f"{missing[:4]}{'...' if len(missing) > 4 else ''}, surplus {surplus[:4]}{'...' if len(surplus) > 4 else ''}")
    kv: Dict[str, List[Optional[torch.Tensor]]] = {pre: [None, None] for pre in order}
    for k, (pre, n) in want.items():
        if tuple(ad[k].shape) != (width[pre], ctx):
            raise L.PPError(f"{where}: ip_adapter {k} has shape {tuple(ad[k].shape)}, {pre} needs {(width[pre], ctx)}")
        kv[pre][0 if n == "to_k_ip" else 1] = ad[k]
    out: Dict[str, object] = {k: ip[k].detach().float().cpu() for k in IMAGE_PROJ_KEYS}
    out["kv"] = {pre: (a.detach().float().cpu(), b.detach().float().cpu()) for pre, (a, b) in kv.items()}
    out["T"], out["D"] = T, D
    return out


def projection_module(ad: Dict[str, object], ctx: int) -> ImageProjection:
    """The host-side ImageProjection carrying an adapter's loaded weights."""
    m = ImageProjection(image_embed_dim=ad["D"], cross_attention_dim=ctx, num_image_text_embeds=ad["T"])
    with torch.no_grad():
        m.image_embeds.weight.copy_(ad["proj.weight"])
        m.image_embeds.bias.copy_(ad["proj.bias"])
        m.norm.weight.copy_(ad["norm.weight"])
        m.norm.bias.copy_(ad["norm.bias"])
    return m.eval()


def scales_list(scale, n: int) -> Tuple[float, ...]:
    if isinstance(scale, (list, tuple)):
        if len(scale) != n:
            raise ValueError(f"`scale` should be a list of the same length as the number of IP-Adapters: got {len(scale)} scales "
                             f"and {n} IP-Adapters")
        return tuple(float(v) for v in scale)
    return (float(scale),) * n
