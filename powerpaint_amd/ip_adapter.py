"""IP-Adapter (image prompts) for the UNet's HIP path: reading adapter files, checking them against the network, and the
host-side `ImageProjection` modules `unet.encoder_hid_proj.image_projection_layers` holds (DESIGN.md "IP-Adapter").

Follows the names of diffusers 0.27 (`IPAdapterMixin.load_ip_adapter`, `UNet2DConditionLoadersMixin._load_ip_adapter_weights`,
`ImageProjection`, `MultiIPAdapterImageProjection`, `IPAdapterAttnProcessor2_0`), which the reference's BrushNet pipeline calls
(pipeline_PowerPaint_Brushnet_CA.py:632-706).  Two families load: base adapters -- a Linear + LayerNorm image projection of
the pooled image embeds to T tokens -- and Plus adapters, whose image projection is the Resampler (diffusers-0.27
`IPAdapterPlusImageProjection`: Q latent queries attend over the tower's patch states and themselves, `depth` times); both
carry, per cross-attention, the bias-free pair to_k_ip / to_v_ip.  Files of the other families (FaceID, full-face) are refused
by the key that gives them away.  Nothing is ever downloaded.
"""
import os
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

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


class IPPlus(NamedTuple):
    """What SDNet.ip records for a Plus adapter (a base adapter's entry is the plain pair (T, D)): T = Q tokens per image,
    D = E, the width of the hidden states it takes; then the Resampler's own sizes."""
    T: int
    D: int
    dim: int
    out: int
    depth: int
    heads: int
    ff: int


RESAMPLER_HEAD_DIM = 64       # fixed by the file format: heads = to_q rows / 64


def plus_image_proj_shapes(Q: int, dim: int, E: int, out: int, depth: int, inner: int, ff: int) -> Dict[str, tuple]:
    """Every image_proj key of a Plus file with its shape."""
    shp = {"latents": (1, Q, dim), "proj_in.weight": (dim, E), "proj_in.bias": (dim,), "proj_out.weight": (out, dim),
           "proj_out.bias": (out,), "norm_out.weight": (out,), "norm_out.bias": (out,)}
    for i in range(depth):
        p = f"layers.{i}"
        shp.update({f"{p}.0.norm1.weight": (dim,), f"{p}.0.norm1.bias": (dim,), f"{p}.0.norm2.weight": (dim,),
                    f"{p}.0.norm2.bias": (dim,), f"{p}.0.to_q.weight": (inner, dim), f"{p}.0.to_kv.weight": (2 * inner, dim),
                    f"{p}.0.to_out.weight": (dim, inner), f"{p}.1.0.weight": (dim,), f"{p}.1.0.bias": (dim,),
                    f"{p}.1.1.weight": (ff, dim), f"{p}.1.3.weight": (dim, ff)})
    return shp


class _ResamplerAttention(nn.Module):
    def __init__(self, dim: int, heads: int):
        super().__init__()
        inner = heads * RESAMPLER_HEAD_DIM
        self.heads = heads
        self.to_q = nn.Linear(dim, inner, bias=False)
        self.to_k = nn.Linear(dim, inner, bias=False)
        self.to_v = nn.Linear(dim, inner, bias=False)
        self.to_out = nn.ModuleList([nn.Linear(inner, dim, bias=False)])

    def forward(self, latents, kv_in):
        N, Q, _ = latents.shape

        def split(t):
            return t.view(N, t.shape[1], self.heads, RESAMPLER_HEAD_DIM).transpose(1, 2)

        q, k, v = split(self.to_q(latents)), split(self.to_k(kv_in)), split(self.to_v(kv_in))
        p = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * RESAMPLER_HEAD_DIM ** -0.5, dim=-1)
        return self.to_out[0](torch.matmul(p, v).transpose(1, 2).reshape(N, Q, -1))


class _GELUProj(nn.Module):
    def __init__(self, dim: int, ff: int):
        super().__init__()
        self.proj = nn.Linear(dim, ff, bias=False)

    def forward(self, x):
        return torch.nn.functional.gelu(self.proj(x))


class _ResamplerFF(nn.Module):
    def __init__(self, dim: int, ff: int):
        super().__init__()
        self.net = nn.ModuleList([_GELUProj(dim, ff), nn.Identity(), nn.Linear(ff, dim, bias=False)])

    def forward(self, x):
        return self.net[2](self.net[0](x))


class IPAdapterPlusImageProjection(nn.Module):
    """The Resampler under diffusers-0.27's parameter names: hidden states x [N, S, E] -> Q tokens [N, Q, out].  Per layer i:
    layers.i.0 = LayerNorm over x, layers.i.1 = LayerNorm over the latents, layers.i.2 = the attention (to_q, to_k, to_v,
    to_out.0; keys = the S image rows, then the Q latent rows), layers.i.3 = (LayerNorm, FeedForward with net.0.proj, GELU
    (erf), net.2); no linear inside a layer has a bias.  Host side, fp32: on the HIP path the same arithmetic runs in the
    UNet's setup plan (SDNet.build_setup)."""

    def __init__(self, embed_dims: int = 768, output_dims: int = 1024, hidden_dims: int = 1280, depth: int = 4,
                 heads: int = 16, num_queries: int = 8, ffn_dim: int = 0):
        super().__init__()
        ffn_dim = ffn_dim or 4 * hidden_dims
        self.latents = nn.Parameter(torch.randn(1, num_queries, hidden_dims) / hidden_dims ** 0.5)
        self.proj_in = nn.Linear(embed_dims, hidden_dims)
        self.proj_out = nn.Linear(hidden_dims, output_dims)
        self.norm_out = nn.LayerNorm(output_dims)
        self.layers = nn.ModuleList([
            nn.ModuleList([nn.LayerNorm(hidden_dims), nn.LayerNorm(hidden_dims), _ResamplerAttention(hidden_dims, heads),
                           nn.Sequential(nn.LayerNorm(hidden_dims), _ResamplerFF(hidden_dims, ffn_dim))])
            for _ in range(depth)])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        latents = self.latents.repeat(x.shape[0], 1, 1)
        x = self.proj_in(x)
        for ln0, ln1, attn, ff in self.layers:
            ln = ln1(latents)
            latents = attn(ln, torch.cat([ln0(x), ln], dim=1)) + latents
            latents = ff(latents) + latents
        return self.norm_out(self.proj_out(latents))


def plus_key_conversion(depth: int) -> Dict[str, str]:
    """file key (image_proj.*) -> diffusers-0.27 parameter name; `to_kv` maps to to_k (first half of the rows) and is
    listed under the to_k name (the to_v half is f"layers.{i}.2.to_v.weight")."""
    m = {k: k for k in ("latents", "proj_in.weight", "proj_in.bias", "proj_out.weight", "proj_out.bias", "norm_out.weight",
                        "norm_out.bias")}
    for i in range(depth):
        f, t = f"layers.{i}", f"layers.{i}"
        for wb in ("weight", "bias"):
            m[f"{f}.0.norm1.{wb}"] = f"{t}.0.{wb}"
            m[f"{f}.0.norm2.{wb}"] = f"{t}.1.{wb}"
            m[f"{f}.1.0.{wb}"] = f"{t}.3.0.{wb}"
        m[f"{f}.0.to_q.weight"] = f"{t}.2.to_q.weight"
        m[f"{f}.0.to_kv.weight"] = f"{t}.2.to_k.weight"
        m[f"{f}.0.to_out.weight"] = f"{t}.2.to_out.0.weight"
        m[f"{f}.1.1.weight"] = f"{t}.3.1.net.0.proj.weight"
        m[f"{f}.1.3.weight"] = f"{t}.3.1.net.2.weight"
    return m


class MultiIPAdapterImageProjection(nn.Module):
    """One projection per adapter over a list of embeds -- [B, n, D] for a base layer, [B, n, S, E] for a Plus layer, reshaped
    as diffusers does, (B n,) + shape[2:] -- : the n images' tokens side by side, [B, n T, ctx] each.
    On the HIP path the same arithmetic runs in the UNet's setup plan (SDNet.build_setup); this module is what
    `unet.encoder_hid_proj` shows to callers (and what the pipeline's length / type checks look at)."""

    def __init__(self, layers: Sequence[nn.Module]):
        super().__init__()
        self.image_projection_layers = nn.ModuleList(layers)

    def forward(self, image_embeds: List[torch.Tensor]) -> List[torch.Tensor]:
        check_image_embeds(image_embeds, len(self.image_projection_layers),
                           [isinstance(m, IPAdapterPlusImageProjection) for m in self.image_projection_layers])
        out = []
        for e, layer in zip(image_embeds, self.image_projection_layers):
            B, n = e.shape[0], e.shape[1]
            y = layer(e.reshape((B * n,) + tuple(e.shape[2:])))
            out.append(y.reshape(B, n * y.shape[1], -1))
        return out


def check_image_embeds(image_embeds, n_adapters: int, plus: Optional[Sequence[bool]] = None):
    """plus: per adapter, is it a Plus adapter (4-D embeds [B, n, S, E]); None = base adapters only."""
    if not isinstance(image_embeds, (list, tuple)):
        raise ValueError(f"image_embeds must be a list of [B, n, D] tensors (one per IP-Adapter), got {type(image_embeds)}")
    if len(image_embeds) != n_adapters:
        raise ValueError(f"image_embeds must have the same length as the number of IP-Adapters: got {len(image_embeds)} "
                         f"tensors and {n_adapters} IP-Adapters")
    for i, e in enumerate(image_embeds):
        if plus is not None and plus[i]:
            if not torch.is_tensor(e) or e.dim() != 4:
                raise ValueError(f"image_embeds[{i}] belongs to an IP-Adapter Plus and must be a 4-D tensor [B, n, S, E] (the image "
                                 f"encoder's hidden_states[-2] per image), got "
                                 f"{tuple(e.shape) if torch.is_tensor(e) else type(e)}")
        elif not torch.is_tensor(e) or e.dim() != 3:
            if plus is not None and torch.is_tensor(e) and e.dim() == 4:
                raise ValueError(f"image_embeds[{i}] belongs to a base IP-Adapter and must be a 3-D tensor [B, n, D] (pooled image "
                                 f"embeds), got the 4-D {tuple(e.shape)} of an IP-Adapter Plus")
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
        if k.startswith("perceiver_resampler."):
            raise L.PPError(f"{where}: image_proj key {k!r} belongs to an IP-Adapter FaceID (Plus) file; base and Plus adapters "
                            f"run on the HIP path, FaceID adapters do not")
        if k.startswith("proj.0.") or k.startswith("proj.2."):
            raise L.PPError(f"{where}: image_proj key {k!r} belongs to an IP-Adapter full-face file (or FaceID): its 257 tokens "
                            f"per image exceed the {L.PP_IP_MAX_TOKENS} the kernel takes; base and Plus adapters run on the HIP "
                            f"path")
    for k in ad:
        if "lora" in k:
            raise L.PPError(f"{where}: ip_adapter key {k!r} belongs to an IP-Adapter FaceID file (LoRA terms); base and Plus "
                            f"adapters run on the HIP path, FaceID adapters do not")
    ctx = net.ctx_dim
    if "latents" in ip:
        out = _check_plus_image_proj(ip, ctx, where)
    else:
        for k in ip:
            if k.startswith("proj_in.") or k.startswith("layers.") or k.startswith("proj_out.") or k.startswith("norm_out."):
                raise L.PPError(f"{where}: image_proj key {k!r} belongs to an IP-Adapter Plus (Resampler) file, but its `latents` "
                                f"are missing")
        missing = [k for k in IMAGE_PROJ_KEYS if k not in ip]
        surplus = [k for k in ip if k not in IMAGE_PROJ_KEYS]
        if missing or surplus:
            raise L.PPError(f"{where}: image_proj must hold exactly {list(IMAGE_PROJ_KEYS)}: missing {missing}, surplus {surplus}")
        w = ip["proj.weight"]
        if w.dim() != 2 or w.shape[0] % ctx or w.shape[0] == 0:
            raise L.PPError(f"{where}: image_proj proj.weight has shape {tuple(w.shape)}; expected [T * {ctx}][D]")
        T, D = w.shape[0] // ctx, w.shape[1]
        if T > L.PP_IP_MAX_TOKENS:
            raise L.PPError(f"{where}: image_proj proj.weight gives {T} tokens per image, the kernel takes {L.PP_IP_MAX_TOKENS}")
        for k, shp in (("proj.bias", (T * ctx,)), ("norm.weight", (ctx,)), ("norm.bias", (ctx,))):
            if tuple(ip[k].shape) != shp:
                raise L.PPError(f"{where}: image_proj {k} has shape {tuple(ip[k].shape)}, expected {shp}")
        out = {k: ip[k].detach().float().cpu() for k in IMAGE_PROJ_KEYS}
        out["kind"], out["T"], out["D"] = "base", T, D
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
    out["kv"] = {pre: (a.detach().float().cpu(), b.detach().float().cpu()) for pre, (a, b) in kv.items()}
    return out


def _check_plus_image_proj(ip: Dict[str, torch.Tensor], ctx: int, where: str) -> Dict[str, object]:
    """The image_proj half of a Plus (Resampler) file: every key and shape of the format, the sizes derived from them."""
    fam = "IP-Adapter Plus (Resampler)"
    for k in ("latents", "proj_in.weight", "proj_out.weight"):
        if k not in ip:
            raise L.PPError(f"{where}: image_proj key 'latents' marks an {fam} file, which lacks image_proj key {k!r}")
    lat, w_in, w_out = ip["latents"], ip["proj_in.weight"], ip["proj_out.weight"]
    if lat.dim() != 3 or lat.shape[0] != 1 or w_in.dim() != 2 or w_out.dim() != 2:
        raise L.PPError(f"{where}: {fam}: latents {tuple(lat.shape)}, proj_in.weight {tuple(w_in.shape)}, proj_out.weight "
                        f"{tuple(w_out.shape)}; expected [1, Q, dim], [dim, E], [out, dim]")
    Q, dim, E, out_dim = lat.shape[1], lat.shape[2], w_in.shape[1], w_out.shape[0]
    depth = 1 + max([int(k.split(".")[1]) for k in ip if k.startswith("layers.") and k.split(".")[1].isdigit()], default=-1)
    if depth < 1:
        raise L.PPError(f"{where}: {fam} file without image_proj layers.* keys")
    for k in ("layers.0.0.to_q.weight", "layers.0.1.1.weight"):
        if k not in ip or ip[k].dim() != 2:
            raise L.PPError(f"{where}: {fam} file without a 2-D image_proj key {k!r}")
    inner, ff = ip["layers.0.0.to_q.weight"].shape[0], ip["layers.0.1.1.weight"].shape[0]
    want = plus_image_proj_shapes(Q, dim, E, out_dim, depth, inner, ff)
    missing = [k for k in want if k not in ip]
    surplus = [k for k in ip if k not in want]
    if missing or surplus:
        raise L.PPError(f"{where}: {fam}: image_proj keys do not match a Resampler of depth {depth}: missing {missing[:4]}"
                        f"{'...' if len(missing) > 4 else ''}, surplus {surplus[:4]}{'...' if len(surplus) > 4 else ''}")
    for k, shp in want.items():
        if tuple(ip[k].shape) != shp:
            raise L.PPError(f"{where}: {fam}: image_proj {k} has shape {tuple(ip[k].shape)}, expected {shp}")
    if out_dim != ctx:
        raise L.PPError(f"{where}: {fam}: proj_out gives tokens of width out = {out_dim}, the UNet's cross-attention takes {ctx}")
    if inner % RESAMPLER_HEAD_DIM:
        raise L.PPError(f"{where}: {fam}: to_q gives inner = {inner} channels, not a multiple of the format's head dimension "
                        f"{RESAMPLER_HEAD_DIM}")
    for name, v in (("dim", dim), ("inner", inner), ("ff", ff)):       # (E is zero-padded to 64 where it is packed, as a base D)
        if v % 64:
            raise L.PPError(f"{where}: {fam}: {name} = {v} is not a multiple of 64 (the GEMM contracts 64 at a time)")
    if Q > L.PP_IP_MAX_TOKENS:
        raise L.PPError(f"{where}: {fam}: latents give Q = {Q} tokens per image, the kernel takes {L.PP_IP_MAX_TOKENS}")
    out: Dict[str, object] = {k: ip[k].detach().float().cpu() for k in want}
    out["kind"], out["T"], out["D"] = "plus", Q, E
    out["plus"] = IPPlus(Q, E, dim, out_dim, depth, inner // RESAMPLER_HEAD_DIM, ff)
    return out


def plus_projection_module(ad: Dict[str, object]) -> IPAdapterPlusImageProjection:
    """The host-side IPAdapterPlusImageProjection filled from a checked Plus adapter (`to_kv` split in halves)."""
    sp: IPPlus = ad["plus"]
    m = IPAdapterPlusImageProjection(embed_dims=sp.D, output_dims=sp.out, hidden_dims=sp.dim, depth=sp.depth, heads=sp.heads,
                                     num_queries=sp.T, ffn_dim=sp.ff)
    sd = {}
    inner = sp.heads * RESAMPLER_HEAD_DIM
    for fk, dk in plus_key_conversion(sp.depth).items():
        if fk.endswith("to_kv.weight"):
            sd[dk], sd[dk.replace("to_k.", "to_v.")] = ad[fk][:inner].clone(), ad[fk][inner:].clone()
        else:
            sd[dk] = ad[fk].clone()
    m.load_state_dict(sd, strict=True)
    return m.eval()


def projection_module(ad: Dict[str, object], ctx: int) -> nn.Module:
    """The host-side ImageProjection / IPAdapterPlusImageProjection carrying an adapter's loaded weights."""
    if ad.get("kind") == "plus":
        return plus_projection_module(ad)
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
