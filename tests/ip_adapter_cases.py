"""Shared by the IP-Adapter tests and the fixture generator (not a test file; nothing here is imported by the product).

IP-Adapter as the reference's BrushNet pipeline runs it (pipeline_PowerPaint_Brushnet_CA.py:632-706, 853-866, 1279-1290,
1363-1366, 1430-1441): `prepare_ip_adapter_image_embeds` makes one [B, n, D] tensor per adapter, the UNet's
`encoder_hid_proj` (diffusers-0.27 `MultiIPAdapterImageProjection` over `ImageProjection`s) turns them into image tokens and
hands every attention `encoder_hidden_states = (text, [tokens_0, ...])` (unet_2d_condition.py:1030-1037), and the attn2
processors (diffusers-0.27 `IPAdapterAttnProcessor2_0`) add one separately-softmaxed attention over each adapter's tokens.
diffusers is not a dependency of this repository, so the processor and the projections are RESTATED here from their
contract -- parity with the library is unpinned until tests/test_diffusers_pin_ip_adapter.py runs somewhere diffusers imports.

  * `IPAttention`: to_q / to_k / to_v / to_out of an oracle `Attention` plus `to_k_ip` / `to_v_ip` ModuleLists and `scale`;
    forward(x, ctx) with ctx = (text, [ip_0, ...]):  a = sdpa(q, K_text, V_text);  a += scale_i * sdpa(q, to_k_ip_i(ip_i),
    to_v_ip_i(ip_i)) per adapter;  to_out(a).
  * `install_ip_attention(unet, n)`: every attn2 of an oracle UNet becomes an IPAttention (BasicTransformerBlock.forward hands
    ctx through untouched); returns them in FILE order -- down blocks, up blocks, mid block.
  * `ImageProjection` / `MultiProjection`: Linear D -> T * 768, reshape [B, T, 768], LayerNorm; per adapter over [B, n, D]
    embeds with the n images' tokens side by side.
  * `IPUNet`: an oracle UNet with `encoder_hid_proj` and the `added_cond_kwargs["image_embeds"]` branch in front of it.
"""
import math
from types import SimpleNamespace

import torch
import torch.nn as nn

CTX = 768
EMBED_DIM = 32          # image-embed dimension of the fixture's adapters
TOKENS = 4              # tokens per image (base adapters)
W_STD = 0.5             # to_k_ip / to_v_ip ~ N(0, (W_STD / sqrt(768))^2): the image term is of the text term's size
ATOL, RTOL = 2e-4, 1e-4                 # CPU loop gate (tests/test_ksamplers.py)
LOOP_COS, LOOP_ERR = 0.9997, 4.5e-2     # GPU loop gate of the k-sampler tests: max-abs in units of max(1, max|ref|)
SEED = 5

# name -> (number of adapters, scales, images per prompt of each adapter, image prompt through the encoder?)
CASES = dict(one=dict(n=1, scales=[1.0], images=[1], encoder=False),
             two=dict(n=2, scales=[0.7, 0.4], images=[1, 2], encoder=False),
             image=dict(n=1, scales=[1.0], images=[1], encoder=True))


class IPAttention(nn.Module):
    def __init__(self, attn, n_adapters: int, ctx_dim: int = CTX):
        super().__init__()
        self.heads = attn.heads
        self.to_q, self.to_k, self.to_v, self.to_out = attn.to_q, attn.to_k, attn.to_v, attn.to_out
        inner = attn.to_q.out_features
        self.to_k_ip = nn.ModuleList([nn.Linear(ctx_dim, inner, bias=False) for _ in range(n_adapters)])
        self.to_v_ip = nn.ModuleList([nn.Linear(ctx_dim, inner, bias=False) for _ in range(n_adapters)])
        self.scale = [1.0] * n_adapters

    def _heads(self, t):
        B, N, _ = t.shape
        return t.view(B, N, self.heads, -1).transpose(1, 2)

    def _sdpa(self, q, k, v):
        s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(q.shape[-1])
        o = torch.matmul(torch.softmax(s, dim=-1), v)
        return o.transpose(1, 2).reshape(o.shape[0], o.shape[2], -1)

    def forward(self, x, ctx=None):
        text, ips = ctx
        q = self._heads(self.to_q(x))
        a = self._sdpa(q, self._heads(self.to_k(text)), self._heads(self.to_v(text)))
        for e, wk, wv, s in zip(ips, self.to_k_ip, self.to_v_ip, self.scale):
            a = a + s * self._sdpa(q, self._heads(wk(e)), self._heads(wv(e)))
        return self.to_out[0](a)


def cross_attention_blocks(unet):
    """The BasicTransformerBlocks of an oracle UNet in the order an adapter file numbers them: down, up, mid."""
    out = []
    for part in (unet.down_blocks, unet.up_blocks, [unet.mid_block]):
        for blk in part:
            for tr in (getattr(blk, "attentions", None) or []):
                out += list(tr.transformer_blocks)
    return out


def install_ip_attention(unet, n_adapters: int):
    mods = []
    for tb in cross_attention_blocks(unet):
        if not isinstance(tb.attn2, IPAttention):
            tb.attn2 = IPAttention(tb.attn2, n_adapters)
        mods.append(tb.attn2)
    return mods


class ImageProjection(nn.Module):
    def __init__(self, image_embed_dim=EMBED_DIM, cross_attention_dim=CTX, num_image_text_embeds=TOKENS):
        super().__init__()
        self.num_image_text_embeds = num_image_text_embeds
        self.image_embeds = nn.Linear(image_embed_dim, num_image_text_embeds * cross_attention_dim)
        self.norm = nn.LayerNorm(cross_attention_dim)

    def forward(self, image_embeds):
        y = self.image_embeds(image_embeds).reshape(image_embeds.shape[0], self.num_image_text_embeds, -1)
        return self.norm(y)


class MultiProjection(nn.Module):
    """Restated diffusers-0.27 MultiIPAdapterImageProjection: [B, n, D] per adapter -> [B, n T, ctx] per adapter."""

    def __init__(self, layers):
        super().__init__()
        self.image_projection_layers = nn.ModuleList(layers)

    def forward(self, image_embeds):
        out = []
        for e, layer in zip(image_embeds, self.image_projection_layers):
            B, n = e.shape[0], e.shape[1]
            y = layer(e.reshape((B * n,) + tuple(e.shape[2:])))
            out.append(y.reshape((B, n * y.shape[1]) + tuple(y.shape[2:])))
        return out


def bf16_round(t):
    return t.to(torch.bfloat16).float()


def adapter_state_dict(unet, seed: int, tokens: int = TOKENS, embed_dim: int = EMBED_DIM, std: float = W_STD):
    """A base adapter in file form for the oracle UNet's architecture: {"image_proj": {...}, "ip_adapter": {"{2k+1}.to_k_ip.weight",
    ...}}, matrices rounded to bf16 (what the HIP path stores), seeded."""
    g = torch.Generator().manual_seed(seed)
    ip = {"proj.weight": bf16_round(torch.randn(tokens * CTX, embed_dim, generator=g) / math.sqrt(embed_dim)),
          "proj.bias": 0.1 * torch.randn(tokens * CTX, generator=g),
          "norm.weight": 1.0 + 0.1 * torch.randn(CTX, generator=g), "norm.bias": 0.05 * torch.randn(CTX, generator=g)}
    ad = {}
    for k, tb in enumerate(cross_attention_blocks(unet)):
        c = tb.attn2.to_q.out_features
        for n in ("to_k_ip", "to_v_ip"):
            ad[f"{2 * k + 1}.{n}.weight"] = bf16_round(torch.randn(c, CTX, generator=g) * (std / math.sqrt(CTX)))
    return {"image_proj": ip, "ip_adapter": ad}


def load_into_oracle(unet, state_dicts, scales):
    """install_ip_attention + the adapters' weights -> (the projection module, the IPAttention modules)."""
    mods = install_ip_attention(unet, len(state_dicts))
    layers = []
    with torch.no_grad():
        for i, sd in enumerate(state_dicts):
            ip = sd["image_proj"]
            T = ip["proj.weight"].shape[0] // CTX
            lay = ImageProjection(ip["proj.weight"].shape[1], CTX, T)
            lay.image_embeds.weight.copy_(ip["proj.weight"]); lay.image_embeds.bias.copy_(ip["proj.bias"])
            lay.norm.weight.copy_(ip["norm.weight"]); lay.norm.bias.copy_(ip["norm.bias"])
            layers.append(lay.eval())
            for k, m in enumerate(mods):
                m.to_k_ip[i].weight.copy_(sd["ip_adapter"][f"{2 * k + 1}.to_k_ip.weight"])
                m.to_v_ip[i].weight.copy_(sd["ip_adapter"][f"{2 * k + 1}.to_v_ip.weight"])
    for m in mods:
        m.scale = [float(s) for s in scales]
    return MultiProjection(layers).eval(), mods


def forward_any_size(unet, sample, timestep, ctx):
    """The oracle UNet's plain forward pass with `upsample_size` handed to every up block but the last (the size of the skip
    tensor the next block pops: `forward_upsample_size` of the reference, unet_2d_condition.py:1120-1126,1311-1312).  The oracle's
    own forward does not pass it and cannot run latent sizes with an odd level; at even sizes the two are the same arithmetic
    (checked in tests/test_ip_adapter.py)."""
    import torch.nn.functional as F
    from oracle import sd_modules as OM
    emb = OM._time_embed(unet, sample, timestep)
    h = unet.conv_in(sample)
    res = (h,)
    for blk in unet.down_blocks:
        h, r = blk(h, emb, ctx)
        res += r
    h = unet.mid_block(h, emb, ctx)
    for i, blk in enumerate(unet.up_blocks):
        n = len(blk.resnets)
        r, res = res[-n:], res[:-n]
        size = tuple(res[-1].shape[2:]) if i != len(unet.up_blocks) - 1 else None
        h = blk(h, r, emb, ctx, upsample_size=size)
    return (unet.conv_out(F.silu(unet.conv_norm_out(h))),)


class IPUNet(nn.Module):
    """An oracle UNet whose attn2s are IPAttentions, behind the `ip_image_proj` branch of the reference UNet's
    process_encoder_hidden_states (unet_2d_condition.py:1030-1037)."""

    def __init__(self, unet, state_dicts, scales):
        super().__init__()
        self.unet = unet
        self.encoder_hid_proj, self.ip_modules = load_into_oracle(unet, state_dicts, scales)
        self.config = SimpleNamespace(**vars(unet.config))
        self.config.encoder_hid_dim_type = "ip_image_proj"

    @property
    def dtype(self):
        return self.unet.dtype

    @property
    def device(self):
        return self.unet.device

    def forward(self, sample, timestep, encoder_hidden_states, added_cond_kwargs=None, **kw):
        if added_cond_kwargs is None or "image_embeds" not in added_cond_kwargs:
            raise ValueError("`image_embeds` missing from added_cond_kwargs")
        ctx = (encoder_hidden_states, self.encoder_hid_proj(added_cond_kwargs["image_embeds"]))
        if not kw:
            return forward_any_size(self.unet, sample, timestep, ctx)
        return self.unet(sample, timestep, ctx, **kw)


class PlainTupleUNet(nn.Module):
    """The adapter-free UNet of the same call: ignores the image prompt (what a no-op implementation would compute)."""

    def __init__(self, unet):
        super().__init__()
        self.unet, self.config = unet, unet.config
        self.encoder_hid_proj = None

    dtype = property(lambda s: s.unet.dtype)
    device = property(lambda s: s.unet.device)

    def forward(self, sample, timestep, encoder_hidden_states, added_cond_kwargs=None, **kw):
        return self.unet(sample, timestep, encoder_hidden_states, **kw)


class TinyImageEncoder(nn.Module):
    """Stand-in `image_encoder` of case `image`: [B, 3, 8, 8] pixel tensors -> .image_embeds [B, EMBED_DIM]."""

    def __init__(self, seed: int = 77):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.proj = nn.Linear(3 * 8 * 8, EMBED_DIM)
        with torch.no_grad():
            self.proj.weight.copy_(torch.randn(EMBED_DIM, 192, generator=g) / math.sqrt(192))
            self.proj.bias.copy_(0.1 * torch.randn(EMBED_DIM, generator=g))

    def forward(self, image, **kw):
        return SimpleNamespace(image_embeds=self.proj(image.flatten(1)))


def case_adapters(unet, name):
    c = CASES[name]
    return [adapter_state_dict(unet, 900 + 10 * i + len(name)) for i in range(c["n"])]


def case_prompt(name, variant: int = 0):
    """The image prompt of a fixture case: precomputed embeds (a list of [2, n, D]: negative half, positive half) or the pixel
    tensor for the stand-in encoder.  variant 1: other values (the second call of the per-call-state test)."""
    c = CASES[name]
    g = torch.Generator().manual_seed(4000 + 17 * variant + len(name))
    if c["encoder"]:
        return dict(ip_adapter_image=torch.randn(1, 3, 8, 8, generator=g))
    embeds = []
    for n in c["images"]:
        pos = torch.randn(1, n, EMBED_DIM, generator=g)
        neg = 0.3 * torch.randn(1, n, EMBED_DIM, generator=g)
        embeds.append(torch.cat([neg, pos]))
    return dict(ip_adapter_image_embeds=embeds)


def loop_gate(out, ref):
    out, ref = out.float().cpu(), ref.float()
    cos = torch.nn.functional.cosine_similarity(out.flatten(), ref.flatten(), dim=0).item()
    err = (out - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    return cos, err, bool(cos >= LOOP_COS and err <= LOOP_ERR)


def net_gate(out, ref, dtype):
    """The project's network gates (tests/test_golden.py, tests/test_fp16_gpu.py)."""
    out, ref = out.float().cpu(), ref.float()
    cos = torch.nn.functional.cosine_similarity(out.flatten(), ref.flatten(), dim=0).item()
    err = (out - ref).abs().max().item()
    if dtype == torch.bfloat16:
        return cos, err, bool(cos >= 0.999 and err <= 3e-2 * max(1.0, ref.abs().max().item()))
    return cos, err, bool(cos >= 0.99999 and err <= 7.5e-3)


# ---------------------------------------------------------------------------------------------------------------- kernel
KERNEL_HEADS_D = [(8, 40), (8, 80), (8, 160), (1, 40)]
KERNEL_NQ = [1, 64, 100]
KERNEL_NK = [1, 4, 8, 16]
U32 = 2.0 ** -24


def kernel_inputs(batch, heads, d, nq, nk, dtype, ldq=None, ldo=None, seed=0, logit=None):
    """q [batch * nq][ldq], k / v [batch][nk][C], o [batch * nq + guard][ldo] in `dtype`; distinct K / V per batch item.  logit:
    scale q and k so that |qk_scale * q . k| reaches about that value."""
    C = heads * d
    ldq, ldo = ldq or C, ldo or C
    g = torch.Generator().manual_seed(1234 + seed)
    q = torch.randn(batch * nq, ldq, generator=g)
    k = torch.randn(batch, nk, C, generator=g)
    v = torch.randn(batch, nk, C, generator=g) + 0.25
    o = torch.randn(batch * nq, ldo, generator=g)
    if logit is not None:
        f = math.sqrt(logit / 3.0)       # q . k / sqrt(d) of unit normals is ~N(0, 1): three sigma -> `logit`
        q, k = q * f, k * f
    return q.to(dtype), k.to(dtype), v.to(dtype), o.to(dtype)


def kernel_ref(q, k, v, o, batch, heads, d, nq, nk, qk_scale, ip_scale):
    """float64 evaluation of the formula on the stored 16-bit inputs -> (ref [batch * nq][C], mag, smax): mag = |o| + |ip_scale|
    sum_j |p_j v_j| per element, smax = max_j qk_scale sum_i |q_i k_ji| per (row, head) broadcast to the head's channels."""
    C = heads * d
    qd = q[:, :C].double().view(batch, nq, heads, d).transpose(1, 2)
    od = o[:, :C].double()
    kd = k.double().view(batch, nk, heads, d).transpose(1, 2)
    vd = v.double().view(batch, nk, heads, d).transpose(1, 2)
    s = torch.matmul(qd, kd.transpose(-1, -2)) * qk_scale
    p = torch.softmax(s, dim=-1)
    a = torch.matmul(p, vd).transpose(1, 2).reshape(batch * nq, C)
    absa = torch.matmul(p, vd.abs()).transpose(1, 2).reshape(batch * nq, C)
    smax = (torch.matmul(qd.abs(), kd.abs().transpose(-1, -2)) * abs(qk_scale)).amax(-1)          # [batch, heads, nq]
    smax = smax.transpose(1, 2).reshape(batch * nq, heads, 1).expand(-1, -1, d).reshape(batch * nq, C)
    return od + ip_scale * a, od.abs() + abs(ip_scale) * absa, smax


def kernel_gate(ref, mag, smax, d, nk, dtype):
    """Per-element bound on |kernel - ref| (derived in tests/test_ip_adapter_gpu.py's docstring)."""
    r16 = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    floor = 0.0 if dtype == torch.bfloat16 else 2.0 ** -24          # fp16 subnormal spacing
    c_acc = U32 * (2.0 * (d + 2) * smax + nk + 40.0)
    return r16 * ref.abs() + c_acc * mag + floor
