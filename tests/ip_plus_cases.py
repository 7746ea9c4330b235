"""Shared by the IP-Adapter Plus tests and the fixture generator (not a test file; nothing here is imported by the product).

IP-Adapter Plus differs from a base adapter (tests/ip_adapter_cases.py) in its image projection alone: the Resampler, which
turns the image encoder's patch states [N, S, E] into Q tokens per image.  diffusers is not a dependency of this repository and
the reference imports the class from diffusers (`IPAdapterPlusImageProjection`), so the Resampler is RESTATED here from its
contract -- the adapter FILE's own key names and the published arithmetic -- independently of the package's module
(powerpaint_amd.ip_adapter.IPAdapterPlusImageProjection, which carries diffusers' parameter names):

    x = proj_in(x);  l = latents repeated N times
    per layer:  xn, ln = norm1(x), norm2(l);  q = to_q(ln);  k | v = to_kv(cat([xn, ln], 1)) (first half of the columns K)
                l = to_out(softmax(q k^T / sqrt(64)) v) + l        per head of 64 channels
                l = W2 gelu_erf(W1 LayerNorm(l)) + l
    tokens = norm_out(proj_out(l))

  * `Resampler` / `Resampler.from_file(image_proj)`: that, with the file's keys as its state_dict keys.
  * `plus_state_dict(unet, seed, Q, dim, E, depth, heads, ff)`: a seeded Plus adapter in file form for an oracle UNet.
  * `HiddenStateEncoder`: a stand-in `image_encoder` with `.hidden_states` (three of them: [-2] is not the last).
  * `PlusIPUNet`: ip_adapter_cases.IPUNet with a Resampler (Plus) or an ImageProjection (base) per adapter in front.
  * the fixture's cases, and pp_perceiver_attn's float64 reference and per-element bound.
"""
import math
from types import SimpleNamespace

import torch
import torch.nn as nn

import ip_adapter_cases as IC
from ip_adapter_cases import IPUNet, kernel_gate, kernel_ref, loop_gate, net_gate  # noqa: F401  (what the Plus tests share)

HEAD_DIM = 64
# the fixture's Plus adapters: 16 tokens per image from S = 10 hidden states of width 32
FIX = dict(Q=16, dim=64, E=32, depth=2, heads=2, ff=128)
FIX_S = 10
W_STD = IC.W_STD

# name -> kinds of the adapters, scales, images per prompt, image prompt through the encoder?
CASES = dict(plus=dict(kinds=["plus"], scales=[1.0], images=[1], encoder=False),
             plus_image=dict(kinds=["plus"], scales=[1.0], images=[1], encoder=True),
             mixed=dict(kinds=["base", "plus"], scales=[0.7, 0.4], images=[1, 2], encoder=False))


class PerceiverAttention(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        inner = heads * HEAD_DIM
        self.heads = heads
        self.norm1, self.norm2 = nn.LayerNorm(dim), nn.LayerNorm(dim)
        self.to_q = nn.Linear(dim, inner, bias=False)
        self.to_kv = nn.Linear(dim, 2 * inner, bias=False)
        self.to_out = nn.Linear(inner, dim, bias=False)

    def forward(self, x, latents):
        xn, ln = self.norm1(x), self.norm2(latents)
        N, Q, _ = ln.shape
        q = self.to_q(ln)
        k, v = self.to_kv(torch.cat([xn, ln], dim=1)).chunk(2, dim=-1)

        def heads(t):
            return t.reshape(N, t.shape[1], self.heads, HEAD_DIM).transpose(1, 2)

        s = torch.matmul(heads(q), heads(k).transpose(-1, -2)) / math.sqrt(HEAD_DIM)
        a = torch.matmul(torch.softmax(s.float(), dim=-1).to(s.dtype), heads(v))
        return self.to_out(a.transpose(1, 2).reshape(N, Q, -1))


class Resampler(nn.Module):
    def __init__(self, Q, dim, E, out, depth, heads, ff):
        super().__init__()
        self.latents = nn.Parameter(torch.zeros(1, Q, dim))
        self.proj_in, self.proj_out, self.norm_out = nn.Linear(E, dim), nn.Linear(dim, out), nn.LayerNorm(out)
        self.layers = nn.ModuleList([
            nn.ModuleList([PerceiverAttention(dim, heads),
                           nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, ff, bias=False), nn.GELU(),
                                         nn.Linear(ff, dim, bias=False))]) for _ in range(depth)])

    @classmethod
    def from_file(cls, ip):
        Q, dim = ip["latents"].shape[1:]
        depth = 1 + max(int(k.split(".")[1]) for k in ip if k.startswith("layers."))
        m = cls(Q, dim, ip["proj_in.weight"].shape[1], ip["proj_out.weight"].shape[0], depth,
                ip["layers.0.0.to_q.weight"].shape[0] // HEAD_DIM, ip["layers.0.1.1.weight"].shape[0])
        m.load_state_dict({k: v.float() for k, v in ip.items()}, strict=True)
        return m.eval()

    def forward(self, x):
        latents = self.latents.repeat(x.shape[0], 1, 1)
        x = self.proj_in(x)
        for attn, ff in self.layers:
            latents = attn(x, latents) + latents
            latents = ff(latents) + latents
        return self.norm_out(self.proj_out(latents))


def plus_image_proj(g, Q, dim, E, depth, heads, ff, out=IC.CTX):
    """The image_proj half of a Plus file: matrices and latents rounded to bf16 (what the HIP path stores), seeded by `g`."""
    inner = heads * HEAD_DIM
    r = IC.bf16_round

    def mat(n, k):
        return r(torch.randn(n, k, generator=g) / math.sqrt(k))

    def ln(n):
        return 1.0 + 0.1 * torch.randn(n, generator=g), 0.05 * torch.randn(n, generator=g)

    ip = {"latents": r(torch.randn(1, Q, dim, generator=g)), "proj_in.weight": mat(dim, E),
          "proj_in.bias": 0.1 * torch.randn(dim, generator=g), "proj_out.weight": mat(out, dim),
          "proj_out.bias": 0.1 * torch.randn(out, generator=g)}
    ip["norm_out.weight"], ip["norm_out.bias"] = ln(out)
    for i in range(depth):
        p = f"layers.{i}"
        ip[f"{p}.0.norm1.weight"], ip[f"{p}.0.norm1.bias"] = ln(dim)
        ip[f"{p}.0.norm2.weight"], ip[f"{p}.0.norm2.bias"] = ln(dim)
        ip[f"{p}.0.to_q.weight"], ip[f"{p}.0.to_kv.weight"] = mat(inner, dim), mat(2 * inner, dim)
        ip[f"{p}.0.to_out.weight"] = mat(dim, inner)
        ip[f"{p}.1.0.weight"], ip[f"{p}.1.0.bias"] = ln(dim)
        ip[f"{p}.1.1.weight"], ip[f"{p}.1.3.weight"] = mat(ff, dim), mat(dim, ff)
    return ip


def plus_state_dict(unet, seed, Q, dim, E, depth, heads, ff, std=W_STD):
    """A Plus adapter in file form for the oracle UNet's architecture: the Resampler's image_proj and, as for a base adapter,
    {"{2k+1}.to_k_ip.weight", ...}; matrices rounded to bf16, seeded."""
    g = torch.Generator().manual_seed(seed)
    ip = plus_image_proj(g, Q, dim, E, depth, heads, ff)
    ad = {}
    for k, tb in enumerate(IC.cross_attention_blocks(unet)):
        c = tb.attn2.to_q.out_features
        for n in ("to_k_ip", "to_v_ip"):
            ad[f"{2 * k + 1}.{n}.weight"] = IC.bf16_round(torch.randn(c, IC.CTX, generator=g) * (std / math.sqrt(IC.CTX)))
    return {"image_proj": ip, "ip_adapter": ad}


def projection_layer(sd):
    ip = sd["image_proj"]
    if "latents" in ip:
        return Resampler.from_file(ip)
    lay = IC.ImageProjection(ip["proj.weight"].shape[1], IC.CTX, ip["proj.weight"].shape[0] // IC.CTX)
    with torch.no_grad():
        lay.image_embeds.weight.copy_(ip["proj.weight"]); lay.image_embeds.bias.copy_(ip["proj.bias"])
        lay.norm.weight.copy_(ip["norm.weight"]); lay.norm.bias.copy_(ip["norm.bias"])
    return lay.eval()


class PlusIPUNet(IPUNet):
    """ip_adapter_cases.IPUNet whose projection layers follow the adapters' kinds (its own loader knows base files only)."""

    def __init__(self, unet, state_dicts, scales):
        nn.Module.__init__(self)
        self.unet = unet
        mods = IC.install_ip_attention(unet, len(state_dicts))
        with torch.no_grad():
            for i, sd in enumerate(state_dicts):
                for k, m in enumerate(mods):
                    m.to_k_ip[i].weight.copy_(sd["ip_adapter"][f"{2 * k + 1}.to_k_ip.weight"])
                    m.to_v_ip[i].weight.copy_(sd["ip_adapter"][f"{2 * k + 1}.to_v_ip.weight"])
        for m in mods:
            m.scale = [float(s) for s in scales]
        self.encoder_hid_proj = IC.MultiProjection([projection_layer(sd) for sd in state_dicts]).eval()
        self.ip_modules = mods
        self.config = SimpleNamespace(**vars(unet.config))
        self.config.encoder_hid_dim_type = "ip_image_proj"


class HiddenStateEncoder(nn.Module):
    """Stand-in `image_encoder` of case `plus_image`: [B, 3, 8, 8] pixel tensors -> .hidden_states, three [B, S, E] tensors (so
    that [-2] is neither the first nor the last), and .image_embeds.  The biases make the hidden states of a zero image
    non-zero, as a real tower's are."""

    def __init__(self, seed: int = 78, S: int = FIX_S, E: int = FIX["E"]):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.S, self.E = S, E
        self.embed = nn.Linear(192, S * E)
        self.mix1, self.mix2 = nn.Linear(E, E), nn.Linear(E, E)
        with torch.no_grad():
            self.embed.weight.copy_(torch.randn(S * E, 192, generator=g) / math.sqrt(192))
            self.embed.bias.copy_(0.5 * torch.randn(S * E, generator=g))
            for m in (self.mix1, self.mix2):
                m.weight.copy_(torch.randn(E, E, generator=g) / math.sqrt(E))
                m.bias.copy_(0.3 * torch.randn(E, generator=g))

    def forward(self, image, output_hidden_states=False, **kw):
        h0 = self.embed(image.flatten(1)).reshape(image.shape[0], self.S, self.E)
        h1 = h0 + torch.tanh(self.mix1(h0))
        h2 = h1 + torch.tanh(self.mix2(h1))
        return SimpleNamespace(hidden_states=(h0, h1, h2) if output_hidden_states else None, image_embeds=h2[:, 0])


def case_adapters(unet, name, std=W_STD):
    c = CASES[name]
    return [plus_state_dict(unet, 700 + 10 * i + len(name), std=std, **FIX) if kind == "plus"
            else IC.adapter_state_dict(unet, 700 + 10 * i + len(name), std=std) for i, kind in enumerate(c["kinds"])]


def case_prompt(name, variant: int = 0):
    """The image prompt of a fixture case: precomputed embeds (negative half, then positive half: [2, n, D] for a base
    adapter, [2, n, S, E] for a Plus one) or the pixel tensor for the stand-in encoder.  variant 1: other values."""
    c = CASES[name]
    g = torch.Generator().manual_seed(5000 + 17 * variant + len(name))
    if c["encoder"]:
        return dict(ip_adapter_image=torch.randn(1, 3, 8, 8, generator=g))
    embeds = []
    for kind, n in zip(c["kinds"], c["images"]):
        shape = (1, n, FIX_S, FIX["E"]) if kind == "plus" else (1, n, IC.EMBED_DIM)
        pos = torch.randn(*shape, generator=g)
        neg = 0.3 * torch.randn(*shape, generator=g)
        embeds.append(torch.cat([neg, pos]))
    return dict(ip_adapter_image_embeds=embeds)


# ---------------------------------------------------------------------------------------------------------------- kernel
U32 = IC.U32


def perceiver_inputs(batch, heads, nq, nx, nl, dtype, seed=0, logit=None, pad=16, big_key=None):
    """q [batch * nq][C + pad]; kv_x [batch * nx][2 C + pad], kv_l [batch * nl][2 C + pad] (None for nl = 0), rows of [K | V], in
    `dtype`; distinct per batch item.  logit: scale q and k so that |q . k| / 8 reaches about that value; big_key: that key
    (index over the nx + nl keys) gets 2.5 times the other keys' K, so the largest logits sit in its tile."""
    C = heads * HEAD_DIM
    g = torch.Generator().manual_seed(4321 + seed)
    q = torch.randn(batch * nq, C + pad, generator=g)
    kv = torch.randn(batch, nx + nl, 2 * C + pad, generator=g)
    kv[:, :, C:2 * C] += 0.25
    if logit is not None:
        f = math.sqrt(logit / 3.0)
        q[:, :C] *= f
        kv[:, :, :C] *= f
    if big_key is not None:
        kv[:, big_key, :C] *= 2.5
    kv_x = kv[:, :nx].reshape(batch * nx, -1).contiguous()
    kv_l = kv[:, nx:].reshape(batch * nl, -1).contiguous() if nl else None
    return q.to(dtype), kv_x.to(dtype), (kv_l.to(dtype) if nl else None)


def perceiver_ref(q, kv_x, kv_l, batch, heads, nq, scale, dt=torch.float64, drop=None):
    """Evaluation in `dt` of the formula on the stored 16-bit inputs -> (ref [batch * nq][C], mag = sum_t |p_t v_t|, smax =
    max_t scale sum_j |q_j k_tj| per (row, head) broadcast to the head's channels, vmax = max |v|).  drop: leave that key out."""
    C = heads * HEAD_DIM
    nx = kv_x.shape[0] // batch
    kv = kv_x.to(dt).view(batch, nx, -1)
    if kv_l is not None:
        kv = torch.cat([kv, kv_l.to(dt).view(batch, kv_l.shape[0] // batch, -1)], 1)
    if drop is not None:
        kv = torch.cat([kv[:, :drop], kv[:, drop + 1:]], 1)
    nk = kv.shape[1]
    qd = q[:, :C].to(dt).view(batch, nq, heads, HEAD_DIM).transpose(1, 2)
    kd = kv[:, :, :C].reshape(batch, nk, heads, HEAD_DIM).transpose(1, 2)
    vd = kv[:, :, C:2 * C].reshape(batch, nk, heads, HEAD_DIM).transpose(1, 2)
    p = torch.softmax(torch.matmul(qd, kd.transpose(-1, -2)) * scale, dim=-1)
    ref = torch.matmul(p, vd).transpose(1, 2).reshape(batch * nq, C)
    mag = torch.matmul(p, vd.abs()).transpose(1, 2).reshape(batch * nq, C)
    smax = (torch.matmul(qd.abs(), kd.abs().transpose(-1, -2)) * abs(scale)).amax(-1)
    smax = smax.transpose(1, 2).reshape(batch * nq, heads, 1).expand(-1, -1, HEAD_DIM).reshape(batch * nq, C)
    return ref, mag, smax, float(vd.abs().max())


def perceiver_gate(ref, mag, smax, vmax, nk, dtype, d=HEAD_DIM):
    """Per-element bound on |pp_perceiver_attn - ref| (derived in tests/test_ip_adapter_plus_gpu.py's docstring)."""
    r16 = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11          # unit roundoff: 8 / 11 significant bits, to nearest
    floor = 0.0 if dtype == torch.bfloat16 else 2.0 ** -24 + nk * 2.0 ** -25 * vmax
    c_acc = U32 * (2.0 * (d + 4) * smax + 3.0 * nk + 40.0)
    return r16 * ref.abs() + (r16 + c_acc) * mag + floor
