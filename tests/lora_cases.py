"""Shared helpers of tests/test_lora.py and tests/test_lora_gpu.py (not a test module): seeded adapters, the two file
conventions written out key by key, and the float64 merge that is the reference of every merge check."""
import torch

from powerpaint_amd.lora import LoraAdapter


def make_factors(targets, weights, rank, seed, rel=0.1, alpha=None, modules=None):
    """{module: (down, up, alpha)} over `modules` (all of `targets` when None): seeded normal factors scaled so that the
    delta that is ADDED at weight 1, scale 1 -- (alpha / r) U D -- has rms = rel * rms(W) of its module
    (weights: "<module>.weight" -> tensor, or None for unit-rms deltas)."""
    g = torch.Generator("cpu").manual_seed(seed)
    out = {}
    for m in (modules if modules is not None else targets):
        shp = tuple(targets[m])
        down = torch.randn(rank, *shp[1:], generator=g)
        up = torch.randn(shp[0], rank, generator=g)
        a = float(alpha) if alpha is not None else float(rank)
        delta = (a / rank) * up.double() @ down.reshape(rank, -1).double()
        want = rel * (weights[m + ".weight"].double().pow(2).mean().sqrt().item() if weights is not None else 1.0)
        up = (up * (want / delta.pow(2).mean().sqrt().item())).contiguous()
        out[m] = (down.contiguous(), up, a)
    return out


def merged_weights_f64(weights, adapters, scale=1.0):
    """"<module>.weight" -> float64 W + sum_a w_a * scale * (alpha_a / r_a) U_a D_a for every module an adapter touches.
    adapters: [(factors, weight)]."""
    out = {}
    for fac, w in adapters:
        for m, (down, up, alpha) in fac.items():
            k = m + ".weight"
            base = out[k] if k in out else weights[k].double()
            r = down.shape[0]
            d = up.double().reshape(up.shape[0], r) @ down.double().reshape(r, -1)
            out[k] = base + (w * scale * alpha / r) * d.reshape(base.shape)
    return out


def diffusers_keys(adapter: LoraAdapter, style="peft"):
    """The adapter as a diffusers / PEFT state dict (alpha is not stored: it must equal the rank)."""
    dn, un = (".lora_A.weight", ".lora_B.weight") if style == "peft" else (".lora.down.weight", ".lora.up.weight")
    sd = {}
    for comp, fac in adapter.components().items():
        for m, (down, up, alpha) in fac.items():
            assert alpha == down.shape[0]
            sd[f"{comp}.{m}{dn}"] = down.clone()
            sd[f"{comp}.{m}{un}"] = (up.reshape(*up.shape, 1, 1) if down.dim() == 4 else up).clone()
    return sd


def kohya_keys(adapter: LoraAdapter):
    sd = {}
    for comp, fac in adapter.components().items():
        pre = "lora_unet_" if comp == "unet" else "lora_te_"
        for m, (down, up, alpha) in fac.items():
            n = pre + m.replace(".", "_")
            sd[n + ".lora_down.weight"] = down.clone()
            sd[n + ".lora_up.weight"] = (up.reshape(*up.shape, 1, 1) if down.dim() == 4 else up).clone()
            sd[n + ".alpha"] = torch.tensor(float(alpha))
    return sd
