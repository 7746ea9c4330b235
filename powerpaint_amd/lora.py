"""LoRA adapter files -> per-module low-rank factors (host side of the adapter merge, DESIGN.md "LoRA adapters").

The reference's pipelines inherit diffusers' LoraLoaderMixin
(/root/reference/powerpaint/pipelines/pipeline_PowerPaint_Brushnet_CA.py:147-148); here an adapter is read into

    {component ("unet" | "text_encoder"): {target module name: (down [r][in...], up [out][r], alpha)}}      fp32, host

and merged into the packed weights on the device (SDNet.repack / pp_lora_merge):

    W_eff = W + sum_a  w_a * s * (alpha_a / r_a) * U_a @ D_a

Two key conventions are recognised from the keys themselves (restated from their published form; neither diffusers nor
peft is imported):
  * diffusers / PEFT:  unet.<module>.lora_A.weight (down) / .lora_B.weight (up), the older
    unet.<module>.lora.down.weight / .lora.up.weight; text_encoder.<module>.… likewise; alpha = rank;
  * kohya-ss:  lora_unet_<module, dots as underscores>.lora_down.weight / .lora_up.weight / .alpha and
    lora_te_text_model_encoder_layers_<i>_….  The underscore form is ambiguous ("to_out_0", "ff_net_0_proj"), so it is
    looked up in a table built from the model's OWN module names, never taken apart as a string.
Whatever is not implemented is refused by name (a swallowed key would load, run and give the wrong image): a key that
matches no module, a shape that does not fit, DoRA / LoHa / LoKr / LoCon-mid tensors, bias deltas, ranks above the kernel's.
"""
import os
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import torch

from . import _lib as L

MAX_RANK = L.PP_LORA_MAX_RANK
MAX_ADAPTERS = L.PP_LORA_MAX_ADAPTERS
LORA_WEIGHT_NAMES = ("pytorch_lora_weights.safetensors", "pytorch_lora_weights.bin")
TEXT_TARGETS = ("q_proj", "k_proj", "v_proj", "out_proj", "fc1", "fc2")
_REFUSED = (("dora_scale", "DoRA"), ("hada_", "LoHa"), ("lokr_", "LoKr"), (".lora_mid.", "LoCon lora_mid"))

Factors = Tuple[torch.Tensor, torch.Tensor, float]       # (down, up, alpha)


@dataclass
class LoraAdapter:
    unet: Dict[str, Factors] = field(default_factory=dict)
    text_encoder: Dict[str, Factors] = field(default_factory=dict)

    def components(self):
        return {"unet": self.unet, "text_encoder": self.text_encoder}

    def equal(self, other: "LoraAdapter") -> bool:
        for a, b in ((self.unet, other.unet), (self.text_encoder, other.text_encoder)):
            if sorted(a) != sorted(b):
                return False
            for m in a:
                if not (torch.equal(a[m][0], b[m][0]) and torch.equal(a[m][1], b[m][1]) and float(a[m][2]) == float(b[m][2])):
                    return False
        return True


def unet_targets(net) -> Dict[str, Tuple[int, ...]]:
    """module name -> weight shape of every adapter target of an SDNet: all 2-D and 4-D `.weight`s of its
    state_dict_spec() (attention projections, feed-forward, proj_in / proj_out, resnet and sampler convs, conv_in / conv_out,
    time embedding); the norms (1-D) take none."""
    return {k[:-len(".weight")]: tuple(s) for k, s in net.state_dict_spec().items()
            if k.endswith(".weight") and len(s) in (2, 4)}


def text_targets(text_encoder) -> Dict[str, Tuple[int, ...]]:
    """module name -> weight shape of the CLIP text tower's targets, from its own named_modules()."""
    return {n: tuple(m.weight.shape) for n, m in text_encoder.named_modules()
            if isinstance(m, torch.nn.Linear) and n.rsplit(".", 1)[-1] in TEXT_TARGETS}


def _default_unet_targets():
    from .engine import SDNet
    return unet_targets(SDNet("unet", 4))


def _default_text_targets():
    from .models.clip_text import CLIPTextModel
    return text_targets(CLIPTextModel(device="meta"))


def _read_file(path: str, weight_name: Optional[str]) -> Dict[str, torch.Tensor]:
    from .loaders import read_state_dict
    if os.path.isdir(path):
        names = (weight_name,) if weight_name else LORA_WEIGHT_NAMES
        for n in names:
            if os.path.isfile(os.path.join(path, n)):
                return read_state_dict(os.path.join(path, n))
        raise L.PPError(f"no LoRA weight file in {path} (looked for {', '.join(names)})")
    if not os.path.isfile(path):
        raise L.PPError(f"LoRA file {path} not found (there is no hub download on this path)")
    return read_state_dict(path)


def read_lora(path_or_dict, weight_name: Optional[str] = None, unet_modules: Optional[Dict[str, tuple]] = None,
              text_modules: Optional[Dict[str, tuple]] = None) -> LoraAdapter:
    """Read a `.safetensors` / `.bin` adapter file (or a directory holding one, or a state dict) into a LoraAdapter.
    unet_modules / text_modules: the target tables of the models the adapter is meant for (`unet_targets(net)`,
    `text_targets(text_encoder)`); the SD-1.5 UNet and the SD-1.5 CLIP text tower when not given."""
    sd = path_or_dict if isinstance(path_or_dict, dict) else _read_file(str(path_or_dict), weight_name)
    tables = {"unet": unet_modules if unet_modules is not None else _default_unet_targets(),
              "text_encoder": text_modules if text_modules is not None else _default_text_targets()}
    under = {c: {m.replace(".", "_"): m for m in t} for c, t in tables.items()}
    for c, u in under.items():
        if len(u) != len(tables[c]):
            raise L.PPError(f"{c}: two module names collapse to one kohya name")
    parts: Dict[Tuple[str, str], Dict[str, torch.Tensor]] = {}
    for key, t in sd.items():
        for pat, what in _REFUSED:
            if pat in key:
                raise L.PPError(f"LoRA key {key!r}: {what} adapters are not implemented")
        comp = module = role = None
        if key.startswith(("unet.", "text_encoder.")):
            comp, rest = key.split(".", 1)
            for suf, rl in ((".lora_A.weight", "down"), (".lora_B.weight", "up"), (".lora.down.weight", "down"),
                            (".lora.up.weight", "up")):
                if rest.endswith(suf):
                    module, role = rest[:-len(suf)], rl
            if module is None and rest.endswith(".bias"):
                raise L.PPError(f"LoRA key {key!r}: bias deltas are not implemented")
            if module is not None and module not in tables[comp]:
                raise L.PPError(f"LoRA key {key!r} matches no target module of the {comp}")
        elif key.startswith(("lora_unet_", "lora_te_")):
            comp = "unet" if key.startswith("lora_unet_") else "text_encoder"
            rest = key[len("lora_unet_" if comp == "unet" else "lora_te_"):]
            name, _, tail = rest.partition(".")
            role = {"lora_down.weight": "down", "lora_up.weight": "up", "alpha": "alpha"}.get(tail)
            if role is None and tail.endswith(("bias", "diff_b", "diff")):
                raise L.PPError(f"LoRA key {key!r}: bias / full-weight deltas are not implemented")
            if role is not None:
                if name not in under[comp]:
                    raise L.PPError(f"LoRA key {key!r} matches no target module of the {comp}")
                module = under[comp][name]
        if module is None or role is None:
            raise L.PPError(f"LoRA key {key!r} is not recognised (diffusers / PEFT `unet.<module>.lora_A.weight`, "
                            f"`.lora.down.weight` and kohya `lora_unet_<module>.lora_down.weight` / `.alpha` are)")
        slot = parts.setdefault((comp, module), {"_key": key})
        if role in slot:
            raise L.PPError(f"LoRA key {key!r}: the {role} factor of {module} is given twice")
        slot[role] = t
    out = LoraAdapter()
    for (comp, module), p in parts.items():
        key = p["_key"]
        if "down" not in p or "up" not in p:
            raise L.PPError(f"LoRA key {key!r}: {module} has no {'down' if 'down' not in p else 'up'} factor")
        down, up = p["down"].detach().float().contiguous(), p["up"].detach().float().contiguous()
        shape = tuple(tables[comp][module])
        r = down.shape[0]
        up2 = up.reshape(up.shape[0], -1)
        if down.dim() != len(shape) or tuple(down.shape[1:]) != shape[1:] or up2.shape != (shape[0], r) or \
                (up.dim() == 4 and tuple(up.shape[2:]) != (1, 1)) or up.dim() not in (2, 4):
            raise L.PPError(f"LoRA key {key!r}: factors down {tuple(down.shape)} / up {tuple(up.shape)} do not fit "
                            f"{module}.weight {shape}")
        if not 1 <= r <= MAX_RANK:
            raise L.PPError(f"LoRA key {key!r}: rank {r} is outside 1..{MAX_RANK} (the merge kernel's limit)")
        alpha = float(p["alpha"]) if "alpha" in p else float(r)
        out.components()[comp][module] = (down, up2.contiguous(), alpha)
    return out


class AdapterSet:
    """Book-keeping shared by the models: loaded adapters (name -> {module: factors}), the active list with weights."""

    def __init__(self):
        self.loaded: Dict[str, Dict[str, Factors]] = {}
        self.active: Dict[str, float] = {}
        self.gen: Dict[str, int] = {}        # name -> serial number of the load: a NAME can come back with other contents
        self._serial = 0

    def add(self, name: str, factors: Dict[str, Factors]):
        if name in self.loaded:
            raise ValueError(f"Adapter name {name} already in use")
        self.loaded[name] = factors
        self._serial += 1
        self.gen[name] = self._serial
        self.active[name] = 1.0          # (as in diffusers: a freshly loaded adapter becomes active beside the others)

    def set(self, names, weights=None):
        names = [names] if isinstance(names, str) else list(names)
        if weights is None:
            weights = [1.0] * len(names)
        elif not isinstance(weights, (list, tuple)):
            weights = [weights] * len(names)
        if len(weights) != len(names):
            raise ValueError(f"Length of adapter names {len(names)} is not equal to the length of their weights {len(weights)}")
        for n in names:
            if n not in self.loaded:
                raise ValueError(f"Adapter {n!r} is not loaded (loaded: {sorted(self.loaded)})")
        if len(names) > MAX_ADAPTERS:
            raise L.PPError(f"at most {MAX_ADAPTERS} adapters can be active at once ({len(names)} asked for)")
        self.active = {n: float(1.0 if w is None else w) for n, w in zip(names, weights)}

    def delete(self, names):
        names = [names] if isinstance(names, str) else list(names)
        for n in names:
            if n not in self.loaded:
                raise ValueError(f"Adapter {n!r} is not loaded")
            del self.loaded[n]
            del self.gen[n]
            self.active.pop(n, None)

    def state(self, scale: float):
        """What the merged weights depend on (None = no adapter in them): which LOADS are active (name and serial number, so
        that an adapter deleted and loaded again under its old name is another one), their weights, the scale."""
        act = tuple((n, self.gen[n], w) for n, w in self.active.items())
        return (act, float(scale)) if act else None
