"""Token merging (ToMe for Stable Diffusion, Bolya & Hoffman 2023) on the HIP path: `apply_patch` / `remove_patch` with the
`tomesd` package's names and defaults.

In front of every eligible self-attention the r most redundant tokens are averaged into their most similar destination token,
attention runs on the remaining rows and its output is copied back out to every token ("Token merging";
csrc/tome.hip).  Only `merge_attn` is implemented; `merge_crossattn` and `merge_mlp` are refused, never ignored.  Patching or
unpatching costs one re-plan of the network; new random windows cost nothing (they are data the launches read).
"""
from typing import Optional

import torch

from .engine import SDNet, ToMe


class _State:
    """The CPU generator the destination windows are drawn from: the caller's, or one forked from torch's global CPU RNG
    state at first use (tomesd's behaviour)."""

    def __init__(self, generator: Optional[torch.Generator]):
        self._g = generator

    def generator(self) -> torch.Generator:
        if self._g is None:
            self._g = torch.Generator(device="cpu")
            self._g.set_state(torch.get_rng_state())
        return self._g


def _network(model):
    m = model.unet if hasattr(model, "unet") else model        # a pipeline patches its UNet, as tomesd does
    if not isinstance(getattr(m, "net", None), SDNet):
        raise TypeError(f"apply_patch / remove_patch take a pipeline or a UNet / BrushNet / ControlNet of the HIP path, "
                        f"not {type(model).__name__}")
    return m.net


def apply_patch(model, ratio: float = 0.5, max_downsample: int = 1, sx: int = 2, sy: int = 2, use_rand: bool = True,
                merge_attn: bool = True, merge_crossattn: bool = False, merge_mlp: bool = False,
                generator: Optional[torch.Generator] = None):
    """tomesd.apply_patch.  ratio: share of the tokens merged away (capped at the sources: 1 - 1 / (sx sy)); max_downsample:
    1, 2, 4 or 8 -- blocks at a level with at most that downsample factor take part; sx, sy: the window a destination is chosen
    from; use_rand: a random destination per window and evaluation (off, or with an odd batch: the window's first token);
    generator: a CPU torch.Generator for the windows.  Returns `model`."""
    if merge_crossattn:
        raise NotImplementedError("merge_crossattn=True: token merging in front of the cross-attention is not implemented")
    if merge_mlp:
        raise NotImplementedError("merge_mlp=True: token merging in front of the feed-forward is not implemented")
    if not (float(ratio) >= 0.0):
        raise ValueError(f"ratio must be >= 0, got {ratio}")
    if max_downsample not in (1, 2, 4, 8):
        raise ValueError(f"max_downsample must be 1, 2, 4 or 8, got {max_downsample}")
    if int(sx) != sx or int(sy) != sy or sx < 1 or sy < 1 or sx * sy > 256:
        raise ValueError(f"sx and sy must be integers >= 1 with sx * sy <= 256, got {sx}, {sy}")
    if generator is not None and (not isinstance(generator, torch.Generator) or generator.device.type != "cpu"):
        raise ValueError("generator must be a CPU torch.Generator (the windows are drawn on the host, once per call)")
    net = _network(model)
    remove_patch(model)
    if merge_attn:
        net.tome = ToMe(float(ratio), int(max_downsample), int(sx), int(sy), bool(use_rand))
        net.tome_state = _State(generator)
    return model


def remove_patch(model):
    """tomesd.remove_patch: the plans and the outputs of a network that never had it.  Returns `model`."""
    net = _network(model)
    net.tome = None
    net.tome_state = None
    return model
