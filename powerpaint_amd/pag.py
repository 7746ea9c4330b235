"""Perturbed-attention guidance (PAG, Ahn et al. 2024) on the HIP path: diffusers' `PAGMixin` (0.30) with its arguments
`pag_scale`, `pag_adaptive_scale`, `pag_applied_layers`.

The networks run one more segment of the batch, `[uncond, cond, cond]` with CFG and `[cond, cond]` without, whose selected
self-attentions are the identity (`attn1`'s output is `to_out(to_v(norm1(x)))`: pp_attn_identity_v copies V out of V^T), and
the guided noise moves away from it:  e = e_u + g (e_c - e_u) + s_i (e_c - e_p)  (pp_pag_combine in front of the scheduler's
step launch).  DESIGN.md, "Perturbed-attention guidance".  Everything in this file is host code without a device: the layer
resolver, the per-row scale rule, the batch layout, the refusals, and the combine as tensor code for a duck-typed scheduler.
"""
import re
from typing import Iterable, List, Optional, Sequence, Tuple, Union

import torch

from . import _lib as L
from .engine import PAG


def attn1_names(prefixes: Iterable[str]) -> List[str]:
    """The self-attention modules' names as diffusers' `named_modules()` spells them, from the transformers' prefixes."""
    return [f"{p}.transformer_blocks.0.attn1" for p in prefixes]


def _fake_integral_match(entry: str, name: str) -> bool:
    e, n = entry.split(".")[-1], name.split(".")[-1]
    return e.isnumeric() and n.isnumeric() and e == n


def resolve_layers(layers: Union[str, Sequence[str]], names: Sequence[str]) -> List[str]:
    """`PAGMixin._set_pag_attn_processor`'s selection over `names`: every entry is used as `re.search(entry, name)`; a match
    is discarded when the last dot-component of the entry and of the name are both numeric and equal; an entry that selects
    nothing raises ValueError naming it.  -> the selected names in the order of `names`."""
    if isinstance(layers, str):
        layers = [layers]
    if not isinstance(layers, (list, tuple)) or not layers or not all(isinstance(e, str) for e in layers):
        raise ValueError(f"Expected `pag_applied_layers` to be a string or a list of strings but got {type(layers).__name__}: "
                         f"{layers!r}")
    picked = set()
    for entry in layers:
        hit = [n for n in names if re.search(entry, n) is not None and not _fake_integral_match(entry, n)]
        if not hit:
            raise ValueError(f"Cannot find PAG layer to set attention processor for: {entry}")
        picked.update(hit)
    return [n for n in names if n in picked]


def resolve_prefixes(layers, prefixes: Sequence[str]) -> Tuple[str, ...]:
    """resolve_layers over the attn1 names of the transformers `prefixes` -> the selected transformers' prefixes."""
    names = attn1_names(prefixes)
    chosen = set(resolve_layers(layers, names))
    return tuple(p for p, n in zip(prefixes, names) if n in chosen)


def scale_rows(pag_scale: float, pag_adaptive_scale: float, timesteps) -> List[float]:
    """`PAGMixin._get_pag_scale` per schedule row: s_i = pag_scale when pag_adaptive_scale == 0, else
    max(pag_scale - pag_adaptive_scale * (1000 - t_i), 0).  One row = one network evaluation: fractional t_i (the midpoint
    rows of the two-stage samplers) are taken as they are."""
    s, a = float(pag_scale), float(pag_adaptive_scale)
    if s < 0 or a < 0:
        raise ValueError(f"pag_scale and pag_adaptive_scale must be >= 0, got {pag_scale}, {pag_adaptive_scale}")
    ts = [float(t) for t in (timesteps.tolist() if torch.is_tensor(timesteps) else timesteps)]
    if a == 0.0:
        return [s] * len(ts)
    return [max(s - a * (1000.0 - t), 0.0) for t in ts]


def segments(do_cfg: bool) -> int:
    """Batch segments of a PAG evaluation: [uncond, cond, perturbed] or [cond, perturbed]."""
    return 3 if do_cfg else 2


def layout(t: Optional[torch.Tensor], B: int, do_cfg: bool) -> Optional[torch.Tensor]:
    """A per-call input in the PAG batch layout (`_prepare_perturbed_attention_guidance`): an un-duplicated [B, ...] tensor is
    repeated over every segment, a CFG pair [2B, ...] becomes [first, second, second]; [B, ...] without CFG [t, t]."""
    if t is None or not torch.is_tensor(t):
        return t
    n = segments(do_cfg)
    if t.shape[0] == n * B:
        return t
    if t.shape[0] == B:
        return torch.cat([t] * n, 0)
    if do_cfg and t.shape[0] == 2 * B:
        return torch.cat([t, t[B:]], 0)
    raise L.PPError(f"perturbed-attention guidance: an input of batch {t.shape[0]} fits neither the batch {B} nor its CFG pair")


def combine(eps: torch.Tensor, do_cfg: bool, guidance_scale: float, s: float) -> torch.Tensor:
    """`_apply_perturbed_attention_guidance` as tensor code (the loop of a duck-typed scheduler)."""
    if do_cfg:
        eu, ec, ep = eps.chunk(3)
        return eu + guidance_scale * (ec - eu) + s * (ec - ep)
    ec, ep = eps.chunk(2)
    return ec + s * (ec - ep)


def check_supported(tome: bool = False, guess_mode: bool = False):
    """What is refused by name together with PAG (never ignored)."""
    if tome:
        raise L.PPError("token merging (ToMe, tome.apply_patch) together with perturbed-attention guidance (PAG, pag_scale > 0) "
                        "is not implemented: merging the rows of a segment whose self-attention is the identity is a separate "
                        "design -- call tome.remove_patch or run with pag_scale = 0")
    if guess_mode:
        raise L.PPError("guess_mode=True together with perturbed-attention guidance (PAG, pag_scale > 0) is not implemented: "
                        "the side network would need the perturbed segment's residuals laid out beside the padded pair")


def setting(layers: Sequence[str], n_perturbed: int) -> Optional[PAG]:
    """The UNet's PAG setting: resolved transformer prefixes + batch items of the perturbed segment (None: off)."""
    return PAG(tuple(layers), int(n_perturbed)) if n_perturbed > 0 else None
