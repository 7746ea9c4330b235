"""DeepCache on the HIP path: `DeepCacheSDHelper` with the `DeepCache` package's method names.

Between consecutive denoising steps the deep features of the UNet barely move (Ma et al., "DeepCache", CVPR 2024).  A FULL
evaluation is the network as it is, which also keeps `c`, the hidden tensor handed to one of the outer up layers; a SHALLOW
evaluation runs conv_in, the first k down modules, the up layers from that one on (entering on the cached c) and conv_out, and
nothing else: no mid block, no deeper level.  Which evaluations are full is a host schedule (`cache_interval`); where the cut
lies (`cache_branch_id`, k = id + 1) is part of the plan key: patching costs one re-plan of each patched network, after which
every runtime holds two plans on one arena (NetRuntime.ensure; DESIGN.md, "DeepCache").  It is an approximation, so it is opt-in.

The rule, for one network with skip tensors S[0..n-1] (conv_in's output, then every down layer's and downsampler's; SD-1.5:
n = 12) and up layers U[0..n-1] (U[j] takes S[n-1-j]): c is what U[n-1-k] is handed, side-network adds included; a shallow
evaluation makes S[0..k], then runs U[n-1-k..n-1] with the upsamplers between them.  BrushNet follows the rule on its own
trunk with its own c and produces the zero-conv residuals of the live positions only; a ControlNet runs its down path up to
S[k] and the zero convs 0..k and has no cache.  Evaluations are counted from 0 at the start of every pipeline call, every row
of a two-stage sampler counts, and evaluation e is full iff e % cache_interval == 0, for every network of the pipeline alike.

Parity with the `DeepCache` package is UNPINNED: the package is not installed where this was written, the rule above is a
restatement from its public description (deterministic, and for any layers_per_block), not a comparison against its output.
"""
from typing import List

from . import _lib as L
from .engine import DeepCache, SDNet


def _models(model) -> List[object]:
    """The model wrappers behind `model`: a pipeline's UNet, BrushNet and ControlNet(s), or the one network handed in."""
    ms = []
    for name in ("unet", "brushnet", "controlnet"):
        m = getattr(model, name, None)
        if m is not None:
            ms += list(m.nets) if hasattr(m, "nets") else [m]
    if not ms:
        ms = list(model.nets) if hasattr(model, "nets") else [model]
    if not ms or not all(isinstance(getattr(m, "net", None), SDNet) for m in ms):
        raise TypeError(f"DeepCacheSDHelper takes a pipeline or a UNet / BrushNet / ControlNet of the HIP path, "
                        f"not {type(model).__name__}")
    return ms


def check_params(nets, cache_interval, cache_branch_id, skip_mode="uniform"):
    """The refusals of `set_params` / `enable`, by name."""
    if skip_mode != "uniform":
        raise NotImplementedError(f"skip_mode={skip_mode!r}: only the uniform schedule (every cache_interval-th evaluation is "
                                  f"full) is implemented")
    if isinstance(cache_interval, bool) or not isinstance(cache_interval, int) or cache_interval < 1:
        raise ValueError(f"cache_interval must be an integer >= 1, got {cache_interval!r}")
    if isinstance(cache_branch_id, bool) or not isinstance(cache_branch_id, int):
        raise ValueError(f"cache_branch_id must be an integer, got {cache_branch_id!r}")
    for net in nets:
        n = net.skip_count()
        if not 0 <= cache_branch_id <= n - 2:
            raise ValueError(f"cache_branch_id must lie in 0..{n - 2} for this {net.kind} ({n} skip tensors), got {cache_branch_id}")


class DeepCacheSDHelper:
    """helper = DeepCacheSDHelper(pipe); helper.set_params(cache_interval=3, cache_branch_id=0); helper.enable(); ...;
    helper.disable().  `pipe`: a pipeline (every network it holds is patched) or one UNet / BrushNet / ControlNet."""

    def __init__(self, pipe=None):
        self.pipe = pipe
        self.params = dict(cache_interval=3, cache_branch_id=0, skip_mode="uniform")
        self.enabled = False

    def _nets(self):
        if self.pipe is None:
            raise ValueError("DeepCacheSDHelper: no pipeline or network given")
        return _models(self.pipe)

    def set_params(self, cache_interval: int = 3, cache_branch_id: int = 0, skip_mode: str = "uniform"):
        """Before or after `enable`.  A new cache_interval alone re-plans nothing; a new cache_branch_id re-plans."""
        check_params([m.net for m in self._nets()] if self.pipe is not None else [], cache_interval, cache_branch_id, skip_mode)
        self.params = dict(cache_interval=cache_interval, cache_branch_id=cache_branch_id, skip_mode=skip_mode)
        if self.enabled:
            self.enable()
        return self

    def enable(self, pipe=None):
        """Patch every network; every network's evaluation counter starts again at 0 (the next evaluation is full)."""
        if pipe is not None:
            self.pipe = pipe
        ms = self._nets()
        p = self.params
        check_params([m.net for m in ms], p["cache_interval"], p["cache_branch_id"], p["skip_mode"])
        for m in ms:
            if m.net.tome is not None:
                raise L.PPError("DeepCache together with token merging (ToMe) on the same network is not implemented: "
                                "tome.remove_patch first")
        for m in ms:
            m.net.deepcache = DeepCache(int(p["cache_branch_id"]), int(p["cache_interval"]))
            rt = getattr(m, "rt", None)
            if rt is not None:
                rt.dc_eval = 0
        self.enabled = True
        return self

    def disable(self):
        """The plans and the outputs of networks that never had it."""
        for m in self._nets():
            m.net.deepcache = None
        self.enabled = False
        return self

