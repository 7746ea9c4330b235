"""HyperTile on the HIP path: `apply_patch` / `remove_patch` in the shape of powerpaint_amd/tome.py.

Every top-level self-attention (the blocks whose token grid is the latent grid itself, head dim 40) is restricted to spatial
tiles of the latent: a token attends only inside its own th x tw tile, block-diagonal attention over an nh x nw tiling, which
divides the score count by nh * nw.  The tiles are walked by the tiled form of the pipelined attention kernel with address
arithmetic alone ("HyperTile"; csrc/attention_pipe.hip): one launch where there is one today, no new buffers.  It is
an approximation, so it is opt-in.  Patching or unpatching costs one re-plan of each patched network.

The tiling rule is HyperTile's at swap_size = 1, restated so that it is deterministic (`layout`).  Parity with the `hypertile`
package (and the A1111 / Forge / ComfyUI built-ins) is UNPINNED: the package is not installed where this was written, the rule
below is a restatement from its public description, not a comparison against its output.
"""
from typing import Tuple

from . import _lib as L
from .engine import HyperTile, SDNet, hypertile_split


def layout(H: int, W: int, tile_size: int = 256) -> Tuple[int, int]:
    """(nh, nw) for an H x W latent.  T = max(32, tile_size) // 8 is the target tile side in latent pixels; a side v is cut
    into v // side(v) tiles, side(v) = the smallest divisor of v that is >= min(T, v).  A prime side, or one with no divisor
    >= T other than itself, is not split; (1, 1) leaves the attention as it is.  Pure host function."""
    _check_tile_size(tile_size)
    if int(H) != H or int(W) != W or H < 1 or W < 1:
        raise ValueError(f"H and W must be positive integers, got {H}, {W}")
    return hypertile_split(int(H), int(tile_size)), hypertile_split(int(W), int(tile_size))


def _check_tile_size(tile_size):
    if isinstance(tile_size, bool) or int(tile_size) != tile_size or tile_size <= 0 or tile_size % 8:
        raise ValueError(f"tile_size must be a positive multiple of 8 (pixels), got {tile_size}")


def _networks(model):
    """The SDNets behind `model`: a pipeline's UNet, BrushNet and ControlNet(s), or the one network handed in."""
    ms = []
    for name in ("unet", "brushnet", "controlnet"):
        m = getattr(model, name, None)
        if m is not None:
            ms += list(m.nets) if hasattr(m, "nets") else [m]
    if not ms:
        ms = list(model.nets) if hasattr(model, "nets") else [model]
    nets = [getattr(m, "net", None) for m in ms]
    if not nets or not all(isinstance(n, SDNet) for n in nets):
        raise TypeError(f"apply_patch / remove_patch take a pipeline or a UNet / BrushNet / ControlNet of the HIP path, "
                        f"not {type(model).__name__}")
    return nets


def apply_patch(model, tile_size: int = 256, swap_size: int = 1, max_depth: int = 0):
    """tile_size: the target tile side in pixels (a positive multiple of 8; the rule: `layout`).  swap_size and max_depth are
    HyperTile's arguments of those names and only their values here are implemented.  On a pipeline every network it holds
    is patched.  Which blocks tile on a given latent: `net.hypertile_layout(H, W)`.  Returns `model`."""
    if swap_size != 1:
        raise NotImplementedError("swap_size != 1: random tile sizes per step (device data under the captured graph) are not "
                                  "implemented")
    if max_depth != 0:
        raise NotImplementedError("max_depth != 0: tiling below the top level (head dims 80 / 160) is not implemented")
    _check_tile_size(tile_size)
    nets = _networks(model)
    for net in nets:
        if net.tome is not None:
            raise L.PPError("HyperTile together with token merging (ToMe) on the same network is not implemented: "
                            "tome.remove_patch first")
    for net in nets:
        net.hypertile = HyperTile(int(tile_size))
    return model


def remove_patch(model):
    """The plans and the outputs of networks that never had it.  Returns `model`."""
    for net in _networks(model):
        net.hypertile = None
    return model
