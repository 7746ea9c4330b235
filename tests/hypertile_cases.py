"""Shared by the HyperTile tests (not a test file): the semantics in float64, independent of powerpaint_amd.  Plain torch.

HyperTile restricts a self-attention over the h x w tokens of a latent to spatial tiles: the grid is cut into nh x nw tiles of
th x tw = (h / nh) x (w / nw) tokens and every token attends only inside its own tile.

PARITY IS UNPINNED.  The `hypertile` package (and the A1111 / Forge / ComfyUI built-ins it went into) is not installed where
these tests were written, so nothing here was compared against its output.  The rule below is HyperTile's at swap_size = 1
(one fixed divisor per side instead of a random choice among the `swap_size` smallest ones), restated so that it is
deterministic; a figure measured with the package may differ where the package picks another divisor.

The rule, on the latent H x W of the call (tile_size in pixels, 8 pixels per latent pixel):
    T       = max(32, tile_size) // 8                     target tile side in latent pixels
    side(v) = the smallest divisor of v that is >= min(T, v)
    n(v)    = v // side(v)
    nh, nw  = n(H), n(W);  th, tw = H // nh, W // nw;  nh * nw == 1: the attention is left as it is
A prime side, or one with no divisor >= T other than itself, is not split.

The token map: token r of tile (ty, tx), r in [0, th * tw), is row  (ty * th + r // tw) * w + tx * tw + r % tw  of the batch
item (tiles in row-major order, tokens inside a tile in row-major order).

The error bound of a kernel against `tiled_attention_f64` is the P3 gate of tests/attention_cases.py (derived there per key
count), evaluated per TILE: a query's probabilities, its denominator and (fp16) the subnormal term sum_j |V_j| run over the
th * tw keys of its tile, not over the grid.  `tile_gate` does that by handing the gathered tiles to AC.gate_p3 as
batch * nh * nw items of th * tw keys.
"""
import torch

import attention_cases as AC

# (v, tile_size) -> n(v): the sides the issue names, the three tile sizes, the min(T, v) clamp (v < T: one tile, side = v)
RULE_SIDES = {
    (64, 256): 2, (128, 256): 4, (96, 256): 3, (29, 256): 1, (65, 256): 1, (40, 256): 1, (48, 256): 1,
    (64, 128): 4, (128, 128): 8, (96, 128): 6, (29, 128): 1, (65, 128): 1, (40, 128): 2, (48, 128): 3,
    (64, 512): 1, (128, 512): 2, (96, 512): 1, (29, 512): 1, (65, 512): 1, (40, 512): 1, (48, 512): 1,
    (16, 256): 1, (31, 256): 1, (32, 256): 1, (3, 128): 1, (1, 256): 1,          # the clamp: v <= T
    (192, 256): 6, (192, 768): 2, (66, 256): 2, (130, 256): 2, (64, 8): 16, (64, 32): 16, (64, 40): 8,   # T >= 4 always; T = 5 -> side 8
}
RULE_LAYOUTS = {(64, 64): (2, 2), (128, 128): (4, 4), (96, 64): (3, 2), (29, 32): (1, 1), (16, 64): (1, 2), (16, 40): (1, 1)}

# (h, w, nh, nw) of the kernel tests: the smallest shapes at which the address walk can go wrong
KERNEL_CASES = [
    (16, 64, 1, 2),     # tw = 32: two runs per 64-key LDS tile
    (8, 128, 1, 2),     # tw = 64: one run per tile, a wrap after every tile
    (4, 256, 1, 2),     # tw = 128: a wrap every second tile
    (32, 32, 2, 1),     # bands: nw = 1, contiguous tiles
    (32, 64, 2, 2),     # both axes split
    (20, 32, 2, 1),     # 320-token tiles: a partly filled query block in the 128- and the 256-query forms (contiguous)
    (10, 64, 1, 2),     # ... and with tw = 32
    (64, 64, 2, 2),     # the headline's own geometry, once
]


def side(v: int, tile_size: int) -> int:
    T = min(max(32, tile_size) // 8, v)
    s = T
    while v % s:
        s += 1
    return s


def split(v: int, tile_size: int) -> int:
    return v // side(v, tile_size)


def layout(H: int, W: int, tile_size: int = 256):
    return split(H, tile_size), split(W, tile_size)


def token_map(h: int, w: int, nh: int, nw: int) -> torch.Tensor:
    """int64 [nh * nw, th * tw]: row of the batch item that holds token r of tile (ty, tx), by the formula."""
    th, tw = h // nh, w // nw
    out = torch.empty(nh * nw, th * tw, dtype=torch.int64)
    for ty in range(nh):
        for tx in range(nw):
            for r in range(th * tw):
                out[ty * nw + tx, r] = (ty * th + r // tw) * w + tx * tw + r % tw
    return out


def to_tiles(x: torch.Tensor, h: int, w: int, nh: int, nw: int) -> torch.Tensor:
    """[B, h * w, ...] -> [B * nh * nw, th * tw, ...] by rearrange (no index table)."""
    B, rest = x.shape[0], x.shape[2:]
    th, tw = h // nh, w // nw
    x = x.reshape(B, nh, th, nw, tw, *rest)
    x = x.permute(0, 1, 3, 2, 4, *range(5, 5 + len(rest)))
    return x.reshape(B * nh * nw, th * tw, *rest)


def from_tiles(x: torch.Tensor, B: int, h: int, w: int, nh: int, nw: int) -> torch.Tensor:
    """The inverse of to_tiles: [B * nh * nw, th * tw, ...] -> [B, h * w, ...]."""
    rest = x.shape[2:]
    th, tw = h // nh, w // nw
    x = x.reshape(B, nh, nw, th, tw, *rest)
    x = x.permute(0, 1, 3, 2, 4, *range(5, 5 + len(rest)))
    return x.reshape(B, h * w, *rest)


def tiled_attention_f64(q, k, v, h, w, nh, nw, scale, with_abs=False):
    """q, k, v [B, h * w, heads, d] (any float format) -> softmax(q k^T scale) v inside every tile, float64, same shape:
    rearrange, softmax attention per tile, rearrange back.  with_abs: also A = P |V| (the gate's magnitude term)."""
    B = q.shape[0]
    qt, kt, vt = (to_tiles(t.double(), h, w, nh, nw).transpose(1, 2) for t in (q, k, v))     # [B', heads, nt, d]
    p = torch.softmax(torch.matmul(qt, kt.transpose(-1, -2)) * scale, -1)
    o = from_tiles(torch.matmul(p, vt).transpose(1, 2), B, h, w, nh, nw)
    if not with_abs:
        return o
    return o, from_tiles(torch.matmul(p, vt.abs()).transpose(1, 2), B, h, w, nh, nw)


def tile_gate(ref, A, v, h, w, nh, nw, dtype):
    """The P3 gate of attention_cases at the TILE's key count.  ref, A, v: [B, h * w, heads, d] -> gate of that shape."""
    B, n, H, d = ref.shape
    nt, T = n // (nh * nw), nh * nw
    flat = lambda t: to_tiles(t, h, w, nh, nw).reshape(B * T * nt, H * d)      # noqa: E731
    g = AC.gate_p3(flat(ref), flat(A), flat(v), B * T, H, nt, d, dtype)
    return from_tiles(g.reshape(B * T, nt, H, d), B, h, w, nh, nw)
