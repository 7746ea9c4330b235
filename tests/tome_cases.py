"""Token merging (ToMe for Stable Diffusion, Bolya & Hoffman 2023) restated on the CPU in float64: what the pp_tome_* kernels
and the engine's token-merging path are tested against.  The algorithm is the `tomesd` package's
`bipartite_soft_matching_random2d` and `ToMeBlock` (`x = unmerge(attn1(merge(norm1(x)))) + x`, matching computed from the
block's input x); neither tomesd nor diffusers is a dependency of the tests, so parity with tomesd itself is unpinned.

Conventions shared with include/pp_hip.h ("Token merging"):
  * tokens of an h x w grid in row-major order; hsy = h // sy, wsx = w // sx windows; window (i, j) with in-window index k has
    its destination at token (i*sy + k // sx, j*sx + k % sx); every other token (leftover rows / columns included) is a source;
  * per source the destination with the highest cosine (an equal maximum: the lower destination token); the r sources with the
    highest best cosine are merged (an equal score: the lower token); a zero row has cosine 0 with everything;
  * merged sequence: the kept sources in ascending token order, then the destinations in ascending token order; a destination
    row is the plain mean of itself and the sources merged into it; unmerge copies row pos[t] to token t.
"""
import math
from typing import Dict, List, Optional

import torch

F64 = torch.float64


def downsample_of(orig_tokens: int, tokens: int) -> int:
    """tomesd's level of a block: ceil(sqrt(orig_tokens // tokens))."""
    return int(math.ceil(math.sqrt(orig_tokens // tokens)))


def eligible(orig_tokens: int, tokens: int, max_downsample: int) -> bool:
    return downsample_of(orig_tokens, tokens) <= max_downsample


def merged_count(n: int, ratio: float, nd: int) -> int:
    """r = int(n * ratio), capped at the number of source tokens."""
    return max(0, min(int(n * ratio), n - nd))


def window_count(h: int, w: int, sx: int, sy: int) -> int:
    return (h // sy) * (w // sx)


class Draws:
    """The window draws of a run: one torch.randint per eligible block per network evaluation, in execution order, shared by
    the batch.  No draw is made (and the generator is not advanced) when use_rand is off or the logical batch is odd."""

    def __init__(self, generator: Optional[torch.Generator], use_rand: bool = True):
        self.g, self.use_rand, self.count = generator, use_rand, 0

    def draw(self, h: int, w: int, sx: int, sy: int, logical_batch: int) -> torch.Tensor:
        hsy, wsx = h // sy, w // sx
        if not self.use_rand or logical_batch % 2 == 1:
            return torch.zeros(hsy * wsx, dtype=torch.uint8)
        self.count += 1
        return torch.randint(sy * sx, (hsy, wsx, 1), generator=self.g).reshape(-1).to(torch.uint8)


def partition(h: int, w: int, sx: int, sy: int, win: torch.Tensor):
    """-> (src tokens ascending, dst tokens ascending) of the window table row `win` [hsy*wsx]."""
    hsy, wsx = h // sy, w // sx
    is_dst = torch.zeros(h * w, dtype=torch.bool)
    for i in range(hsy):
        for j in range(wsx):
            k = int(win[i * wsx + j])
            is_dst[(i * sy + k // sx) * w + j * sx + k % sx] = True
    tok = torch.arange(h * w)
    return tok[~is_dst], tok[is_dst]


def cosines(x: torch.Tensor, src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """x [N, C] (any float dtype; evaluated in float64) -> cos [NS, ND]."""
    x = x.to(F64)
    nrm = x.norm(dim=-1, keepdim=True)
    m = torch.where(nrm > 0, x / nrm.clamp_min(1e-300), torch.zeros_like(x))
    return m[src] @ m[dst].T


def decide(x: torch.Tensor, h: int, w: int, sx: int, sy: int, win: torch.Tensor, r: int,
           best_override: Optional[torch.Tensor] = None, merged_override: Optional[torch.Tensor] = None) -> Dict[str, object]:
    """The decisions of one batch item: x [N, C].  Returns
         best [N] int64     destination token per source, -1 at destinations
         score [N] float64  its cosine, -2 at destinations
         merged [N] bool    the r merged sources
         pos [N] int64, rowtok [N - r] int64, lists: per destination rank the merged sources ascending
         best_margin [N]    best minus second-best cosine per source (inf with one destination; 0 at destinations)
         sel_margin         r-th minus (r+1)-th highest score (inf when r is 0 or every source is merged)
       best_override / merged_override: decisions taken from elsewhere (a GPU run) in place of the argmax / the selection."""
    n = h * w
    src, dst = partition(h, w, sx, sy, win)
    cos = cosines(x, src, dst)
    top = cos.max(dim=1).values
    first = (cos == top[:, None]).to(torch.int8).argmax(dim=1)          # the lowest destination among equal maxima
    best = torch.full((n,), -1, dtype=torch.int64)
    score = torch.full((n,), -2.0, dtype=F64)
    best[src] = dst[first]
    score[src] = top
    margin = torch.zeros(n, dtype=F64)
    if dst.numel() > 1:
        margin[src] = top - cos.scatter(1, first[:, None], -math.inf).max(dim=1).values
    else:
        margin[src] = math.inf
    if best_override is not None:
        best = best_override.to(torch.int64).clone()
        col = torch.searchsorted(dst, best[src])
        score[src] = cos[torch.arange(src.numel()), col]
    order = torch.sort(score[src], descending=True, stable=True).indices      # equal scores: ascending token
    merged = torch.zeros(n, dtype=torch.bool)
    merged[src[order[:r]]] = True
    s_sorted = score[src][order]
    sel_margin = float(s_sorted[r - 1] - s_sorted[r]) if 0 < r < src.numel() else math.inf
    if merged_override is not None:
        merged = merged_override.to(torch.bool).clone()
    kept = src[~merged[src]]
    rowtok = torch.cat([kept, dst])
    pos = torch.empty(n, dtype=torch.int64)
    pos[rowtok] = torch.arange(rowtok.numel())
    msrc = src[merged[src]]
    pos[msrc] = pos[best[msrc]]
    lists: List[List[int]] = [[] for _ in range(dst.numel())]
    for t in msrc.tolist():
        lists[int(pos[t]) - kept.numel()].append(t)
    return dict(src=src, dst=dst, best=best, score=score, merged=merged, pos=pos, rowtok=rowtok, lists=lists,
                best_margin=margin, sel_margin=sel_margin, nkept=int(kept.numel()))


def merge_rows(rows: torch.Tensor, d: Dict[str, object]) -> torch.Tensor:
    """rows [N, D] -> [N - r, D] float64: kept rows copied, destination rows the mean of themselves and their list."""
    rows = rows.to(F64)
    out = rows[d["rowtok"]].clone()
    for rank, lst in enumerate(d["lists"]):
        if lst:
            m = d["nkept"] + rank
            out[m] = (rows[int(d["rowtok"][m])] + rows[lst].sum(dim=0)) / (len(lst) + 1)
    return out


def unmerge_rows(rows: torch.Tensor, d: Dict[str, object]) -> torch.Tensor:
    return rows[d["pos"]]


def smooth_tokens(batch: int, h: int, w: int, c: int, seed: int, noise: float = 0.25) -> torch.Tensor:
    """[batch, h*w, c] float64: a few low spatial frequencies per channel plus noise -- neighbouring tokens are similar but no
    two are equal (what a hidden state looks like to the matching)."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=F64) / h, torch.arange(w, dtype=F64) / w, indexing="ij")
    out = torch.zeros(batch, h * w, c, dtype=F64)
    for k in range(3):
        a = torch.randn(batch, 1, c, generator=g, dtype=F64)
        ph = torch.rand(batch, 1, c, generator=g, dtype=F64) * 6.283185307179586
        fy, fx = torch.randint(0, 3, (2,), generator=g).tolist()
        arg = (6.283185307179586 * (fy * yy + fx * xx)).reshape(1, h * w, 1)
        out += a * torch.cos(arg + ph)
    return out + noise * torch.randn(batch, h * w, c, generator=g, dtype=F64)


def twin_tokens(batch: int, h: int, w: int, c: int, win: torch.Tensor, seed: int, sx: int = 2, sy: int = 2) -> torch.Tensor:
    """[batch, h*w, c] float64 with decisions that are far from ambiguous at any grid size: the destinations are independent
    Gaussian rows (cosines of about c^-1/2 with each other), every source is one of them plus noise of its own level, the levels
    spread evenly over [0.2, 1.0] in a random order -- one clear best destination per source, and best scores spaced
    by about 0.3 / sources."""
    g = torch.Generator().manual_seed(seed)
    src, dst = partition(h, w, sx, sy, win)
    x = torch.zeros(batch, h * w, c, dtype=F64)
    for b in range(batch):
        x[b, dst] = torch.randn(dst.numel(), c, generator=g, dtype=F64)
        twin = dst[torch.randint(dst.numel(), (src.numel(),), generator=g)]
        level = 0.2 + 0.8 * torch.randperm(src.numel(), generator=g).to(F64) / src.numel()
        x[b, src] = x[b, twin] + level[:, None] * torch.randn(src.numel(), c, generator=g, dtype=F64)
    return x
