"""DeepCache restated, independent of powerpaint_amd: wrappers around oracle.sd_modules networks that keep the evaluation counter
and the cache, so they stand in for the networks in the oracle's loops (oracle/loops.py).

Parity with the `DeepCache` package (`DeepCacheSDHelper`) is UNPINNED: the package is not installed where this was written,
the rule below is a restatement from its public description (made deterministic, and valid for any layers_per_block), not a
comparison against its output.

The rule, for one network (UNet, BrushNet or ControlNet trunk):
  S[0..n-1]  the skip tensors in the order the down path produces them: conv_in's output, then each down block's layer outputs
             and its downsampler's output (SD-1.5: n = 12; TINY: n = 4)
  U[0..n-1]  the up layers (resnet, plus its transformer where the block has one) in execution order; U[j] consumes S[n-1-j]
  k          cache_branch_id + 1, 0 <= cache_branch_id <= n - 2
A FULL evaluation is the network as it is; it also keeps c, the hidden state handed to U[n-1-k]: the output of whatever
precedes that layer (the previous up layer, the upsampler in front of it, for k = n - 1 the mid block), with every BrushNet /
ControlNet add the network applies to that output.  A SHALLOW evaluation computes the time embedding, conv_in, the down modules
that produce S[1..k], then with h = c the up layers U[n-1-k..n-1] and every upsampler between them, conv_norm_out and conv_out;
every live up layer gets the skip it gets in the full network; the mid block and everything else do not run.
BrushNet: the rule on its own trunk with its own c; shallow, only the zero-conv residuals of live positions exist (down 0..k, the
live up layers and upsamplers), the UNet adds them where the full network adds them, the mid residual is not used.  ControlNet:
the down path up to S[k] and the zero convs 0..k, added to the UNet's S[0..k]; no cache; guess_mode's logspace scales keep their
full-network values at the live positions.
Schedule: evaluations count from 0 (`reset()`); evaluation e is full iff e % cache_interval == 0.

The walk below (`_down`, `_up`) runs the FULL network as well: with cache_interval = 1 its outputs equal the plain oracle's bit
for bit (tests/test_deepcache.py), which is what makes it a restatement of the oracle and not a second network.
"""
import torch
import torch.nn.functional as F

from oracle import sd_modules as OM

TINY = dict(block_out_channels=(320, 640), layers_per_block=1,
            down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"))

# where a shallow evaluation produces no residual: a one-element tensor the oracle loops' `cat([zeros_like(d), d])` (guess mode)
# accepts and that no shallow consumer ever reads
DEAD = torch.zeros(1)

# ---------------------------------------------------------------------------------------------------------- index table
# (n, live down modules behind conv_in, live up modules, the module whose output is c), written out by hand from the rule.
# A layer is named by its resnet (its transformer, where the block has one, goes with it).
_D0, _D1, _D2 = "down_blocks.0.", "down_blocks.1.", "down_blocks.2."
_U0, _U1, _U2, _U3 = "up_blocks.0.", "up_blocks.1.", "up_blocks.2.", "up_blocks.3."
_SD_TOP_UP = [_U3 + "resnets.0", _U3 + "resnets.1", _U3 + "resnets.2"]
_SD_U2 = [_U2 + "resnets.0", _U2 + "resnets.1", _U2 + "resnets.2", _U2 + "upsamplers.0"]
_SD_U1 = [_U1 + "resnets.0", _U1 + "resnets.1", _U1 + "resnets.2", _U1 + "upsamplers.0"]
_SD_U0 = [_U0 + "resnets.0", _U0 + "resnets.1", _U0 + "resnets.2", _U0 + "upsamplers.0"]
_SD_DOWN = ["conv_in", _D0 + "resnets.0", _D0 + "resnets.1", _D0 + "downsamplers.0", _D1 + "resnets.0", _D1 + "resnets.1",
            _D1 + "downsamplers.0", _D2 + "resnets.0", _D2 + "resnets.1", _D2 + "downsamplers.0", "down_blocks.3.resnets.0",
            "down_blocks.3.resnets.1"]
INDEX_SD15 = {
    0: (12, _SD_DOWN[:2], _SD_TOP_UP[1:], _U3 + "resnets.0"),
    1: (12, _SD_DOWN[:3], _SD_TOP_UP, _U2 + "upsamplers.0"),
    2: (12, _SD_DOWN[:4], [_U2 + "resnets.2", _U2 + "upsamplers.0"] + _SD_TOP_UP, _U2 + "resnets.1"),
    3: (12, _SD_DOWN[:5], [_U2 + "resnets.1", _U2 + "resnets.2", _U2 + "upsamplers.0"] + _SD_TOP_UP, _U2 + "resnets.0"),
    5: (12, _SD_DOWN[:7], [_U1 + "resnets.2", _U1 + "upsamplers.0"] + _SD_U2 + _SD_TOP_UP, _U1 + "resnets.1"),
    10: (12, _SD_DOWN[:12], _SD_U0 + _SD_U1 + _SD_U2 + _SD_TOP_UP, "mid_block"),
}
INDEX_TINY = {
    0: (4, ["conv_in", _D0 + "resnets.0"], [_U1 + "resnets.0", _U1 + "resnets.1"], _U0 + "upsamplers.0"),
    1: (4, ["conv_in", _D0 + "resnets.0", _D0 + "downsamplers.0"],
        [_U0 + "resnets.1", _U0 + "upsamplers.0", _U1 + "resnets.0", _U1 + "resnets.1"], _U0 + "resnets.0"),
    2: (4, ["conv_in", _D0 + "resnets.0", _D0 + "downsamplers.0", _D1 + "resnets.0"],
        [_U0 + "resnets.0", _U0 + "resnets.1", _U0 + "upsamplers.0", _U1 + "resnets.0", _U1 + "resnets.1"], "mid_block"),
}

# the program the fused loop picks per evaluation ("F" full, "S" shallow), by hand
SCHEDULES = {
    # (evaluations, cache_interval) -> pattern
    (7, 3): "FSSFSSF",            # 7 DDIM steps
    (7, 2): "FSFSFSF",            # 4 Heun steps = 7 table rows (the last step has no second stage)
    (3, 3): "FSS",                # strength 0.5 of 6 DDIM steps: 3 evaluations, the first of the call is full
    (5, 1): "FFFFF",
}


def schedule(evaluations: int, cache_interval: int) -> str:
    return "".join("F" if e % cache_interval == 0 else "S" for e in range(evaluations))


# ---------------------------------------------------------------------------------------------------------- networks
def tiny_oracle(kind, seed=0, in_channels=9):
    """The oracle half of test_models_gpu.make_tiny (same seeds, same constructor order): fp32, matrix weights on the bf16 grid."""
    torch.manual_seed(seed)
    if kind == "unet":
        o = OM.UNet2DConditionModel(in_channels=in_channels, **TINY)
    elif kind == "brushnet":
        o = OM.randomize_zero_convs(OM.BrushNetModel(in_channels=4, conditioning_channels=5, **TINY))
    else:
        o = OM.randomize_zero_convs(OM.ControlNetModel(in_channels=4, **{k: v for k, v in TINY.items() if k != "up_block_types"}))
    with torch.no_grad():
        for _, p in o.named_parameters():
            if p.dim() >= 2:
                p.copy_(p.to(torch.bfloat16).float())
    return o.eval()


# (make_tiny's weights need no sharpening here: on fresh inputs a shallow evaluation of TINY differs from the plain oracle by
#  cosine 0.80 .. 0.91 and max-abs 0.6 .. 1.0 at cache_branch_id 0, 1 and 2, against a gate of 0.999 / 0.04 --
#  tests/test_deepcache.py::test_shallow_on_fresh_inputs_leaves_the_gate asserts it.)


# ---------------------------------------------------------------------------------------------------------- the walk
def skip_count(m) -> int:
    return 1 + sum(len(b.resnets) + (b.downsamplers is not None) for b in m.down_blocks)


def _down(m, h, emb, ctx, stop, adds=None):
    """S[0..stop] from h = S[0] (BrushNet's add on conv_in's output already applied to h, not to S[0]: the caller passes both).
    adds: the UNet's down_block_add_samples behind position 0, consumed in order.  -> (h, [S[1..stop]], names)"""
    S, names = [], []
    for i, blk in enumerate(m.down_blocks):
        for j, resnet in enumerate(blk.resnets):
            if len(S) == stop:
                return h, S, names
            h = resnet(h, emb)
            if blk.has_cross_attention:
                h = blk.attentions[j](h, encoder_hidden_states=ctx)[0]
            if adds is not None:
                h = h + adds.pop(0)
            S.append(h)
            names.append(f"down_blocks.{i}.resnets.{j}")
        if blk.downsamplers is not None:
            if len(S) == stop:
                return h, S, names
            h = blk.downsamplers[0](h)
            if adds is not None:
                h = h + adds.pop(0)
            S.append(h)
            names.append(f"down_blocks.{i}.downsamplers.0")
    return h, S, names


def _up(m, h, S, emb, ctx, first, c=None, adds=None, sized=False, prev="mid_block"):
    """The up path from layer `first` on.  h: the mid block's output (first == 0 or a full evaluation), ignored when `c` is
    given (a shallow evaluation enters on c).  S: the skip tensors, S[j] at index j (only those the live layers take need to be
    there).  adds: the UNet's up_block_add_samples BY POSITION (layers and upsamplers in execution order).  sized: BrushNet hands
    every upsampler the size of the skip tensor the next block takes (BrushNet_CA.py:874); the UNet does not.
    -> (h, outputs by position (None where nothing ran), c as seen at layer `first`, names of what ran, name of c's producer)"""
    n = len(S)
    outs, names, u, pos, kept, kept_name = [], [], 0, 0, None, None
    shallow = c is not None
    nb = len(m.up_blocks)
    for i, blk in enumerate(m.up_blocks):
        for j, resnet in enumerate(blk.resnets):
            if u == first:
                kept, kept_name = (c if shallow else h), prev
                h = kept
            if shallow and u < first:
                outs.append(None)
            else:
                h = resnet(torch.cat([h, S[n - 1 - u]], dim=1), emb)
                if blk.has_cross_attention:
                    h = blk.attentions[j](h, encoder_hidden_states=ctx)[0]
                outs.append(h)
                if adds is not None:
                    h = h + adds[pos]
                names.append(f"up_blocks.{i}.resnets.{j}")
            prev = f"up_blocks.{i}.resnets.{j}"
            u, pos = u + 1, pos + 1
        if blk.upsamplers is not None:
            if shallow and u - 1 < first:
                outs.append(None)
            else:
                size = S[n - 1 - u].shape[2:] if (sized and i != nb - 1) else None
                h = blk.upsamplers[0](h, size)
                outs.append(h)
                if adds is not None:
                    h = h + adds[pos]
                names.append(f"up_blocks.{i}.upsamplers.0")
            prev = f"up_blocks.{i}.upsamplers.0"
            pos += 1
    return h, outs, kept, names, kept_name


class _Cached:
    """Counter, cache and the delegation every wrapper shares."""

    def __init__(self, model, cache_interval=3, cache_branch_id=0):
        self.m = model
        self.n = skip_count(model)
        if not (isinstance(cache_interval, int) and cache_interval >= 1):
            raise ValueError("cache_interval")
        if not 0 <= cache_branch_id <= self.n - 2:
            raise ValueError("cache_branch_id")
        self.interval, self.k = cache_interval, cache_branch_id + 1
        self.reset()

    def reset(self):
        self.e, self.c, self.trace = 0, None, []

    def _next(self) -> bool:
        """-> is this evaluation shallow?"""
        shallow = self.e % self.interval != 0
        self.e += 1
        self.trace.append("S" if shallow else "F")
        return shallow

    @property
    def config(self):
        return self.m.config

    @property
    def dtype(self):
        return self.m.dtype


class DeepCacheUNet(_Cached):
    def __call__(self, sample, timestep, encoder_hidden_states, down_block_additional_residuals=None,
                 mid_block_additional_residual=None, down_block_add_samples=None, mid_block_add_sample=None,
                 up_block_add_samples=None, **unused):
        m, k, n = self.m, self.k, self.n
        shallow = self._next()
        ctx = encoder_hidden_states
        is_ctrl = mid_block_additional_residual is not None and down_block_additional_residuals is not None
        is_brush = down_block_add_samples is not None and mid_block_add_sample is not None and up_block_add_samples is not None
        with torch.no_grad():
            emb = OM._time_embed(m, sample, timestep)
            h = m.conv_in(sample)
            S0 = h
            dadds = list(down_block_add_samples) if is_brush else None
            if is_brush:
                h = h + dadds.pop(0)
            h, S, self.down_names = _down(m, h, emb, ctx, k if shallow else n - 1, dadds)
            S = [S0] + S
            if is_ctrl:
                S = [a + b for a, b in zip(S, down_block_additional_residuals)]
            if not shallow:
                h = m.mid_block(h, emb, ctx)
                if is_ctrl:
                    h = h + mid_block_additional_residual
                if is_brush:
                    h = h + mid_block_add_sample
            S = S + [None] * (n - len(S))
            h, _, kept, self.up_names, self.cache_name = _up(m, h, S, emb, ctx, n - 1 - k, c=self.c if shallow else None,
                                                              adds=list(up_block_add_samples) if is_brush else None)
            if not shallow:
                self.c = kept
            for lst in (down_block_add_samples, up_block_add_samples):      # (consumed destructively, as the network does)
                if isinstance(lst, list):
                    del lst[:]
            return (m.conv_out(F.silu(m.conv_norm_out(h))),)


class DeepCacheBrushNet(_Cached):
    def __call__(self, sample, timestep, encoder_hidden_states, brushnet_cond, conditioning_scale=1.0, guess_mode=False,
                 **unused):
        m, k, n = self.m, self.k, self.n
        shallow = self._next()
        ctx = encoder_hidden_states
        with torch.no_grad():
            emb = OM._time_embed(m, sample, timestep)
            h = m.conv_in_condition(torch.cat([sample, brushnet_cond], 1))
            S0 = h
            h, S, self.down_names = _down(m, h, emb, ctx, k if shallow else n - 1)
            S = [S0] + S
            mid = None
            if not shallow:
                h = m.mid_block(h, emb, ctx)
                mid = h
            Sx = S + [None] * (n - len(S))
            h, ups, kept, self.up_names, self.cache_name = _up(m, h, Sx, emb, ctx, n - 1 - k, c=self.c if shallow else None,
                                                               sized=True)
            if not shallow:
                self.c = kept
            feats = Sx + [mid] + ups
            zcs = list(m.brushnet_down_blocks) + [m.brushnet_mid_block] + list(m.brushnet_up_blocks)
            if guess_mode and not m.config.global_pool_conditions:
                scales = torch.logspace(-1, 0, len(zcs)) * conditioning_scale
            else:
                scales = [conditioning_scale] * len(zcs)
            res = [z(f) * sc if f is not None else DEAD for f, z, sc in zip(feats, zcs, scales)]
            self.live = [p for p, f in enumerate(feats) if f is not None]
            return res[:n], res[n], res[n + 1:]


class DeepCacheControlNet(_Cached):
    def __call__(self, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale=1.0, guess_mode=False,
                 **unused):
        m, k, n = self.m, self.k, self.n
        shallow = self._next()
        ctx = encoder_hidden_states
        with torch.no_grad():
            emb = OM._time_embed(m, sample, timestep)
            h = m.conv_in(sample) + m.controlnet_cond_embedding(controlnet_cond)
            S0 = h
            h, S, self.down_names = _down(m, h, emb, ctx, k if shallow else n - 1)
            S = [S0] + S
            mid = None if shallow else m.mid_block(h, emb, ctx)
            feats = S + [None] * (n - len(S)) + [mid]
            zcs = list(m.controlnet_down_blocks) + [m.controlnet_mid_block]
            if guess_mode and not m.config.global_pool_conditions:
                scales = torch.logspace(-1, 0, len(zcs)) * conditioning_scale
            else:
                scales = [conditioning_scale] * len(zcs)
            res = [z(f) * sc if f is not None else DEAD for f, z, sc in zip(feats, zcs, scales)]
            self.live = [p for p, f in enumerate(feats) if f is not None]
            return res[:n], res[n]

