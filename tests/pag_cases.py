"""Perturbed-attention guidance (diffusers' PAGMixin, 0.30), restated independently of powerpaint_amd/pag.py: the layer
resolver, the per-row scale rule and the combine in float64, the identity "attention", and the oracle side of the network and
pipeline tests (a context manager that patches `OM.BasicTransformerBlock.forward`, and the denoising loops over the patched
oracle networks).  Shared by tests/test_pag.py (CPU) and tests/test_pag_kernels_gpu.py / tests/test_pag_gpu.py.

The rules (the specification):
  switch     PAG is on iff pag_scale > 0
  batch      [uncond, cond, cond] with CFG, [cond, cond] without; the LAST segment is perturbed; every CFG-duplicated input
             follows the same layout
  perturb    in a selected attn1 the perturbed items get to_out(to_v(norm1(x))): the attention output is V itself
  layers     every entry of pag_applied_layers is used as re.search(entry, name) over the self-attention modules' names; a
             match is discarded when the last dot-component of entry and name are both numeric and equal; an entry that
             selects nothing raises ValueError naming it
  scale      s_i = pag_scale if pag_adaptive_scale == 0 else max(pag_scale - pag_adaptive_scale * (1000 - t_i), 0)
  combine    e = e_u + g (e_c - e_u) + s_i (e_c - e_p)   |   e = e_c + s_i (e_c - e_p) without CFG
"""
import re

import numpy as np
import torch


# ------------------------------------------------------------------------------------------------ host rules
def resolve(layers, names):
    layers = [layers] if isinstance(layers, str) else list(layers)
    out = []
    for entry in layers:
        tail = entry.split(".")[-1]
        hit = []
        for n in names:
            last = n.split(".")[-1]
            fake = tail.isnumeric() and last.isnumeric() and tail == last
            if re.search(entry, n) is not None and not fake:
                hit.append(n)
        if not hit:
            raise ValueError(f"no self-attention module matches {entry!r}")
        out += [n for n in hit if n not in out]
    return sorted(out, key=list(names).index)


def scale_f64(pag_scale, pag_adaptive_scale, t):
    if pag_adaptive_scale == 0:
        return np.float64(pag_scale)
    return max(np.float64(pag_scale) - np.float64(pag_adaptive_scale) * (1000.0 - np.float64(t)), np.float64(0.0))


def combine_f64(eps, cfg, g, s):
    """eps: [3][n] (cfg) or [2][n] array -> segment 0 after the combine, float64."""
    e = np.asarray(eps, dtype=np.float64)
    if cfg:
        return e[0] + np.float64(g) * (e[1] - e[0]) + np.float64(s) * (e[1] - e[2])
    return e[0] + np.float64(s) * (e[0] - e[1])


def identity_v_ref(vt, n):
    """vt: [items][C][ldvt] -> [items][n][C]: what pp_attn_identity_v writes for those items."""
    return vt[:, :, :n].transpose(1, 2).contiguous()


def layout(t, B, cfg):
    """A CFG pair [2B] -> [first, second, second]; an un-duplicated [B] tensor -> one copy per segment."""
    segs = 3 if cfg else 2
    if t.shape[0] == B:
        return torch.cat([t] * segs)
    assert cfg and t.shape[0] == 2 * B
    return torch.cat([t, t[B:]])


def attn1_names(model):
    """The self-attention modules of an oracle network by name, in registration order (diffusers' `named_modules()`)."""
    return [n for n, _ in model.named_modules() if n.endswith(".attn1")]


# ------------------------------------------------------------------------------------------------ the oracle side
class OraclePAG:
    """Patches OM.BasicTransformerBlock.forward: in the blocks of `unet` whose attn1 is in `names`, the last `n` batch items
    get  x + to_out(to_v(norm1(x)))  in place of the self-attention; blocks of other networks (BrushNet, ControlNet) and
    unselected blocks run unchanged.  `hits` counts the perturbed evaluations per name."""

    def __init__(self, unet, names, n):
        from oracle import sd_modules as OM
        self.OM, self.n = OM, int(n)
        mods = dict(unet.named_modules())
        self.sel = {id(mods[nm[:-len(".attn1")]]): nm for nm in names}
        assert len(self.sel) == len(names)
        self.hits = {nm: 0 for nm in names}

    def __enter__(self):
        self.orig, this = self.OM.BasicTransformerBlock.forward, self

        def fwd(blk, x, ctx):
            nm = this.sel.get(id(blk))
            if nm is None or not this.n:
                return this.orig(blk, x, ctx)
            this.hits[nm] += 1
            h = blk.norm1(x)
            keep = blk.attn1(h[:-this.n])
            pert = blk.attn1.to_out[0](blk.attn1.to_v(h[-this.n:]))
            x = x + torch.cat([keep, pert])
            x = x + blk.attn2(blk.norm2(x), ctx)
            return x + blk.ff(blk.norm3(x))

        self.OM.BasicTransformerBlock.forward = fwd
        return self

    def __exit__(self, *exc):
        self.OM.BasicTransformerBlock.forward = self.orig


class TwoControlNets:
    """Several oracle ControlNets summed as MultiControlNetModel does, with this step's per-net scales from the window schedule
    `rows` (a closed window: scale 0, the net is left out) and each net's own control image for the whole PAG batch."""

    def __init__(self, nets, conds, rows):
        self.nets, self.conds, self.rows, self.i = nets, conds, rows, 0

    def __call__(self, x, t, encoder_hidden_states, controlnet_cond=None, conditioning_scale=None, guess_mode=False):
        down = mid = None
        for net, cond, sc in zip(self.nets, self.conds, self.rows[self.i]):
            d, m = net(x, t, encoder_hidden_states=encoder_hidden_states, controlnet_cond=cond, conditioning_scale=sc,
                       guess_mode=guess_mode)
            down = list(d) if down is None else [a + b for a, b in zip(down, d)]
            mid = m if mid is None else mid + m
        self.i += 1
        return down, mid


def _guided(noise_pred, cfg, g, s):
    if cfg:
        u, c, p = noise_pred.chunk(3)
        return u + g * (c - u) + s * (c - p)
    c, p = noise_pred.chunk(2)
    return c + s * (c - p)


@torch.no_grad()
def loop_v2_pag(unet, brushnet, scheduler, names, latents, conditioning_latents, prompt_embeds, prompt_embedsU, steps,
                guidance_scale, pag_scale, pag_adaptive_scale=0.0, generator=None):
    """The BrushNet loop (oracle/loops.py: loop_v2) with PAG: every network on (2 + cfg) B items, the third segment fed the
    second's inputs, the UNet's selected self-attentions perturbed for the last B.  prompt_embeds / prompt_embedsU /
    conditioning_latents arrive as loop_v2 takes them ([uncond, cond] with CFG)."""
    import inspect
    scheduler.set_timesteps(steps)
    cfg = guidance_scale > 1.0
    B = latents.shape[0]
    segs = 3 if cfg else 2
    pe, peU, cl = layout(prompt_embeds, B, cfg), layout(prompt_embedsU, B, cfg), layout(conditioning_latents, B, cfg)
    extra = {"generator": generator} if "generator" in inspect.signature(scheduler.step).parameters else {}
    latents = latents * scheduler.init_noise_sigma
    for t in scheduler.timesteps:
        x = scheduler.scale_model_input(torch.cat([latents] * segs), t)
        down, mid, up = brushnet(x, t, encoder_hidden_states=pe, brushnet_cond=cl, conditioning_scale=1.0, guess_mode=False)
        with OraclePAG(unet, names, B):
            noise_pred = unet(x, t, encoder_hidden_states=peU, down_block_add_samples=list(down), mid_block_add_sample=mid,
                              up_block_add_samples=list(up))[0]
        s = float(scale_f64(pag_scale, pag_adaptive_scale, float(t)))
        latents = scheduler.step(_guided(noise_pred, cfg, guidance_scale, s), t, latents, **extra)[0]
    return latents


@torch.no_grad()
def loop_v1_pag(unet, scheduler, names, latents, mask, masked_image_latents, prompt_embeds, steps, guidance_scale, pag_scale,
                pag_adaptive_scale=0.0, controlnet=None, control_image=None, image_latents=None, noise=None):
    """The ppt-v1 loop (oracle/loops.py: loop_v1; optionally a ControlNet callable, optionally the 4-channel blend) with PAG.
    mask / masked_image_latents are un-duplicated [B]; prompt_embeds is the CFG pair; control_image whatever `controlnet`
    takes for (2 + cfg) B items."""
    scheduler.set_timesteps(steps)
    cfg = guidance_scale > 1.0
    B = latents.shape[0]
    segs = 3 if cfg else 2
    pe = layout(prompt_embeds, B, cfg)
    latents = latents * scheduler.init_noise_sigma
    ts = scheduler.timesteps
    for i, t in enumerate(ts):
        x = scheduler.scale_model_input(torch.cat([latents] * segs), t)
        kw = {}
        if controlnet is not None:
            down, mid = controlnet(x, t, encoder_hidden_states=pe, controlnet_cond=control_image, conditioning_scale=None,
                                   guess_mode=False)
            kw = dict(down_block_additional_residuals=down, mid_block_additional_residual=mid)
        if unet.config.in_channels == 9:
            x = torch.cat([x, torch.cat([mask] * segs), torch.cat([masked_image_latents] * segs)], dim=1)
        with OraclePAG(unet, names, B):
            noise_pred = unet(x, t, encoder_hidden_states=pe, **kw)[0]
        s = float(scale_f64(pag_scale, pag_adaptive_scale, float(t)))
        latents = scheduler.step(_guided(noise_pred, cfg, guidance_scale, s), t, latents)[0]
        if unet.config.in_channels == 4 and image_latents is not None:
            proper = image_latents[:1]
            if i < len(ts) - 1:
                proper = scheduler.add_noise(proper, noise, torch.tensor([ts[i + 1]]))
            latents = (1 - mask[:1]) * proper + mask[:1] * latents
    return latents
