"""The fused denoising loop: one launch program per step, replayed eagerly or as a hipGraph.

One step (reference: /root/reference/powerpaint/pipelines/pipeline_PowerPaint.py:988-1041,
pipeline_PowerPaint_Brushnet_CA.py:1384-1466, pipeline_PowerPaint_ControlNet.py:1663-1741): per network one head launch
(time-embedding row of the per-schedule table, x_in[:, 0:4] <- cat([latents] * 2) without a copy of the cat, GroupNorm
accumulators zeroed) and the network's plan, side networks first, their residuals staying in HBM as NHWC; then the
scheduler's step launch on the fp32 latents (CFG combine + step), by family (schedulers.py: `step_launch`, `noise_for`):

    family                       head launch           step launch            state (`_keep[2]`)   noise `run` draws per row
    DDIM                         pp_step_head          pp_cfg_sched_step      none                 eta > 0: every row
    DPM-Solver++, PNDM, UniPC    pp_step_head          pp_cfg_sched_step      1, 5, 4 slots        none
    LCM                          pp_step_head          pp_cfg_lcm_step        none                 every row but the last
    Euler, Euler a               pp_step_head_scaled   pp_cfg_sigma_step      none                 Euler a: every row; Euler drops
    Heun, DPM2, DPM2 a, LMS      pp_step_head_scaled   pp_cfg_ksampler_step   4 slots              DPM2 a: every row; else none
(pp_step_head_scaled: the networks see latents / sqrt(sigma^2 + 1), `scale_model_input`; one row = one network evaluation.)
Behind it pp_ddim_variance_noise (DDIM, eta > 0) and pp_latent_blend (ppt-v1 with a 4-channel UNet: the known region noised
to the next timestep).  The step launch's last block moves the step counter on where nothing behind it reads the counter;
else pp_step_advance does.  No host->device traffic and no host synchronisation inside the loop.

Perturbed-attention guidance (`pag_scale > 0`, powerpaint_amd/pag.py): every network runs (2 + do_cfg) B items, `[uncond, cond,
cond]` or `[cond, cond]`, the last segment perturbed inside the UNet; the head launch replicates the latents over all of them.
In front of the step launch pp_pag_combine writes  e_u + g (e_c - e_u) + s_i (e_c - e_p)  into segment 0 of eps, s_i read from
a device table with one scale per schedule row, and the step launch runs with cfg = 0 on that segment.  The scales are data:
a new scale pair reaches a captured graph without a re-capture.

`guidance_rescale > 0` with CFG (powerpaint_amd/guidance.py, diffusers' rescale_noise_cfg): pp_cfg_rescale stands where
pp_pag_combine stands (with PAG's table when PAG is on, replacing that launch): the combine, then per sample the factor
phi sqrt(SSD(e_c) / SSD(combine)) + 1 - phi, into segment 0; the step launch runs with cfg = 0.  phi lives in a one-float
device cell that `run` refills: a new value reaches a captured graph without a re-capture.  0, or no CFG: the program without it.

Several ControlNets (`side` = a MultiControlNetModel, pipeline_PowerPaint_ControlNet.py:306,1678-1694): one runtime per
net (own arena, time-embedding table, hoisted control-image embedding, twin-prefix decision); the step is
    head(net 0) .. head(net N-1), head(UNet), plan(net 0) .. plan(net N-1), plan(UNet), scheduler step
in ONE stream and ONE hipGraph without parallel branches.  The UNet is wired to net 0's residual buffers; the first net
of a step overwrites them and every later net's zero convs add to them in place through the GEMM epilogue's `res1`
(NetRuntime.chained_step_calls): the sum costs no launch and no pass over the residuals.  A net whose guidance window
is closed at a step (scale 0) is LEFT OUT of that step: one program and one captured graph per distinct set of active
nets (at most 2 N + 1 over a schedule), cached on the loop and picked per step on the host; with no net active the
set's program zeroes the shared buffers itself.

Which program a step runs: `_sets` maps a set of active side nets to a `_StepSet` -- its program, captured graph and
zero-conv launch records, each as a pair [full, DeepCache-shallow].  Several ControlNets: one entry per tuple of active nets;
every other loop: the one entry under `_all`.  `_build` assembles every program from `_parts[shallow]`, `_resolve` picks (and
captures) what every step of a call replays before the first step, `_stale` is the one rule for a graph captured with other
by-value arguments.

A scheduler that is not one of powerpaint_amd.schedulers (any object with the diffusers protocol the reference
duck-types: `.timesteps`, `.scale_model_input`, `.step(...)`, e.g. the UniPC scheduler app.py:197 installs) is driven
the way the reference drives it: the network part of the step is the same captured launch program, the guidance
combine and the scheduler's own `.step` run as that object's tensor code on the device, once per step.
"""
import os
from collections import namedtuple
from typing import Callable, List, Optional

import torch

from .. import _lib as L
from .. import guidance as GDM
from .. import pag as PAGM
from ..engine import Plan
from ..schedulers import _SchedulerBase


def _temb_table_enabled() -> bool:
    """(lab) PP_LAB=1 PP_TEMB_TABLE=0: every step runs the time-embedding chain again."""
    return not (os.environ.get("PP_LAB") == "1" and os.environ.get("PP_TEMB_TABLE", "1") == "0")


_Keep = namedtuple("_Keep", "ts step m_prev latents")      # what `bind` leaves for `run`: the device tensors one step reads and moves


class _StepSet:
    """The step programs of one set of active side networks.  `program`, `graph` and `records` are pairs indexed by `shallow`
    (False: the full plans, True: DeepCache's shallow ones); `records`: per included net the launch records its scale is
    written into (several ControlNets only); `scales`: the scales last written; `baked`: `_baked()` at the graphs' capture."""
    __slots__ = ("active", "included", "program", "graph", "records", "scales", "baked")

    def __init__(self, active, included):
        self.active, self.included = active, included
        self.program, self.graph, self.records = [None, None], [None, None], [{}, {}]
        self.scales = self.baked = None


class DenoiseLoop:
    def __init__(self, unet, scheduler, side=None, side_kind: Optional[str] = None, keep_closed_nets: bool = False):
        """keep_closed_nets (several ControlNets only): a net whose guidance window is closed at a step still runs, with
        scale 0, as the reference does (pipeline_PowerPaint_ControlNet.py:1651-1658,1681) -- same numbers, a wasted forward
        pass; the default leaves its launches out of the step.  The pipelines never pass it; it exists to check the
        skipping against."""
        self.foreign = not isinstance(scheduler, _SchedulerBase)     # duck-typed scheduler: its own .step per step
        if self.foreign and not (hasattr(scheduler, "step") and hasattr(scheduler, "timesteps")):
            raise TypeError(f"{type(scheduler).__name__} does not follow the scheduler protocol (.timesteps, .step)")
        self.unet, self.scheduler, self.side, self.side_kind = unet, scheduler, side, side_kind
        self.lib = L.lib()
        self._key = None
        self.keep_closed_nets = bool(keep_closed_nets)
        self._multi = False           # several ControlNets bound: one entry of self._sets per set of active nets, else ONE entry
        self._sets, self._all = {}, ()             # active nets -> _StepSet; the default entry's key: every side net active
        self._parts = {}                           # shallow -> dict(heads, skips, tail): what `_build` assembles programs from
        self.rt = self.side_rt = None
        self.side_rts = []
        self.latents: Optional[torch.Tensor] = None
        self._keep: Optional[_Keep] = None
        # what `bind` takes from its call: guidance (PAG pair, rescale phi, a foreign scheduler's CFG), blend buffers, noise
        self._pag = self._rescale = self._blend = self._guess_ramp = self._gen = None
        self._do_cfg, self._g, self._eta, self._noisy, self._noise_dtype = False, 0.0, 0.0, False, torch.float32
        self._extra_step_kwargs = {}
        self._temb, self._temb_tables = {}, {}     # per runtime: the time-embedding launches its head replaces; their tables
        # device tensors at stable addresses (`_stable`): what each was made as; what the PAG table / phi cell were last filled with
        self._made, self._filled = {}, {}
        self._ticket = self._var_noise = self._pag_table = self._phi_cell = None
        self._blend_x0 = self._blend_mask = self._blend_noise = self._f_ts = self._f_step = self._f_x = None

    def _default(self, what: str, shallow: bool):
        ent = self._sets.get(self._all)
        return getattr(ent, what)[shallow] if ent is not None else None

    # the default entry's: the step program (several ControlNets: every net active -- flops, tools) and its captured graph;
    # DeepCache: the step over the networks' shallow plans, and its graph
    program = property(lambda self: self._default("program", False))
    program_shallow = property(lambda self: self._default("program", True))
    graph = property(lambda self: self._default("graph", False))
    graph_shallow = property(lambda self: self._default("graph", True))

    def _stable(self, name: str, shape, dtype=torch.float32, device=None) -> torch.Tensor:
        """The loop's device tensor `name` at a stable address (a captured graph reads it): allocated, as zeros, only when the
        shape, dtype or device asked for changed -- and what it was last filled with is forgotten with it."""
        made = (tuple(shape), dtype, str(device))
        if self._made.get(name) != made:
            setattr(self, name, torch.zeros(made[0], dtype=dtype, device=device))
            self._made[name] = made
            self._filled.pop(name, None)
        return getattr(self, name)

    # ------------------------------------------------------------------
    def bind(self, latents_shape, do_cfg: bool, guidance_scale: float, prompt_embeds, prompt_embeds_side=None,
             static_inputs=(), side_static_inputs=(), controlnet_cond=None, side_scale: float = 1.0,
             guess_mode: bool = False, eta: float = 0.0, generator=None, noise_dtype=torch.float32, blend=None,
             timestep_cond=None, added_cond_kwargs=None, ip_adapter_masks=None, pag_scale: float = 0.0,
             pag_adaptive_scale: float = 0.0, guidance_rescale: float = 0.0):
        """Compile the per-step program.  latents_shape = (B, 4, h, w) of the *un-duplicated* latents.
        ip_adapter_masks: `cross_attention_kwargs["ip_adapter_masks"]` of the call, [adapters, 1, H, W]; the UNet only, as the
        image embeds.  Their values are device memory the UNet's launches read (NetRuntime.set_ip_masks): new masks of the
        same count reach a captured graph without a re-capture.
        added_cond_kwargs: {"image_embeds": [...]} of a UNet with IP-Adapters (pipeline_PowerPaint_Brushnet_CA.py:1363-1366,
        1430-1441: the UNet only, never the side network); copied in and projected once per call (NetRuntime.set_ip_embeds).
        blend = (image_latents [1,4,h,w], mask [1,1,h,w], noise [B,4,h,w]): the `num_channels_unet == 4` branch of the
        ppt-v1 loop body (pipeline_PowerPaint.py:1025-1039) -- after every scheduler step the unmasked region is
        replaced by the init image's latents noised to the NEXT timestep.
        eta > 0 with this package's DDIM (the only scheduler whose `step` takes it, pipeline_PowerPaint.py:536-551):
        the step program gains `latents += std_dev_t * z`; `run` draws z from `generator` before every step, in
        `noise_dtype`, exactly where the reference's `scheduler.step` calls `randn_tensor`.
        An LCMScheduler (which ignores eta, as `prepare_extra_step_kwargs` never hands it over) consumes such a z on every
        step but the last of its schedule, inside its own step launch (pp_cfg_lcm_step).
        timestep_cond ([B or 1, d], pipeline_PowerPaint_Brushnet_CA.py:1351-1357,1434): the guidance embedding of a UNet with
        `time_cond_proj_dim`; the UNet only (the side network gets none, :1411-1419).  The rows of the time-embedding table
        depend on it: they are refilled when it changes.
        guess_mode (pipeline_PowerPaint_Brushnet_CA.py:1394-1425, pipeline_PowerPaint_ControlNet.py:1669-1702): the
        side network sees only the conditional half of a CFG pair (its inputs -- `prompt_embeds_side`, conditioning
        latents / control image -- arrive un-duplicated) with its residual scales log-spaced from 0.1 to 1; the
        unconditional half of the UNet batch gets zeros.
        pag_scale > 0 (diffusers' PAGMixin): perturbed-attention guidance in the transformers `unet.pag_layers()`; per-call
        inputs arrive as without it (un-duplicated or as the CFG pair) and are laid out `[.., cond, cond]` here.  The scale
        pair is no part of the plan key: `_fill_pag_table` writes one scale per schedule row into device memory.
        guidance_rescale > 0 with do_cfg (diffusers' rescale_noise_cfg): pp_cfg_rescale in front of the step launch.  Whether it
        is on is part of the key; its value is not: `run` writes it into a one-float device cell.  Without CFG: no effect."""
        B, sch = latents_shape[0], self.scheduler
        pag = float(pag_scale) > 0.0
        if pag:
            PAGM.check_supported(tome=getattr(self.unet.net, "tome", None) is not None and self.unet.net.tome.ratio > 0,
                                 guess_mode=bool(guess_mode))
            if getattr(self.unet.net, "deepcache", None) is not None:
                raise L.PPError("DeepCache together with perturbed-attention guidance (PAG, pag_scale > 0) is not implemented: "
                                "DeepCacheSDHelper.disable() first, or pag_scale = 0")
        if self.latents is None or tuple(self.latents.shape) != tuple(latents_shape):
            self.latents = torch.zeros(latents_shape, dtype=torch.float32, device=self.unet.device)
        lat = self.latents
        self._eta = float(eta) if (not self.foreign and sch.takes_eta) else 0.0
        self._gen, self._noise_dtype = generator, noise_dtype
        self._extra_step_kwargs = {}
        if self.foreign:                                     # prepare_extra_step_kwargs for a duck-typed scheduler
            import inspect
            names = set(inspect.signature(sch.step).parameters)
            self._extra_step_kwargs = {k: v for k, v in (("eta", eta), ("generator", generator)) if k in names}
        else:
            sch.set_eta(self._eta)
        # does the bound scheduler's step consume noise the host draws per step?  (stochastic DDIM, LCM, the ancestral classes)
        self._noisy = (not self.foreign) and bool(sch.step_noise)
        if blend is not None and not self.foreign and sch.blend_refused:
            raise L.PPError(f"{type(sch).__name__}: the known-region blend of a 4-channel UNet is not implemented -- "
                            f"{sch.blend_refused}")
        # a sigma-space scheduler: the networks' input is scaled per row of the schedule, at the head of the step
        in_div = sch.in_div_table() if (not self.foreign and sch.scales_input) else None
        if in_div is not None and not _temb_table_enabled():
            raise L.PPError(f"{type(sch).__name__} needs the time-embedding table: without it (PP_TEMB_TABLE=0) the step has "
                            f"no head launch to scale the network input in")
        self._blend = self._blend_buffers(blend, latents_shape)
        half = bool(guess_mode and do_cfg)                   # side network on the conditional half only
        Be = PAGM.segments(do_cfg) * B if pag else (2 * B if do_cfg else B)
        Bs = B if half else Be
        nets, side, controlnet_cond, side_scale = self._resolve_side(controlnet_cond, side_scale, guess_mode)
        multi = nets is not None and len(nets) > 1
        rt, side_rt, side_rts = self._prepare_runtimes(
            latents_shape, Be, Bs, do_cfg, half, guess_mode, nets, side, prompt_embeds, prompt_embeds_side, static_inputs,
            side_static_inputs, controlnet_cond, side_scale, timestep_cond, added_cond_kwargs, ip_adapter_masks, pag=pag)
        # DeepCache: every network of the loop is patched (each runtime then holds a shallow plan next to the full one) or none
        deep = [getattr(r, "shallow_plan", None) is not None for r in side_rts + [rt]]
        if any(deep) and not all(deep):
            raise L.PPError("DeepCache is enabled on some networks of this pipeline and not on others: enable it on the pipeline "
                            "(DeepCacheSDHelper(pipe)), so that every network is full or shallow together")
        if self.foreign:
            ts, step, src, mp = self._foreign_state(latents_shape, do_cfg, guidance_scale)
        else:
            # scheduler state: DPM m_{i-1}; PNDM history + saved sample; UniPC; Heun / DPM2 / DPM2 ancestral / LMS: three
            # derivative slots + the saved sample (DDIM, LCM and the Euler classes keep none)
            ts, step, src, mp = sch.timesteps_f32(), sch.step_counter(), lat, sch.m_prev(lat) if sch.state_slots > 0 else None
        # token merging: one row of destination windows per network evaluation, drawn once per call; the match launches pick
        # their row by the step counter, so a replayed graph merges around fresh windows at every step (no re-capture)
        for r in side_rts + [rt]:
            if r.tome_blocks():
                r.tome_bind(step.data_ptr())
                r.tome_fill(int(ts.numel()), r.net.tome_state)
        key = (tuple(latents_shape), bool(do_cfg), bool(guess_mode), self._noisy, float(guidance_scale), id(rt.step_plan),
               tuple(id(r.step_plan) for r in side_rts) if side_rts else None, type(sch), ts.data_ptr(), step.data_ptr(),
               0 if self.foreign else sch.coef_table().data_ptr(), mp.data_ptr() if mp is not None else 0, src.data_ptr(),
               _temb_table_enabled(), int(ts.numel()), tuple(getattr(r.net.params, "version", 0) for r in [rt] + side_rts),
               tuple(b.data_ptr() for b in self._blend) if self._blend is not None else None,
               sch.renoise_table().data_ptr() if (self._blend is not None and not self.foreign) else 0,
               in_div.data_ptr() if in_div is not None else 0)
        self._pag = (float(pag_scale), float(pag_adaptive_scale)) if pag else None
        if pag:                                  # (the table's address is part of the key, the scales in it are not: `run` fills it)
            key += (("pag", 0 if self.foreign else self._stable("_pag_table", (int(ts.numel()),), device=ts.device).data_ptr()),)
        self._rescale = GDM.check_guidance_rescale(guidance_rescale) if do_cfg else 0.0
        self._rescale = self._rescale if self._rescale > 0.0 else None
        if self._rescale is not None:            # (the cell's address is part of the key, phi in it is not: `run` fills it)
            key += (("rescale", 0 if self.foreign else self._stable("_phi_cell", (1,), device=ts.device).data_ptr()),)
        if key == self._key and self.program is not None:
            # The conditioning scale is a by-value argument of the zero-conv launches: `prepare` has patched the launch
            # records (eager runs see it), but a graph captured with another value still carries the old one.
            if self._stale(self._sets[self._all]):
                self._sets[self._all].graph = [None, None]
            return self
        self._key = key
        tail = self._tail_launches(rt, lat, mp, step, do_cfg, guidance_scale).calls
        self.rt, self.side_rt, self.side_rts = rt, side_rt, side_rts
        self._multi, self._sets, self._parts, self._all = multi, {}, {}, tuple(range(len(side_rts)))
        # DeepCache: one more program, the shallow plans between the same kind of head launches and the SAME tail -- the step
        # counter, the scheduler tables and the PAG / phi cells are read and moved by both programs alike
        for shallow in (False, True) if all(deep) else (False,):
            heads, skips = self._head_launches(side_rts, rt, ts, step, src, Be, Bs, do_cfg or pag, in_div, shallow=shallow)
            self._parts[shallow] = dict(heads=heads, skips=skips, tail=tail)
        ent = self._entry(self._all)
        if all(deep):
            self._build(ent, True)
        self._keep = _Keep(ts, step, mp, lat)
        return self

    # ---- the parts of `bind`, in its order
    def _blend_buffers(self, blend, latents_shape):
        """Loop-owned fp32 copies of `blend` at stable addresses (a captured graph reads them); first image / mask only."""
        if blend is None:
            return None
        _, Cl, h, w = latents_shape
        dev = self.unet.device
        x0, mk, nz = blend
        want = (("_blend_x0", (1, Cl, h, w)), ("_blend_mask", (1, 1, h, w)), ("_blend_noise", latents_shape))
        bufs = tuple(self._stable(name, sh, device=dev) for name, sh in want)
        for b_, v in zip(bufs, (x0[:1], mk[:1], nz)):
            b_.copy_(v.to(device=dev, dtype=torch.float32).reshape(b_.shape))
        return bufs

    def _resolve_side(self, controlnet_cond, side_scale, guess_mode):
        """-> (a MultiControlNetModel's nets or None, the network to `prepare`, control images and scales per net); sets the
        guess-mode ramp.  Several nets get one runtime each; a wrapper around ONE net is that net (same plans, same launches)."""
        nets = list(self.side.nets) if (self.side is not None and hasattr(self.side, "nets")) else None
        multi = nets is not None and len(nets) > 1
        side = self.side if (nets is None or multi) else nets[0]
        if nets is not None:
            if self.side_kind != "controlnet":
                raise L.PPError("a list of side networks is a ControlNet feature (MultiControlNetModel)")
            controlnet_cond = self.side.per_net(controlnet_cond, "controlnet_cond")
            if not isinstance(side_scale, (list, tuple)):
                side_scale = [side_scale] * len(nets)
            side_scale = [float(v) for v in self.side.per_net(side_scale, "side_scale")]
            if not multi:
                controlnet_cond, side_scale = controlnet_cond[0], side_scale[0]
        side0 = nets[0] if multi else side                   # (global_pool_conditions is read from nets[0], :1536-1540)
        # guess mode scales the n residuals by logspace(-1, 0, n) * conditioning_scale (BrushNet_CA.py:905-928): `run`'s
        # per-step scalar schedule is expanded the same way before it is patched into the zero-conv launches
        self._guess_ramp = None
        if guess_mode and side is not None and not side0.config.global_pool_conditions:
            self._guess_ramp = [float(v) for v in torch.logspace(-1, 0, len(side0.net._zero_conv_specs()))]
        return nets, side, controlnet_cond, side_scale

    def _prepare_runtimes(self, latents_shape, Be, Bs, do_cfg, half, guess_mode, nets, side, prompt_embeds,
                          prompt_embeds_side, static_inputs, side_static_inputs, controlnet_cond, side_scale, timestep_cond,
                          added_cond_kwargs, ip_adapter_masks=None, pag: bool = False):
        """-> (rt, side_rt, side_rts): every network prepared, the UNet wired to the side residuals, static channels loaded.
        The CFG pair is built here, as `cat([latents] * 2)` (pipeline_PowerPaint.py:990): where every other network input
        is CFG-duplicated as well, the two halves of a forward pass are identical until the prompt enters and the
        networks run that prefix once (`twin`, SDNet.build_step).  A static input counts as duplicated when it arrives
        with the un-duplicated batch (load_input copies it to both halves) or when its halves compare equal.
        pag: every per-call input goes into the PAG layout first (pag.layout: the third segment gets the second's inputs, the
        side networks' included, as diffusers' PAG pipelines feed theirs); no twin prefix."""
        B, Cl, h, w = latents_shape
        multi = nets is not None and len(nets) > 1
        if pag:
            lay3 = lambda t: PAGM.layout(t, B, bool(do_cfg))      # noqa: E731
            prompt_embeds, prompt_embeds_side = lay3(prompt_embeds), lay3(prompt_embeds_side)
            static_inputs = [(lay3(t), c) for t, c in static_inputs]
            side_static_inputs = [(lay3(t), c) for t, c in side_static_inputs]
            controlnet_cond = [lay3(c) for c in controlnet_cond] if isinstance(controlnet_cond, (list, tuple)) \
                else lay3(controlnet_cond)
            if timestep_cond is not None:
                timestep_cond = timestep_cond[:1]              # (one value over the batch: _check_timestep_cond)
            if added_cond_kwargs and "image_embeds" in added_cond_kwargs:      # [neg, pos] -> [neg, pos, pos]
                added_cond_kwargs = dict(added_cond_kwargs, image_embeds=[lay3(e) for e in added_cond_kwargs["image_embeds"]])

        def halves_equal(t):
            if t is None or not torch.is_tensor(t):
                return False
            if t.shape[0] == B:
                return True
            return t.shape[0] == 2 * B and bool(torch.equal(t[:B], t[B:]))

        twin_u = bool(do_cfg) and not pag and all(halves_equal(t) for t, _ in static_inputs)
        # (the control image goes through set_cond, which accepts the un-duplicated batch as well and copies it to both halves)
        twin_s = bool(do_cfg) and not pag and not half and all(halves_equal(t) for t, _ in side_static_inputs) and \
            (self.side_kind == "brushnet" or multi or halves_equal(controlnet_cond))
        if self.side is not None and self.side.dtype != self.unet.dtype:
            # the fused loop hands the side network's residuals to the UNet as raw NHWC arena pointers, every step: both
            # must store activations in the same 16-bit format (the reference raises a dtype error in its first conv)
            raise L.PPError(f"{type(self.side).__name__} computes in {self.side.dtype}, the UNet in {self.unet.dtype}: "
                            f"load both with the same torch_dtype")
        side_rt, side_rts, wiring_kw = None, [], {}
        if side is not None:
            if half and prompt_embeds_side.shape[0] == Be:
                prompt_embeds_side = prompt_embeds_side.chunk(2)[1]
            if self.side_kind == "brushnet":
                side_rt = side.prepare((Bs, Cl, h, w), prompt_embeds_side, side_scale, bool(guess_mode), half, twin=twin_s)
                d, m, u = side.outputs()
                wiring_kw = dict(down_block_add_samples=d, mid_block_add_sample=m, up_block_add_samples=u)
            elif multi:
                # every net on the same latents and prompt, its own control image (and so its own twin-prefix decision);
                # the UNet reads net 0's residual buffers, which every step's program fills with the sum
                side_rts = [net.prepare((Bs, Cl, h, w), prompt_embeds_side, cond, sc, bool(guess_mode), half,
                                        twin=twin_s and halves_equal(cond))
                            for net, cond, sc in zip(nets, controlnet_cond, side_scale)]
                d, m = nets[0].outputs()
                wiring_kw = dict(down_block_additional_residuals=d, mid_block_additional_residual=m)
            else:
                side_rt = side.prepare((Bs, Cl, h, w), prompt_embeds_side, controlnet_cond, side_scale,
                                       bool(guess_mode), half, twin=twin_s)
                d, m = side.outputs()
                wiring_kw = dict(down_block_additional_residuals=d, mid_block_additional_residual=m)
        if side_rt is not None:
            side_rts = [side_rt]
        if timestep_cond is not None:
            wiring_kw["timestep_cond"] = timestep_cond
        if added_cond_kwargs is not None:
            wiring_kw["added_cond_kwargs"] = added_cond_kwargs
        if ip_adapter_masks is not None:
            wiring_kw["ip_adapter_masks"] = ip_adapter_masks
        if pag:
            wiring_kw["pag_batch"] = B
        rt = self.unet.prepare((Be, self.unet.config.in_channels, h, w), prompt_embeds, twin=twin_u, **wiring_kw)
        # one-time (per call) static channels of the UNet / side inputs
        rt.load_input(list(static_inputs))
        if side_rt is not None and side_static_inputs:
            side_rt.load_input(list(side_static_inputs))
        return rt, side_rt, side_rts

    def _foreign_state(self, latents_shape, do_cfg, guidance_scale):
        """-> (ts, step, src, no state) of a duck-typed scheduler: the timestep table, the step counter and the network
        input (scaled by the scheduler per step), all owned by the loop."""
        dev = self.unet.device
        tsv = torch.as_tensor(self.scheduler.timesteps).detach().to(dev, torch.float32).contiguous()
        self._do_cfg, self._g = bool(do_cfg), float(guidance_scale)
        return (self._stable("_f_ts", tsv.shape, device=dev).copy_(tsv), self._stable("_f_step", (1,), torch.int32, dev),
                self._stable("_f_x", latents_shape, device=dev), None)

    def _head_launches(self, side_rts, rt, ts, step, src, Be, Bs, do_cfg, in_div, shallow: bool = False):
        """-> (heads, skips), per runtime: the launches at the head of the step; the plan indices they replace.
        in_div: the table a sigma-space scheduler scales the networks' input by, else None.
        shallow: for the runtimes' shallow plans (DeepCache); the time-embedding tables are the full plans' (same rows)."""
        lib, sch = self.lib, self.scheduler
        B, Cl, h, w = src.shape
        hw = h * w
        mod = B if do_cfg else 0
        if not shallow:
            self._temb = {}
        heads, skips = {}, {}
        for r in side_rts + [rt]:
            prog = Plan()
            heads[id(r)] = prog.calls
            skips[id(r)] = set()
            plan = r.shallow_plan if shallow else r.step_plan
            info = self._temb_split(r, ts, plan) if _temb_table_enabled() else None
            x = r.lay["x_in"]
            nb_r = Be if r is rt else Bs                    # (guess mode: the side network takes `latents` as is)
            calls = plan.calls
            zero = calls[0] if (calls and calls[0][2] == "zero_u64") else None
            if info is not None:
                if not shallow:
                    self._temb[id(r)] = info
                skips[id(r)] |= set(info["idx"])
            if info is not None and zero is not None:
                # time-embedding row + network input + accumulator zeroing: ONE launch at the head of the step (pp_step_head)
                skips[id(r)].add(0)
                head = (info["table"].data_ptr(), step.data_ptr(), info["out"], info["total"], src.data_ptr(), nb_r, Cl, hw,
                        mod if nb_r != B else 0, x.ptr, x.C, 0, L.dtype_code(r.net.dtype), zero[1][0], zero[1][1])
                fn, div = (lib.pp_step_head, ()) if in_div is None else (lib.pp_step_head_scaled, (in_div.data_ptr(),))
                prog.add("step_head", fn, *head, *div)
                continue
            if in_div is not None:
                raise L.PPError(f"{type(r.net).__name__}: its step plan has no fused head launch, which "
                                f"{type(sch).__name__} needs to scale the network input")
            if info is not None:
                prog.add("temb_row", lib.pp_embed_splice, info["table"].data_ptr(), None, step.data_ptr(), info["out"], 1,
                         info["total"] * 4)
            else:
                prog.add("step_select_t", lib.pp_step_select_t, ts.data_ptr(), step.data_ptr(), r.lay["t_dev"])
            prog.add("nchw_to_nhwc", lib.pp_nchw_to_nhwc, src.data_ptr(), 0, nb_r, Cl, hw, mod if nb_r != B else 0,
                     x.ptr, x.C, 0, L.dtype_code(r.net.dtype))
        return heads, skips

    def _tail_launches(self, rt, lat, mp, step, do_cfg, guidance_scale):
        """-> the launches behind the networks: the scheduler's step launch (`step_launch` of its family), DDIM's variance
        noise, the known-region blend, and the counter's advance where the step launch does not do it itself."""
        prog = Plan()
        lib, sch = self.lib, self.scheduler
        # the step launch's last block moves the counter on (the ticket) where nothing behind it reads it: no pp_step_advance
        fold_advance = (not self.foreign) and not (self._eta > 0) and self._blend is None and \
            not (os.environ.get("PP_LAB") == "1" and os.environ.get("PP_FOLD_ADVANCE", "1") == "0")     # (lab: the two launches)
        if not self.foreign:
            if fold_advance:
                self._stable("_ticket", (1,), torch.int32, lat.device)
            # (a step that reads no noise: any valid address)
            noise = self._stable("_var_noise", lat.shape, lat.dtype, lat.device) if self._noisy else lat
            if self._rescale is not None:
                # guidance_rescale (CFG is on): the combine -- PAG's three-way one with its table when PAG is on, in the place
                # of pp_pag_combine -- and the per-sample rescale into segment 0; the step launch behind it runs with cfg = 0
                B = lat.shape[0]
                prog.add("cfg_rescale", lib.pp_cfg_rescale, rt.outputs["eps"], 3 if self._pag is not None else 2,
                         float(guidance_scale), self._pag_table.data_ptr() if self._pag is not None else None,
                         self._phi_cell.data_ptr(), step.data_ptr(), B, lat.numel() // B)
                do_cfg = False
            elif self._pag is not None:
                # perturbed-attention guidance: the three-way (two-way) combine into segment 0 of eps, its scale read from this
                # row of the table; the step launch behind it takes segment 0 as it is (cfg = 0)
                prog.add("pag_combine", lib.pp_pag_combine, rt.outputs["eps"], int(do_cfg), float(guidance_scale),
                         self._pag_table.data_ptr(), step.data_ptr(), lat.numel())
                do_cfg = False
            prog.add(*sch.step_launch(rt.outputs["eps"], int(do_cfg), float(guidance_scale), lat.data_ptr(),
                                      mp.data_ptr() if mp is not None else None, noise.data_ptr(), lat.numel(),
                                      step.data_ptr(), self._ticket.data_ptr() if fold_advance else None))
            if self._eta > 0:
                prog.add(*sch.variance_launch(lat.data_ptr(), noise.data_ptr(), lat.numel(), step.data_ptr()))
            if self._blend is not None:
                x0, mk, nz = self._blend
                B, Cl, h, w = lat.shape
                prog.add("latent_blend", lib.pp_latent_blend, lat.data_ptr(), x0.data_ptr(), mk.data_ptr(), nz.data_ptr(),
                         sch.renoise_table().data_ptr(), step.data_ptr(), B, Cl, h * w)
        if not fold_advance:
            prog.add("step_advance", lib.pp_step_advance, step.data_ptr())
        return prog

    # ---- perturbed-attention guidance: the per-row scale table (fp32 [rows of the schedule]); guidance_rescale: the one-float cell
    def _fill_pag_table(self, ts):
        """s_i of every schedule row (pag.scale_rows) -> the device table, when the scale pair or the timesteps changed."""
        host = getattr(self.scheduler, "_ts_host", None) if not self.foreign else None
        tsl = [float(v) for v in (host if host is not None else ts).tolist()]
        want = (self._pag, tuple(tsl))
        if want != self._filled.get("_pag_table"):
            self._pag_table.copy_(torch.tensor(PAGM.scale_rows(self._pag[0], self._pag[1], tsl), dtype=torch.float32))
            self._filled["_pag_table"] = want

    def _fill_phi_cell(self):
        """This call's guidance_rescale -> the device cell, when it changed."""
        if self._rescale != self._filled.get("_phi_cell"):
            self._phi_cell.copy_(torch.tensor([self._rescale], dtype=torch.float32))
            self._filled["_phi_cell"] = self._rescale

    # ---- the program table: one entry (programs, graphs, launch records) per set of active side nets
    def _entry(self, active) -> _StepSet:
        """The entry of the side nets `active` (ascending indices), its full program assembled when it is new.  Several
        ControlNets: the heads and plans of those nets only; keep_closed_nets: every net is in, the closed ones get scale 0.
        Every other loop has the one entry `_all`, every side net in it."""
        active = tuple(active)
        ent = self._sets.get(active)
        if ent is None:
            included = list(active if (self._multi and not self.keep_closed_nets) else self._all)
            ent = self._sets[active] = _StepSet(active, included)
            self._build(ent, False)
        return ent

    def _build(self, ent: _StepSet, shallow: bool) -> Plan:
        """`ent.program[shallow]` from `_parts[shallow]`: the heads of the included side nets and the UNet's, every network's
        plan (shallow: its shallow plan) without the launches its head replaces, the tail -- the same call tuples in every
        program.  Several ControlNets: the side plans as copies whose zero convs write net 0's residual buffers, the first
        one overwriting them, the others adding in place (NetRuntime.chained_step_calls; the records kept for `_set_scales`);
        no net included -> one zeroing launch over the buffers (the UNet plan is never rebuilt)."""
        P, rts = self._parts[shallow], self.side_rts
        plan_of = (lambda r: r.shallow_plan) if shallow else (lambda r: r.step_plan)
        own = lambda r: [c for i, c in enumerate(plan_of(r).calls) if i not in P["skips"][id(r)]]      # noqa: E731
        prog = Plan()
        for r in [rts[k] for k in ent.included] + [self.rt]:
            prog.calls += P["heads"][id(r)]
            prog.flops += plan_of(r).flops_executed       # (a program's `flops`: what its launches execute)
        for n, k in enumerate(ent.included):
            if self._multi:
                calls, ent.records[shallow][k] = rts[k].chained_step_calls(rts[0], accumulate=n > 0, scale=0.0,
                                                                          skip=P["skips"][id(rts[k])], shallow=shallow)
            else:
                calls = own(rts[k])
            prog.calls += calls
        if self._multi and not ent.included:
            prog.add("zero_u64", self.lib.pp_zero_u64, *rts[0].residual_block())
        prog.calls += own(self.rt) + P["tail"]
        ent.program[shallow], ent.scales = prog, None      # (the scales are written again, into both programs' records)
        return prog

    # ---- time-embedding table
    def _temb_split(self, r, ts, plan=None):
        """(plan: the runtime's step plan, or its shallow plan -- whose own four launches and result address are returned, with
        the step plan's table.)  The four leading time-embedding launches of a network's step plan (`timestep_embedding` + three
        `linear_skinny`: sinusoid, time_embedding.linear_1/2, all time_emb_proj rows at once) and where their result
        lands; plus a [rows of the schedule][temb_total] fp32 table at a stable address.  None = unexpected layout."""
        plan = plan if plan is not None else r.step_plan
        calls = plan.calls
        idx = [i for i, c in enumerate(calls) if c[2] in ("timestep_embedding", "linear_skinny")]
        if len(idx) != 4 or idx != list(range(idx[0], idx[0] + 4)) or calls[idx[0]][2] != "timestep_embedding":
            return None
        a = calls[idx[-1]][1]
        out, total = int(a[6]), int(a[5])
        tabs, k = self._temb_tables, (id(r), int(ts.numel()), total)
        if k not in tabs:
            tabs[k] = dict(table=torch.zeros(int(ts.numel()), total, dtype=torch.float32, device=ts.device), ts=None,
                           plan=None)
        ent = tabs[k]
        pver = getattr(r.net.params, "version", 0)
        if plan is r.step_plan and (ent["plan"] is not r.step_plan or ent.get("pver") != pver):     # new plan / weights rewritten in place: stale rows
            ent["plan"], ent["ts"], ent["pver"], ent["hkey"] = r.step_plan, None, pver, None
        return dict(idx=idx, out=out, total=total, table=ent["table"], ent=ent, rt=r)

    def _fill_temb_tables(self):
        """(Re)compute the table rows when the timestep table changed since they were made: per row the network's own
        four launches, eagerly, with the step counter pointing at that row."""
        ts, step = self._keep.ts, self._keep.step
        for info in self._temb.values():
            ent, r = info["ent"], info["rt"]
            # (this package's schedulers keep the timesteps on the host: compare there -- a device compare synchronises)
            host = getattr(self.scheduler, "_ts_host", None) if not self.foreign else None
            cver = getattr(r, "tcond_version", 0)          # (guidance-embedded UNet: the rows depend on the call's embedding)
            if ent.get("cver", 0) != cver:
                ent["ts"], ent["hkey"], ent["cver"] = None, None, cver
            hkey = tuple(host.tolist()) if host is not None else None
            if hkey is not None and ent.get("hkey") == hkey:
                continue
            if hkey is None and ent["ts"] is not None and ent["ts"].shape == ts.shape and torch.equal(ent["ts"], ts):
                continue
            stream = torch.cuda.current_stream().cuda_stream
            saved = step.clone()
            view = r.arena.view(info["out"], (info["total"],), torch.float32)
            calls = [r.step_plan.calls[i] for i in info["idx"]]
            for i in range(int(ts.numel())):
                step.fill_(i)
                L.check(self.lib.pp_step_select_t(ts.data_ptr(), step.data_ptr(), r.lay["t_dev"], stream), "pp_step_select_t")
                for fn, args, name in calls:
                    L.check(fn(*args, stream), name)
                info["table"][i].copy_(view)
            step.copy_(saved)
            ent["ts"] = ts.clone()
            ent["hkey"] = hkey

    def _side_scale(self, v):
        """One entry of `run`'s scale schedule as the side runtime stores it (guess mode: the per-residual ramp)."""
        ramp = self._guess_ramp
        return tuple(r * v for r in ramp) if ramp is not None else v

    def _scale_now(self):
        sc = getattr(self.side_rt, "_scale", None)
        return tuple(sc) if isinstance(sc, (list, tuple)) else sc

    # ---- by-value kernel arguments: a captured graph carries the values of its capture
    def _baked(self):
        """What a graph captured now bakes in: the side scale patched into the one side runtime's plan (several ControlNets:
        none, `_set_scales` drops the graphs it outdates) and the IP-Adapter scales of the UNet's launches."""
        return self._scale_now(), self.rt.ip_scales()

    def _stale(self, ent: _StepSet) -> bool:
        return ent.baked != self._baked()

    def _set_scales(self, ent: _StepSet, scales):
        """Several ControlNets: write this call's per-net scales into the set's zero-conv launch records, of both programs
        (by-value kernel arguments: graphs captured with other values are dropped).  Within a call every scale of a set is
        constant.  (Same zero convs in every net: the one guess-mode ramp serves each.)"""
        want = tuple(float(scales[k]) if k in ent.active else 0.0 for k in ent.included)
        if want == ent.scales:
            return
        full, sh = ent.records
        for k, v in zip(ent.included, want):
            ramp = self._guess_ramp
            vals = [r * v for r in ramp] if ramp is not None else [v] * len(full[k])
            for rec, x in zip(full[k], vals):
                rec.scale = float(x)
            if k in sh:
                for rec, p_ in zip(sh[k], self.side_rts[k].shallow_plan.zero_conv_pos):
                    rec.scale = float(vals[p_])
        ent.scales, ent.graph = want, [None, None]

    def _multi_schedule(self, scale_schedule, num_steps) -> List[_StepSet]:
        """Several ControlNets -> per step the set's entry, this call's scales written into it."""
        n = len(self.side_rts)
        if scale_schedule is None:
            raise L.PPError("several ControlNets need a per-step schedule of per-net scales")
        rows = [[float(v) for v in row] for row in scale_schedule[:num_steps]]
        if len(rows) < num_steps or any(len(r) != n for r in rows):
            raise L.PPError(f"scale_schedule must hold {num_steps} rows of {n} per-net scales")
        ents = [self._entry(k for k, v in enumerate(row) if v != 0.0) for row in rows]
        seen = {}
        for ent, row in zip(ents, rows):
            act = tuple(row[k] for k in ent.active)
            if seen.setdefault(ent.active, act) != act:
                raise L.PPError("the scale of an active ControlNet changed inside one call")
        if self._deep() and len(seen) > 1:
            raise L.PPError("DeepCache with several ControlNets whose set of active nets changes during the call (guidance "
                            "windows) is not implemented: one set per call, or DeepCacheSDHelper.disable()")
        for ent, row in zip(ents, rows):
            if self._deep() and ent.program[True] is None:      # (a set's shallow program: on demand)
                self._build(ent, True)
            self._set_scales(ent, row)
        return ents

    # ---- DeepCache: which program an evaluation runs
    def _deep(self) -> bool:
        return self.rt is not None and getattr(self.rt, "shallow_plan", None) is not None and \
            getattr(self.rt.net, "deepcache", None) is not None

    def shallow_rows(self, num_steps: int) -> List[bool]:
        """Per evaluation of a call (one per row of the schedule `run` steps through, counted from 0 at every call): does it
        run the shallow program?  Evaluation e is full iff e % cache_interval == 0; without DeepCache every one is."""
        if not self._deep():
            return [False] * num_steps
        iv = int(self.rt.net.deepcache.interval)
        return [e % iv != 0 for e in range(num_steps)]

    def capture(self, ent: Optional[_StepSet] = None):
        """Capture one step (of the default entry, or of `ent`) into a hipGraph (torch.cuda.CUDAGraph).  The captured launches
        read the step counter from device memory, so the same graph serves every step.  A shallow graph captured with other
        by-value arguments goes with the full one."""
        ent = ent if ent is not None else self._sets[self._all]
        ent.baked = self._baked()
        ent.graph = [self._capture_program(ent.program[False]), None]

    def _capture_program(self, program):
        torch.cuda.synchronize()
        step = self._keep[1]
        saved_step = step.clone()
        saved_lat = self.latents.clone()
        saved_m = self._keep[2].clone() if self._keep[2] is not None else None
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            program.run(s.cuda_stream)             # warm-up outside capture (func attributes, lazy module load)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            program.run(torch.cuda.current_stream().cuda_stream)
        # undo the warm-up's side effects
        step.copy_(saved_step)
        self.latents.copy_(saved_lat)
        if saved_m is not None:
            self._keep[2].copy_(saved_m)
        torch.cuda.synchronize()
        return g

    def _resolve(self, scale_schedule, num_steps, use_graph):
        """Before the first step of a call -> (per step what `_launch` launches, the per-step scales `_patch_scale` gets when
        the one side net's scale varies inside the call, else None).  Per step: the entry (several ControlNets: the set
        active at that step, this call's scales written; else the one entry, a constant scale patched in), its full or
        shallow program, or with use_graph that program's graph, captured here where there is none or a stale one -- the
        full one of an entry first: its warm-up leaves a cache tensor the shallow one's reads.  A varying scale runs eagerly."""
        patches = None
        if self._multi:
            ents = self._multi_schedule(scale_schedule, num_steps)
        else:
            ents = [self._sets[self._all]] * num_steps
            # (a wrapper around one net hands rows of one scale)
            sched = [s[0] if isinstance(s, (list, tuple)) else s for s in scale_schedule or ()]
            if len(set(sched)) > 1:
                use_graph, patches = False, sched if self.side_rt is not None else None
            elif sched and self.side_rt is not None and self._scale_now() != self._side_scale(sched[0]):
                self.side_rt._patch_scale(self._side_scale(sched[0]))    # (a previous call may have left a windowed value)
        steps = []
        for ent, sh in zip(ents, self.shallow_rows(num_steps)):
            if use_graph and (ent.graph[False] is None or self._stale(ent)):
                self.capture(ent)
            if use_graph and sh and ent.graph[True] is None:
                ent.graph[True] = self._capture_program(ent.program[True])
            steps.append((ent.graph if use_graph else ent.program)[sh])
        return steps, patches

    @staticmethod
    def _launch(what, stream):
        """One step: a program's launches into `stream`, or the replay of its captured graph."""
        what.run(stream) if isinstance(what, Plan) else what.replay()

    def run(self, latents: torch.Tensor, num_steps: int, use_graph: bool = True,
            callback: Optional[Callable] = None, timesteps=None, scale_schedule: Optional[List[float]] = None):
        """Runs `num_steps` steps starting from step counter 0.  Returns the fp32 latents tensor (owned by the loop)."""
        if self.foreign:
            return self._run_foreign(latents, num_steps, use_graph, callback, timesteps, scale_schedule)
        self.scheduler.reset()
        if self._ticket is not None:
            self._ticket.zero_()       # (an aborted launch must not leave the step counter's ticket mid-count)
        if self._keep.m_prev is not None:
            self._keep.m_prev.zero_()
        self._fill_temb_tables()
        if self._pag is not None:
            self._fill_pag_table(self._keep.ts)
        if self._rescale is not None:
            self._fill_phi_cell()
        self.latents.copy_(latents.to(self.latents.device, torch.float32))
        steps, patches = self._resolve(scale_schedule, num_steps, use_graph)
        stream = torch.cuda.current_stream().cuda_stream
        for i in range(num_steps):
            if patches is not None:
                self.side_rt._patch_scale(self._side_scale(patches[i]))
            # this row's noise, by the scheduler's own rule (stream-ordered before the step that consumes it)
            z = self.scheduler.noise_for(self.scheduler.begin_index + i, self.latents.shape, self._gen, self.latents.device,
                                         self._noise_dtype)
            if z is not None:
                self._var_noise.copy_(z)
            self._launch(steps[i], stream)
            if callback is not None:
                callback(i, timesteps[i] if timesteps is not None else None, self.latents)
        self._check_faults()
        return self.latents

    def _check_faults(self, blocking: bool = False):
        """Where a plan combines split-K in-kernel (launches of 2 / 4 co-resident splits: pp_gemm_combine_ctr_bytes()): the
        plan's fault word is examined WITHOUT a synchronisation -- copied to pinned memory behind this call's work, read by a
        later call (NetRuntime.check_faults).  `flush_faults()` is the blocking form for a caller that synchronises anyway."""
        for r in [self.rt] + self.side_rts:
            if r is not None and r.combines_in_kernel():
                r.check_faults(blocking=blocking)

    def flush_faults(self):
        """Synchronise and raise if any in-kernel split-K combine since the last check reported a fault."""
        self._check_faults(blocking=True)

    def _run_foreign(self, latents, num_steps, use_graph, callback, timesteps, scale_schedule):
        """Duck-typed scheduler: network part = the captured program (eps lands in the UNet runtime's fp32 output), then
        the guidance combine and `scheduler.step` exactly as the reference's loop body does
        (pipeline_PowerPaint.py:1018-1023)."""
        sch = self.scheduler
        tl = timesteps if timesteps is not None else sch.timesteps
        # The timestep table the captured program indexes holds exactly the timesteps this run steps through: with
        # `strength < 1` the pipelines hand over `scheduler.timesteps[t_start:]` (get_timesteps,
        # pipeline_PowerPaint.py:713-720), and the networks must see those -- not the head of the full schedule that
        # `bind` uploaded -- while `scheduler.step` receives the same values below.
        tsv = torch.as_tensor(tl).detach().to(self._f_ts.device, torch.float32).reshape(-1)
        if tsv.numel() > self._f_ts.numel():
            raise L.PPError(f"{tsv.numel()} timesteps for a loop bound to a schedule of {self._f_ts.numel()}")
        if num_steps > tsv.numel():
            raise L.PPError(f"{num_steps} steps requested, {tsv.numel()} timesteps given")
        self._f_ts[:tsv.numel()].copy_(tsv)
        self._fill_temb_tables()
        self._f_step.zero_()
        lat = latents.to(self.latents.device, torch.float32).clone()
        steps, patches = self._resolve(scale_schedule, num_steps, use_graph)
        stream = torch.cuda.current_stream().cuda_stream
        for i in range(num_steps):
            t = tl[i]
            x = sch.scale_model_input(lat, t) if hasattr(sch, "scale_model_input") else lat
            self._f_x.copy_(x)
            if patches is not None:
                self.side_rt._patch_scale(self._side_scale(patches[i]))
            self._launch(steps[i], stream)
            eps = self.rt.eps_tensor()
            # (guidance_rescale is only ever on with CFG: the conditional prediction is the second segment of two or three)
            text = eps.chunk(3 if self._pag is not None else 2)[1] if self._rescale is not None else None
            if self._pag is not None:
                eps = PAGM.combine(eps, self._do_cfg, self._g, PAGM.scale_rows(self._pag[0], self._pag[1], [float(t)])[0])
            elif self._do_cfg:
                eu, ec = eps.chunk(2)
                eps = eu + self._g * (ec - eu)
            if text is not None:
                eps = GDM.rescale_noise_cfg(eps, text, self._rescale)
            lat = sch.step(eps, t, lat, **self._extra_step_kwargs, return_dict=False)[0].to(torch.float32)
            if self._blend is not None:                       # pipeline_PowerPaint.py:1025-1039, with the scheduler's own add_noise
                x0, mk, nz = self._blend
                proper = x0
                if i < len(tl) - 1:
                    proper = sch.add_noise(x0, nz, torch.as_tensor(tl[i + 1]).reshape(1).to(x0.device)).to(torch.float32)
                lat = (1 - mk) * proper + mk * lat
            if callback is not None:
                callback(i, t, lat)
        self.latents.copy_(lat)
        self._check_faults()
        return self.latents
