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

A scheduler that is not one of powerpaint_amd.schedulers (any object with the diffusers protocol the reference
duck-types: `.timesteps`, `.scale_model_input`, `.step(...)`, e.g. the UniPC scheduler app.py:197 installs) is driven
the way the reference drives it: the network part of the step is the same captured launch program, the guidance
combine and the scheduler's own `.step` run as that object's tensor code on the device, once per step.
"""
import os
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
        self.program: Optional[Plan] = None
        self.graph = None
        self.program_shallow: Optional[Plan] = None     # DeepCache: the step over the networks' shallow plans, and its graph
        self.graph_shallow = None
        self._key = None
        self._graph_scale = None      # side-branch conditioning scale baked into the captured graph (by-value kernel arg)
        self.keep_closed_nets = bool(keep_closed_nets)
        self._multi = False           # several ControlNets bound: per-active-set programs (self._sets) instead of ONE program
        self._sets = {}
        self.side_rts = []
        self.latents: Optional[torch.Tensor] = None

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
            key += (("pag", 0 if self.foreign else self._pag_table_for(int(ts.numel()), ts.device).data_ptr()),)
        self._rescale = GDM.check_guidance_rescale(guidance_rescale) if do_cfg else 0.0
        self._rescale = self._rescale if self._rescale > 0.0 else None
        if self._rescale is not None:            # (the cell's address is part of the key, phi in it is not: `run` fills it)
            key += (("rescale", 0 if self.foreign else self._phi_cell_for(ts.device).data_ptr()),)
        if key == self._key and self.program is not None:
            # The conditioning scale is a by-value argument of the zero-conv launches: `prepare` has patched the launch
            # records (eager runs see it), but a graph captured with another value still carries the old one.
            if self.graph is not None and (self._scale_now() != self._graph_scale or
                                           rt.ip_scales() != getattr(self, "_graph_ip", ())):
                self.graph = None
            return self
        self._key = key
        heads, skips = self._head_launches(side_rts, rt, ts, step, src, Be, Bs, do_cfg or pag, in_div)
        tail = self._tail_launches(rt, lat, mp, step, do_cfg, guidance_scale)
        self.rt, self.side_rt, self.side_rts = rt, side_rt, side_rts
        self.graph = self.graph_shallow = None
        self.program_shallow = None
        self._assemble(multi, heads, skips, tail)
        if all(deep):
            # one more program: the shallow plans between the same kind of head launches and the SAME tail -- the step counter,
            # the scheduler tables and the PAG / phi cells are read and moved by both programs alike
            heads, skips = self._head_launches(side_rts, rt, ts, step, src, Be, Bs, do_cfg or pag, in_div, shallow=True)
            self._assemble(multi, heads, skips, tail, shallow=True)
        self._keep = (ts, step, mp, lat)
        return self

    # ---- the parts of `bind`, in its order
    def _blend_buffers(self, blend, latents_shape):
        """Loop-owned fp32 copies of `blend` at stable addresses (a captured graph reads them); first image / mask only."""
        if blend is None:
            return None
        _, Cl, h, w = latents_shape
        dev = self.unet.device
        x0, mk, nz = blend
        want = ((1, Cl, h, w), (1, 1, h, w), tuple(latents_shape))
        bufs = getattr(self, "_blend_bufs", None)
        if bufs is None or tuple(tuple(b.shape) for b in bufs) != want:
            bufs = self._blend_bufs = tuple(torch.zeros(sh, dtype=torch.float32, device=dev) for sh in want)
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
        if getattr(self, "_f_ts", None) is None or self._f_ts.shape != tsv.shape:
            self._f_ts = tsv
            self._f_step = torch.zeros(1, dtype=torch.int32, device=dev)
            self._f_x = torch.zeros(latents_shape, dtype=torch.float32, device=dev)
        else:
            self._f_ts.copy_(tsv)
        if tuple(self._f_x.shape) != tuple(latents_shape):
            self._f_x = torch.zeros(latents_shape, dtype=torch.float32, device=dev)
        self._do_cfg, self._g = bool(do_cfg), float(guidance_scale)
        return self._f_ts, self._f_step, self._f_x, None

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
            if fold_advance and (getattr(self, "_ticket", None) is None or self._ticket.device != lat.device):
                self._ticket = torch.zeros(1, dtype=torch.int32, device=lat.device)
            if self._noisy and (getattr(self, "_var_noise", None) is None or self._var_noise.shape != lat.shape):
                self._var_noise = torch.zeros_like(lat)
            noise = self._var_noise if self._noisy else lat      # (a step that reads no noise: any valid address)
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

    # ---- perturbed-attention guidance: the per-row scale table
    def _pag_table_for(self, rows: int, device) -> torch.Tensor:
        """fp32 [rows of the schedule] at a stable address (a captured graph reads it)."""
        t = getattr(self, "_pag_table", None)
        if t is None or t.numel() != rows or t.device != device:
            self._pag_table, self._pag_filled = torch.zeros(rows, dtype=torch.float32, device=device), None
        return self._pag_table

    def _fill_pag_table(self, ts):
        """s_i of every schedule row (pag.scale_rows) -> the device table, when the scale pair or the timesteps changed."""
        host = getattr(self.scheduler, "_ts_host", None) if not self.foreign else None
        tsl = [float(v) for v in (host if host is not None else ts).tolist()]
        want = (self._pag, tuple(tsl))
        if want != self._pag_filled:
            self._pag_rows = PAGM.scale_rows(self._pag[0], self._pag[1], tsl)
            self._pag_table.copy_(torch.tensor(self._pag_rows, dtype=torch.float32))
            self._pag_filled = want

    # ---- guidance_rescale: the one-float cell
    def _phi_cell_for(self, device) -> torch.Tensor:
        """fp32 [1] at a stable address (a captured graph reads it)."""
        c = getattr(self, "_phi_cell", None)
        if c is None or c.device != device:
            self._phi_cell, self._phi_filled = torch.zeros(1, dtype=torch.float32, device=device), None
        return self._phi_cell

    def _fill_phi_cell(self):
        """This call's guidance_rescale -> the device cell, when it changed."""
        if self._rescale != self._phi_filled:
            self._phi_cell.copy_(torch.tensor([self._rescale], dtype=torch.float32))
            self._phi_filled = self._rescale

    def _assemble(self, multi, heads, skips, tail, shallow: bool = False):
        """`self.program`: every head, every network's plan without the launches its head replaces, the tail.  Several
        ControlNets: the parts are kept, and one program per set of active nets is assembled on demand (`_set_entry`).
        shallow (DeepCache): the same assembly over the runtimes' shallow plans -> `self.program_shallow`."""
        rts = self.side_rts + [self.rt]
        if multi and shallow:
            self._parts_shallow = dict(heads=heads, skips=skips, tail=tail.calls)
            self.program_shallow = self._set_shallow(self._set_entry(tuple(range(len(self.side_rts)))))
            return
        if multi:
            self._multi, self._sets = multi, {}
            self._parts, self._parts_shallow = dict(heads=heads, skips=skips, tail=tail.calls), None
            self._guess_ramps = [self._guess_ramp] * len(self.side_rts)      # (same zero convs in every net: one ramp, per net)
            self.program = self._set_entry(tuple(range(len(self.side_rts))))["program"]    # (every net active: flops, tools)
            return
        if not shallow:
            self._multi, self._sets = multi, {}
        full = Plan()
        for r in rts:
            full.calls += heads[id(r)]
        for r in rts:
            plan = r.shallow_plan if shallow else r.step_plan
            full.calls += [c for i, c in enumerate(plan.calls) if i not in skips[id(r)]]
            full.flops += plan.flops_executed             # (a program's `flops`: what its launches execute)
        full.calls += tail.calls
        if shallow:
            self.program_shallow = full
        else:
            self.program = full

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
        tabs = self.__dict__.setdefault("_temb_tables", {})
        k = (id(r), int(ts.numel()), total)
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
        ts, step = self._keep[0], self._keep[1]
        for info in getattr(self, "_temb", {}).values():
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
        ramp = getattr(self, "_guess_ramp", None)
        return tuple(r * v for r in ramp) if ramp is not None else v

    def _scale_now(self):
        sc = getattr(self.side_rt, "_scale", None) if getattr(self, "side_rt", None) is not None else None
        return tuple(sc) if isinstance(sc, (list, tuple)) else sc

    # ---- several ControlNets: one program (and graph) per set of active nets
    def _set_entry(self, active):
        """The step program for the nets `active` (ascending indices): heads and plans of those nets only, the first one
        overwriting net 0's residual buffers, the others adding to them in place; no net -> one zeroing launch over the
        buffers (the UNet plan is never rebuilt).  keep_closed_nets: every net is in, the closed ones get scale 0."""
        active = tuple(active)
        ent = self._sets.get(active)
        if ent is not None:
            return ent
        P, rts = self._parts, self.side_rts
        included = list(range(len(rts))) if self.keep_closed_nets else list(active)
        prog = Plan()
        for k in included:
            prog.calls += P["heads"][id(rts[k])]
        prog.calls += P["heads"][id(self.rt)]
        records = {}
        for n, k in enumerate(included):
            calls, records[k] = rts[k].chained_step_calls(rts[0], accumulate=n > 0, scale=0.0,
                                                         skip=P["skips"][id(rts[k])])
            prog.calls += calls
            prog.flops += rts[k].step_plan.flops_executed
        if not included:
            prog.add("zero_u64", self.lib.pp_zero_u64, *rts[0].residual_block())
        prog.calls += [c for i, c in enumerate(self.rt.step_plan.calls) if i not in P["skips"][id(self.rt)]]
        prog.flops += self.rt.step_plan.flops_executed
        prog.calls += P["tail"]
        ent = self._sets[active] = dict(active=active, included=included, program=prog, records=records, graph=None,
                                        scales=None, program_shallow=None, records_shallow={}, graph_shallow=None)
        return ent

    def _set_shallow(self, ent):
        """DeepCache: the set's program over the shallow plans (the same assembly; the zero convs of the live positions)."""
        if ent["program_shallow"] is not None:
            return ent["program_shallow"]
        P, rts = self._parts_shallow, self.side_rts
        prog = Plan()
        for k in ent["included"]:
            prog.calls += P["heads"][id(rts[k])]
        prog.calls += P["heads"][id(self.rt)]
        for n, k in enumerate(ent["included"]):
            calls, ent["records_shallow"][k] = rts[k].chained_step_calls(rts[0], accumulate=n > 0, scale=0.0,
                                                                         skip=P["skips"][id(rts[k])], shallow=True)
            prog.calls += calls
            prog.flops += rts[k].shallow_plan.flops_executed
        if not ent["included"]:
            prog.add("zero_u64", self.lib.pp_zero_u64, *rts[0].residual_block())
        prog.calls += [c for i, c in enumerate(self.rt.shallow_plan.calls) if i not in P["skips"][id(self.rt)]]
        prog.flops += self.rt.shallow_plan.flops_executed
        prog.calls += P["tail"]
        ent["program_shallow"], ent["scales"] = prog, None      # (the scales are written again, into both programs' records)
        return prog

    def _set_scales(self, ent, scales):
        """Write this call's per-net scales into the set's zero-conv launch records (by-value kernel arguments: a graph
        captured with other values is dropped).  Within a call every scale of a set is constant."""
        want = tuple(float(scales[k]) if k in ent["active"] else 0.0 for k in ent["included"])
        if want == ent["scales"]:
            return
        for k, v in zip(ent["included"], want):
            ramp = self._guess_ramps[k]
            vals = [r * v for r in ramp] if ramp is not None else [v] * len(ent["records"][k])
            for rec, x in zip(ent["records"][k], vals):
                rec.scale = float(x)
            if k in ent["records_shallow"]:
                pos = self.side_rts[k].shallow_plan.zero_conv_pos
                for rec, p_ in zip(ent["records_shallow"][k], pos):
                    rec.scale = float(vals[p_])
        ent["scales"], ent["graph"], ent["graph_shallow"] = want, None, None

    def _multi_schedule(self, scale_schedule, num_steps):
        """Per step: the set's entry, its scales written and (use_graph) its graph captured -- all before the first step."""
        n = len(self.side_rts)
        if scale_schedule is None:
            raise L.PPError("several ControlNets need a per-step schedule of per-net scales")
        rows = [[float(v) for v in row] for row in scale_schedule[:num_steps]]
        if len(rows) < num_steps or any(len(r) != n for r in rows):
            raise L.PPError(f"scale_schedule must hold {num_steps} rows of {n} per-net scales")
        ents = []
        for row in rows:
            ent = self._set_entry(tuple(k for k, v in enumerate(row) if v != 0.0))
            ents.append((ent, row))
        seen = {}
        for ent, row in ents:
            act = tuple(row[k] for k in ent["active"])
            if seen.setdefault(ent["active"], act) != act:
                raise L.PPError("the scale of an active ControlNet changed inside one call")
        if self._deep() and len(seen) > 1:
            raise L.PPError("DeepCache with several ControlNets whose set of active nets changes during the call (guidance "
                            "windows) is not implemented: one set per call, or DeepCacheSDHelper.disable()")
        if self._deep():
            for ent, _ in ents:
                self._set_shallow(ent)
        return ents

    # ---- DeepCache: which program an evaluation runs
    def _deep(self) -> bool:
        return getattr(self, "rt", None) is not None and getattr(self.rt, "shallow_plan", None) is not None and \
            getattr(self.rt.net, "deepcache", None) is not None

    def shallow_rows(self, num_steps: int) -> List[bool]:
        """Per evaluation of a call (one per row of the schedule `run` steps through, counted from 0 at every call): does it
        run the shallow program?  Evaluation e is full iff e % cache_interval == 0; without DeepCache every one is."""
        if not self._deep():
            return [False] * num_steps
        iv = int(self.rt.net.deepcache.interval)
        return [e % iv != 0 for e in range(num_steps)]

    def capture(self):
        """Capture one step into a hipGraph (torch.cuda.CUDAGraph).  The captured launches read the step counter from
        device memory, so the same graph serves every step."""
        self._graph_scale = self._scale_now()
        self._graph_ip = self.rt.ip_scales()          # (IP-Adapter scales: by-value arguments of the UNet's launches as well)
        self.graph = self._capture_program(self.program)
        self.graph_shallow = None             # (captured with the same by-value arguments, so it goes with the full one)

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

    def _schedule(self, scale_schedule, num_steps):
        """The prologue `run` and `_run_foreign` share -> (ents, scale_schedule, varying).  Several ControlNets: per step
        the set's entry with this call's scales written, no scalar schedule.  Else the schedule as one scale per step (a
        wrapper around one net hands rows of one scale) and whether it varies inside the call."""
        ents = None
        if self._multi:
            ents = self._multi_schedule(scale_schedule, num_steps)
            for ent, row in ents:
                self._set_scales(ent, row)
            scale_schedule = None
        elif scale_schedule is not None:
            scale_schedule = [s[0] if isinstance(s, (list, tuple)) else s for s in scale_schedule]
        return ents, scale_schedule, scale_schedule is not None and len(set(scale_schedule)) > 1

    def run(self, latents: torch.Tensor, num_steps: int, use_graph: bool = True,
            callback: Optional[Callable] = None, timesteps=None, scale_schedule: Optional[List[float]] = None):
        """Runs `num_steps` steps starting from step counter 0.  Returns the fp32 latents tensor (owned by the loop)."""
        if self.foreign:
            return self._run_foreign(latents, num_steps, use_graph, callback, timesteps, scale_schedule)
        self.scheduler.reset()
        if getattr(self, "_ticket", None) is not None:
            self._ticket.zero_()       # (an aborted launch must not leave the step counter's ticket mid-count)
        if self._keep[2] is not None:
            self._keep[2].zero_()
        self._fill_temb_tables()
        if self._pag is not None:
            self._fill_pag_table(self._keep[0])
        if self._rescale is not None:
            self._fill_phi_cell()
        self.latents.copy_(latents.to(self.latents.device, torch.float32))
        ents, scale_schedule, varying = self._schedule(scale_schedule, num_steps)
        shallow = self.shallow_rows(num_steps)
        if ents is not None and use_graph:        # (every set's graph before the first step)
            for (ent, _), sh in zip(ents, shallow):
                if ent["graph"] is None:          # (the full program first: its warm-up leaves a c the shallow one's can read)
                    ent["graph"] = self._capture_program(ent["program"])
                if sh and ent["graph_shallow"] is None:
                    ent["graph_shallow"] = self._capture_program(ent["program_shallow"])
        if not varying and scale_schedule and self.side_rt is not None and \
                self._scale_now() != self._side_scale(scale_schedule[0]):
            self.side_rt._patch_scale(self._side_scale(scale_schedule[0]))   # (a previous call may have left a windowed value)
        if use_graph and not varying and (self.graph is None or self._graph_scale != self._scale_now() or
                                          getattr(self, "_graph_ip", ()) != self.rt.ip_scales()):
            self.capture()
        if use_graph and not varying and ents is None and any(shallow) and self.graph_shallow is None:
            self.graph_shallow = self._capture_program(self.program_shallow)
        stream = torch.cuda.current_stream().cuda_stream
        for i in range(num_steps):
            if varying and self.side_rt is not None:
                self.side_rt._patch_scale(self._side_scale(scale_schedule[i]))
            # this row's noise, by the scheduler's own rule (stream-ordered before the step that consumes it)
            z = self.scheduler.noise_for(self.scheduler.begin_index + i, self.latents.shape, self._gen, self.latents.device,
                                         self._noise_dtype)
            if z is not None:
                self._var_noise.copy_(z)
            sfx = "_shallow" if shallow[i] else ""
            if ents is not None:
                if use_graph:
                    ents[i][0]["graph" + sfx].replay()
                else:
                    ents[i][0]["program" + sfx].run(stream)
            elif use_graph and not varying:
                (self.graph_shallow if shallow[i] else self.graph).replay()
            else:
                (self.program_shallow if shallow[i] else self.program).run(stream)
            if callback is not None:
                callback(i, timesteps[i] if timesteps is not None else None, self.latents)
        self._check_faults()
        return self.latents

    def _check_faults(self, blocking: bool = False):
        """Where a plan combines split-K in-kernel (launches of 2 / 4 co-resident splits: pp_gemm_combine_ctr_bytes()): the
        plan's fault word is examined WITHOUT a synchronisation -- copied to pinned memory behind this call's work, read by a
        later call (NetRuntime.check_faults).  `flush_faults()` is the blocking form for a caller that synchronises anyway."""
        for r in [getattr(self, "rt", None)] + list(getattr(self, "side_rts", [])):
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
        ents, scale_schedule, varying = self._schedule(scale_schedule, num_steps)
        shallow = self.shallow_rows(num_steps)
        stream = torch.cuda.current_stream().cuda_stream
        for i in range(num_steps):
            t = tl[i]
            sfx = "_shallow" if shallow[i] else ""
            x = sch.scale_model_input(lat, t) if hasattr(sch, "scale_model_input") else lat
            self._f_x.copy_(x)
            if varying and self.side_rt is not None:
                self.side_rt._patch_scale(self._side_scale(scale_schedule[i]))
            if ents is not None:
                ent = ents[i][0]
                if use_graph:
                    if ent["graph" + sfx] is None:
                        ent["graph" + sfx] = self._capture_program(ent["program" + sfx])
                        self._f_step.fill_(i)
                    ent["graph" + sfx].replay()
                else:
                    ent["program" + sfx].run(stream)
            elif use_graph and not varying:
                if self.graph is None or self._graph_scale != self._scale_now() or \
                        getattr(self, "_graph_ip", ()) != self.rt.ip_scales():
                    self.capture()
                    self._f_step.fill_(i)
                if shallow[i] and self.graph_shallow is None:
                    self.graph_shallow = self._capture_program(self.program_shallow)
                    self._f_step.fill_(i)
                (self.graph_shallow if shallow[i] else self.graph).replay()
            else:
                (self.program_shallow if shallow[i] else self.program).run(stream)
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
