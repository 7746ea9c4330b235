"""Schedulers of the hot path with the diffusers duck-type the reference pipelines rely on
(/root/reference/powerpaint/pipelines/pipeline_PowerPaint.py:536-551,906,993,1023,642;
 pipeline_PowerPaint_Brushnet_CA.py:87-128,1391,1449,969): `.set_timesteps`, `.timesteps`, `.order`,
`.init_noise_sigma`, `.scale_model_input`, `.step(..., return_dict=False)[0]`, `.add_noise`, `.config.steps_offset`.

The arithmetic restates the diffusers==0.27.0 classes of the same names (pinned at
/root/reference/requirements/requirements.txt:3, not vendored).  Per-step coefficients are computed on the host in
fp32 torch exactly in the library's operation order and uploaded as a device table `coef[row][8 or 16]`; the tensor math
(CFG combine + step) runs in one fused HIP kernel per family, on fp32 latents:

    family (base class)          classes                                 step kernel             state_slots   scales_input
    _SchedulerBase               DDIM, DPM-Solver++ 2M, PNDM, UniPC      pp_cfg_sched_step       0, 1, 5, 4    no
    LCMScheduler                 LCM                                     pp_cfg_lcm_step         0             no
    _SigmaScheduler              Euler, Euler a                          pp_cfg_sigma_step       0             yes
    _KSampler                    Heun, DPM2, DPM2 a, LMS                 pp_cfg_ksampler_step    4             yes

Each family spells its kernel's argument list out once, in `step_launch`; `_SchedulerBase.step` and the fused loop
(pipelines/_loop.py) both launch what it returns, and both take the step's noise from `noise_for`.  So a foreign loop calling
`scheduler.step` runs the same kernel on the same row as the fused loop.  `kind` is the `kind` argument of
`pp_cfg_sched_step` (0..3); on the other classes it is a tag no kernel takes.  The sigma-space families (and
`use_karras_sigmas`) have latents x0 + sigma eps, `init_noise_sigma` > 1, a real `scale_model_input` and float timesteps.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib as L


def _betas(T, beta_start, beta_end):
    return torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float32) ** 2


# Options of the diffusers schedulers that change the arithmetic and that the fused step kernel does not implement: a
# config carrying another value is REFUSED (a silently dropped key would run and give wrong images).
_ONLY = {"prediction_type": ("epsilon",), "beta_schedule": ("scaled_linear",), "clip_sample": (False,),
         "thresholding": (False,), "rescale_betas_zero_snr": (False,), "use_karras_sigmas": (False,),
         "use_lu_lambdas": (False,), "euler_at_final": (False,), "variance_type": (None,),
         "trained_betas": (None,), "algorithm_type": ("dpmsolver++",), "solver_type": ("midpoint", "bh2"),
         "final_sigmas_type": ("zero",), "lower_order_final": (True,), "lambda_min_clipped": (-float("inf"),),
         "timestep_spacing": ("leading", "linspace", "trailing"), "interpolation_type": ("linear",),
         "timestep_type": ("discrete",), "sigma_min": (None,), "sigma_max": (None,)}


def variance_noise(shape, generator, device, dtype) -> torch.Tensor:
    """diffusers' `randn_tensor` for the per-step DDIM variance noise: drawn on the generator's device (a CPU generator
    gives the same numbers whatever the compute device), returned as contiguous fp32 on `device`."""
    gdev = generator.device if isinstance(generator, torch.Generator) else torch.device(device)
    if isinstance(generator, (list, tuple)):
        z = torch.cat([torch.randn((1,) + tuple(shape[1:]), generator=g, device=g.device, dtype=dtype).to(device)
                       for g in generator])
    else:
        z = torch.randn(tuple(shape), generator=generator, device=gdev, dtype=dtype).to(device)
    return z.to(torch.float32).contiguous()


def _check_config(cls_name, cfg, keys=None, allow=()):
    """`keys`: restrict the check to the options the target class's diffusers constructor names (a donor config's other
    keys never reach it in `from_config`).  `allow`: options this class implements at every value (`use_karras_sigmas` of
    DPM-Solver++ and the Euler classes)."""
    for k, ok in _ONLY.items():
        if (keys is not None and k not in keys) or k in allow:
            continue
        if k in cfg and cfg[k] not in ok:
            raise L.PPError(f"{cls_name}: {k}={cfg[k]!r} is not implemented on the HIP path (supported: {ok})")


def karras_sigmas(sigma_min, sigma_max, n, rho=7.0):
    """Karras et al. (arXiv:2206.00364, eq. 5) as the library's `_convert_to_karras` evaluates it, float64: n noise levels
    from sigma_max down to sigma_min, uniform in sigma^(1/rho)."""
    ramp = np.linspace(0, 1, n)
    lo, hi = float(sigma_min) ** (1 / rho), float(sigma_max) ** (1 / rho)
    return (hi + ramp * (lo - hi)) ** rho


def sigma_to_t(sigma, log_sigmas):
    """The library's `_sigma_to_t`: the (fractional) training timestep whose log sigma, linearly interpolated over the
    table, equals log `sigma`."""
    log_sigma = np.log(np.maximum(sigma, 1e-10))
    dists = log_sigma - log_sigmas[:, np.newaxis]
    low_idx = np.cumsum((dists >= 0), axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
    high_idx = low_idx + 1
    low, high = log_sigmas[low_idx], log_sigmas[high_idx]
    w = np.clip((low - log_sigma) / (low - high), 0, 1)
    return ((1 - w) * low_idx + w * high_idx).reshape(np.shape(sigma))


class _SchedulerBase:
    order = 1
    init_noise_sigma = 1.0
    kind = -1                # the `kind` argument of pp_cfg_sched_step (0..3); elsewhere a tag no kernel takes
    _ALLOWED = ()            # options of `_ONLY` this class implements at every value
    state_slots = 0          # fp32 copies of the latents the step kernel keeps between steps (DPM: 1, PNDM: 5): `m_prev`
    scales_input = False     # the networks' input is scaled per table row, at the head of the step (`in_div_table`)
    takes_eta = False        # this class's step takes `eta` (DDIM)
    discards_draw = False    # the library's step draws noise it does not use (plain Euler): `discard_draw`
    blend_refused = None     # why the known-region blend of a 4-channel UNet is not implemented for this class, if it is not
    _step_fields = {}        # what `step(return_dict=True)` returns next to `prev_sample`

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, **cfg):
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start,
                                      beta_end=beta_end, **cfg)
        self.betas = _betas(num_train_timesteps, beta_start, beta_end)
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, dim=0)
        self.timesteps = None
        self.num_inference_steps = None
        self._coef_dev = None
        self._ts_dev = None
        self._step_dev = None
        self._m_prev = None
        self._device = None
        self._begin = 0
        self._dup_calls = {}

    def set_begin_index(self, begin_index: int = 0):
        """diffusers' `set_begin_index`: the loop enters the schedule at row `begin_index` (`strength < 1`: the pipelines'
        `get_timesteps` hands `scheduler.timesteps[t_start:]` to the loop, pipeline_PowerPaint.py:713-720).  The
        multistep warm-up restarts there -- first-order first step of DPM-Solver++, PLMS start-up, UniPC order ramp and
        no corrector on the first step -- exactly what the library's step-index / counter logic does when the first
        `step()` call carries a later timestep.  `set_timesteps` resets it to 0."""
        if self.timesteps is None:
            raise L.PPError("set_begin_index before set_timesteps")
        if not 0 <= int(begin_index) < len(self._ts_host):
            raise ValueError(f"begin_index {begin_index} outside the schedule of {len(self._ts_host)} entries")
        self._begin = int(begin_index)
        self._fill_table()
        self.timesteps = self._ts_host.clone()
        self._upload(self._device)

    @property
    def begin_index(self):
        return self._begin

    @classmethod
    def from_config(cls, config, **kw):
        """`Scheduler.from_config(other.config)` / a `scheduler_config.json` dict: the keys this class's constructor
        names are taken over, the rest (other schedulers' options, `_class_name`, ...) ignored."""
        import inspect
        src = dict(config) if isinstance(config, dict) else dict(vars(config))
        src.update(kw)
        _check_config(cls.__name__, src, allow=cls._ALLOWED)
        names = set(inspect.signature(cls.__init__).parameters) - {"self", "kw", "cfg"}
        return cls(**{k: v for k, v in src.items() if k in names})

    # -- device state for the fused kernel
    def scale_model_input(self, sample, timestep=None):
        return sample

    def _upload(self, device):
        self._device = torch.device(device) if device is not None else None
        if self._device is not None and self._device.type == "cuda":
            same = (self._coef_dev is not None and self._coef_dev.shape == self._coef.shape
                    and self._coef_dev.device.type == "cuda"
                    and (self._device.index is None or self._coef_dev.device.index == self._device.index))
            if same:   # keep device addresses stable across calls so captured graphs stay valid
                self._coef_dev.copy_(self._coef)
                self._ts_dev.copy_(self.timesteps.to(torch.float32))
                self._step_dev.fill_(self._begin)
            else:
                self._coef_dev = self._coef.to(self._device).contiguous()
                self._ts_dev = self.timesteps.to(self._device, torch.float32).contiguous()
                self._step_dev = torch.full((1,), self._begin, dtype=torch.int32, device=self._device)
            self.timesteps = self.timesteps.to(self._device)
        if self._m_prev is not None:
            self._m_prev.zero_()
        self._dup_calls = {}

    def coef_table(self) -> torch.Tensor:
        return self._coef_dev

    def timesteps_f32(self) -> torch.Tensor:
        return self._ts_dev

    def step_counter(self) -> torch.Tensor:
        return self._step_dev

    def renoise_table(self) -> torch.Tensor:
        """[rows][2] fp32 on the scheduler's device, indexed by the step counter like the coefficient table: what
        `add_noise(x0, noise, timesteps[i + 1])` multiplies x0 and the noise by AFTER step i -- (sqrt(abar), sqrt(1-abar))
        of the next timestep, (1, 0) after the last one.  The ppt-v1 loop with a 4-channel UNet re-noises the known
        region with it every step (pipeline_PowerPaint.py:1025-1039; pp_latent_blend)."""
        tab = self._renoise_rows()
        dev = self._device if self._device is not None else "cpu"
        cur = getattr(self, "_renoise_dev", None)
        want = torch.device(dev)
        if cur is not None and cur.shape == tab.shape and cur.device.type == want.type and \
                (want.index is None or cur.device.index == want.index):
            cur.copy_(tab)            # (stable address: a captured step graph reads it)
        else:
            self._renoise_dev = tab.to(dev).contiguous()
        return self._renoise_dev

    def _renoise_rows(self) -> torch.Tensor:
        ts = self._ts_host.long()
        a = self.alphas_cumprod[ts[1:]].to(torch.float32)
        return torch.stack([torch.cat([a ** 0.5, torch.ones(1)]), torch.cat([(1 - a) ** 0.5, torch.zeros(1)])], 1)

    def m_prev(self, like: torch.Tensor) -> torch.Tensor:
        """The step kernel's state (`state_slots` > 0): one slot has the latents' shape, several are stacked in front."""
        shape = (self.state_slots,) + tuple(like.shape) if self.state_slots > 1 else tuple(like.shape)
        if self._m_prev is None or tuple(self._m_prev.shape) != shape or self._m_prev.device != like.device:
            self._m_prev = torch.zeros(shape, dtype=torch.float32, device=like.device)
        return self._m_prev

    def reset(self):
        if self._step_dev is not None:
            self._step_dev.fill_(self._begin)
        if self._m_prev is not None:
            self._m_prev.zero_()
        self._dup_calls = {}

    def _index_of(self, timestep) -> int:
        """Row of `timestep`.  A timestep the schedule holds more than once (PLMS repeats its second entry, rounded Karras
        timesteps can coincide) is disambiguated by call order: a foreign loop calls step() once per entry."""
        t = float(timestep) if self._ts_host.is_floating_point() else int(timestep)
        idx = (self._ts_host == t).nonzero().flatten().tolist()
        if not idx:
            raise ValueError(f"timestep {t} is not in the schedule")
        if len(idx) == 1:
            return idx[0]
        calls = self._dup_calls.get(t, 0)
        self._dup_calls[t] = calls + 1
        return idx[min(calls, len(idx) - 1)]

    def set_eta(self, eta: float = 0.0):
        """`eta` of the pipelines (pipeline_PowerPaint.py:736-745): only DDIM's step takes it, the other schedulers
        ignore it -- as `prepare_extra_step_kwargs` never hands it to them."""
        return self

    # -- per-step host noise (the loop draws it before the step that consumes it, into a buffer at a stable address)
    @property
    def step_noise(self) -> bool:
        """Does this scheduler's step, as configured now, consume Gaussian noise drawn by the host?  (stochastic DDIM:
        eta > 0; LCM: always).  Part of the loop's program key."""
        return False

    def draws_noise_at(self, row: int) -> bool:
        """Does the step at table row `row` draw noise?  (LCM: every row but the last of the full schedule.)"""
        return self.step_noise

    def noise_for(self, row: int, shape, generator, device, dtype):
        """THE noise rule, of `step` and of the fused loop alike: the Gaussian noise the step at table row `row` consumes,
        drawn like diffusers' `randn_tensor(shape, generator=generator, ...)` -- or None where it consumes none, after
        advancing `generator` by the draw the library makes and does not use (`discards_draw`).  The caller's generator
        ends where the library leaves it."""
        if self.step_noise and self.draws_noise_at(row):
            return variance_noise(shape, generator, device, dtype)
        if self.discards_draw:
            self.discard_draw(shape, generator, dtype)
        return None

    @staticmethod
    def discard_draw(shape, generator, dtype):
        """Advance `generator` by one `randn_tensor(shape)` without keeping or uploading the numbers.  (No generator: the
        library would use the global RNG, which nothing here has to stay in step with.)"""
        gens = generator if isinstance(generator, (list, tuple)) else [generator]
        sh = tuple(shape) if len(gens) == 1 else (1,) + tuple(shape[1:])
        for g in gens:
            if isinstance(g, torch.Generator):
                torch.randn(sh, generator=g, device=g.device, dtype=dtype)

    def step_launch(self, eps, cfg, guidance, lat, state, noise, n, step, ticket):
        """This family's step launch as `Plan.add` takes it, `(name, fn, *args)`: the one place that spells the entry point's
        argument list out.  Raw pointers and integers: eps (the CFG pair when `cfg`), the fp32 latents updated in place, the
        state (`m_prev`) or None, the noise (a row that adds none never reads it: any valid address), `n` elements, the device
        step counter indexing the scheduler's own table, the ticket through which the last block moves it on, or None."""
        return ("cfg_sched_step", L.lib().pp_cfg_sched_step, eps, cfg, guidance, lat, state, n, self.kind,
                self._coef_dev.data_ptr(), step, ticket)

    def step(self, model_output, timestep, sample, eta: float = 0.0, generator=None, return_dict: bool = True, **kw):
        """One table row, x_t -> x_{t-1}, in the family's HIP kernel (fp32 math).  Returns a NEW tensor in sample's dtype;
        the state between the calls (`state_slots`) lives in the scheduler, zeroed by `set_timesteps` / `set_begin_index`.
        `generator`: the step's noise (`noise_for`).  `eta`: stochastic DDIM only (`takes_eta`)."""
        if not sample.is_cuda:
            raise L.PPError("scheduler.step needs CUDA tensors: the step runs in the HIP kernel, no CPU fallback")
        if self.takes_eta and float(eta) != self.eta:
            self.set_eta(eta)
        i = self._index_of(timestep)
        x = sample.detach().to(torch.float32).contiguous().clone()
        e = model_output.detach().to(torch.float32).contiguous()
        step = torch.full((1,), i, dtype=torch.int32, device=x.device)
        z = self.noise_for(i, model_output.shape, generator, x.device, model_output.dtype)
        noise = (x if z is None else z).data_ptr()
        launches = [self.step_launch(e.data_ptr(), 0, 0.0, x.data_ptr(), self.m_prev(x).data_ptr() if self.state_slots else None,
                                     noise, x.numel(), step.data_ptr(), None)]
        if self.takes_eta and self.eta > 0:
            launches.append(self.variance_launch(x.data_ptr(), noise, x.numel(), step.data_ptr()))
        for name, fn, *args in launches:
            L.check(fn(*args, torch.cuda.current_stream().cuda_stream), "pp_" + name)
        out = x.to(sample.dtype)
        return SimpleNamespace(prev_sample=out, **self._step_fields) if return_dict else (out,)

    def add_noise(self, original_samples, noise, timesteps):
        a = self.alphas_cumprod.to(original_samples.device)[timesteps.to(original_samples.device).long()]
        sa = (a ** 0.5).flatten().to(original_samples.dtype)
        s1 = ((1 - a) ** 0.5).flatten().to(original_samples.dtype)
        while sa.dim() < original_samples.dim():
            sa, s1 = sa.unsqueeze(-1), s1.unsqueeze(-1)
        return sa * original_samples + s1 * noise


class DDIMScheduler(_SchedulerBase):
    """epsilon prediction, `leading` spacing, steps_offset = 1, set_alpha_to_one = False, no clipping; eta in [0, 1]."""
    kind = 0
    takes_eta = True

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1,
                 set_alpha_to_one=False, timestep_spacing="leading", **kw):
        _check_config("DDIMScheduler", kw)
        if timestep_spacing != "leading":
            raise L.PPError(f"DDIMScheduler: timestep_spacing={timestep_spacing!r} is not implemented (leading only)")
        super().__init__(num_train_timesteps, beta_start, beta_end, steps_offset=steps_offset,
                         set_alpha_to_one=set_alpha_to_one, timestep_spacing="leading", prediction_type="epsilon")
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.eta = 0.0

    def set_eta(self, eta: float = 0.0):
        """Stochastic DDIM: std_dev_t = eta * sqrt(variance_t) enters the table (columns 3 and 4); the device table is
        rewritten in place, so a captured step graph picks the new values up."""
        if not 0.0 <= float(eta) <= 1.0:
            raise ValueError(f"eta must be in [0, 1], got {eta}")
        if float(eta) == self.eta and self.timesteps is not None:
            return self               # (the table set_timesteps / set_begin_index filled already carries this eta)
        self.eta = float(eta)
        if self.timesteps is not None:
            self._fill_table()
            self.timesteps = self._ts_host.clone()
            begin = self._begin
            self._upload(self._device)
            self._begin = begin
        return self

    @property
    def step_noise(self) -> bool:
        return self.eta > 0

    def variance_launch(self, lat, noise, n, step):
        """eta > 0: `latents += std_dev_t * z`, the launch behind the step launch (same form as `step_launch`)."""
        return ("ddim_variance_noise", L.lib().pp_ddim_variance_noise, lat, noise, n, self._coef_dev.data_ptr(), step)

    def set_timesteps(self, num_inference_steps: int, device=None):
        T = self.config.num_train_timesteps
        self.num_inference_steps = num_inference_steps
        ratio = T // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64) + self.config.steps_offset
        self._ts_host = torch.from_numpy(ts)
        self.timesteps = self._ts_host.clone()
        self._begin = 0
        self._fill_table()
        self._upload(device)

    def _fill_table(self):
        """(rows do not depend on where the loop enters: DDIM keeps no history)"""
        ts, n = self._ts_host.numpy(), self.num_inference_steps
        ratio = self.config.num_train_timesteps // n
        coef = torch.zeros(n, 8, dtype=torch.float32)
        for i, t in enumerate(ts.tolist()):
            prev = t - ratio
            a_t = self.alphas_cumprod[t]
            a_p = self.alphas_cumprod[prev] if prev >= 0 else self.final_alpha_cumprod
            coef[i, 0] = (1 - a_t) ** 0.5
            coef[i, 1] = a_t ** 0.5
            coef[i, 2] = a_p ** 0.5
            # DDIMScheduler.step: variance = (1-a_prev)/(1-a_t) * (1-a_t/a_prev); std_dev_t = eta * sqrt(variance);
            # direction coefficient sqrt(1-a_prev-std_dev_t^2); prev_sample += std_dev_t * noise (pp_ddim_variance_noise)
            sd = self.eta * (((1 - a_p) / (1 - a_t)) * (1 - a_t / a_p)) ** 0.5
            coef[i, 3] = (1 - a_p - sd ** 2) ** 0.5
            coef[i, 4] = sd
        self._coef = coef


def dpm_timesteps(T, n, spacing="linspace", steps_offset=0):
    """DPMSolverMultistepScheduler.set_timesteps of diffusers 0.27 (lambda_min_clipped = -inf => last_timestep = T):
    what `DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)` yields on an SD-1.5 checkpoint is the
    `leading` form with steps_offset 1, the class default is `linspace`."""
    if spacing == "linspace":
        return np.linspace(0, T - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
    if spacing == "leading":
        return (np.arange(0, n + 1) * (T // (n + 1))).round()[::-1][:-1].copy().astype(np.int64) + steps_offset
    if spacing == "trailing":
        return np.arange(T, 0, -T / n).round().copy().astype(np.int64) - 1
    raise ValueError(f"unknown timestep_spacing {spacing}")


class DPMSolverMultistepScheduler(_SchedulerBase):
    """dpmsolver++ (2M), midpoint, `linspace` spacing, final_sigmas_type = "zero", lower_order_final.
    use_karras_sigmas ("DPM++ 2M Karras"): the noise levels are Karras et al.'s rho = 7 ramp between the ends of the full
    training table and the timesteps are their rounded `sigma_to_t` (the spacing options then have no effect, as in the
    library); only the host table changes."""
    kind = 1
    state_slots = 1
    _ALLOWED = ("use_karras_sigmas",)

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, solver_order=2,
                 timestep_spacing="linspace", steps_offset=0, use_karras_sigmas=False, **kw):
        _check_config("DPMSolverMultistepScheduler", kw)
        super().__init__(num_train_timesteps, beta_start, beta_end, solver_order=solver_order, steps_offset=steps_offset,
                         algorithm_type="dpmsolver++", solver_type="midpoint", final_sigmas_type="zero",
                         timestep_spacing=timestep_spacing, prediction_type="epsilon",
                         use_karras_sigmas=bool(use_karras_sigmas))
        if solver_order != 2:
            raise NotImplementedError("only the 2M solver is on the hot path")
        if timestep_spacing not in ("linspace", "leading", "trailing"):
            raise ValueError(f"unknown timestep_spacing {timestep_spacing}")

    @staticmethod
    def _alpha_sigma(sigma):
        alpha_t = 1 / ((sigma ** 2 + 1) ** 0.5)
        return alpha_t, sigma * alpha_t

    def set_timesteps(self, num_inference_steps: int, device=None):
        T = self.config.num_train_timesteps
        self.num_inference_steps = num_inference_steps
        ts = dpm_timesteps(T, num_inference_steps, self.config.timestep_spacing, self.config.steps_offset)
        sig = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
        if self.config.use_karras_sigmas:
            log_sig = np.log(sig)
            sig = karras_sigmas(sig[0], sig[-1], num_inference_steps)
            ts = np.array([sigma_to_t(v, log_sig) for v in sig]).round().astype(np.int64)
        else:
            sig = np.interp(ts, np.arange(0, len(sig)), sig)
        self.sigmas = torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32))
        self._ts_host = torch.from_numpy(ts)
        self.timesteps = self._ts_host.clone()
        self._begin = 0
        self._fill_table()
        self._upload(device)

    def _fill_table(self):
        n = self.num_inference_steps
        coef = torch.zeros(n, 8, dtype=torch.float32)
        for i in range(self._begin, n):
            a_cur, s_cur = self._alpha_sigma(self.sigmas[i])
            a_t, sg_t = self._alpha_sigma(self.sigmas[i + 1])
            lam_t = torch.log(a_t) - torch.log(sg_t)
            lam_s0 = torch.log(a_cur) - torch.log(s_cur)
            h = lam_t - lam_s0
            c3 = a_t * (torch.exp(-h) - 1.0)
            coef[i, 0], coef[i, 1] = s_cur, a_cur
            coef[i, 2] = sg_t / s_cur
            coef[i, 3] = c3
            first_order = (i == self._begin) or (i == n - 1)   # lower_order_nums < 1, lower_order_final (sigma_last = 0)
            if not first_order:
                a_s1, sg_s1 = self._alpha_sigma(self.sigmas[i - 1])
                lam_s1 = torch.log(a_s1) - torch.log(sg_s1)
                r0 = (lam_s0 - lam_s1) / h
                coef[i, 4] = 0.5 * c3
                coef[i, 5] = 1.0 / r0
        self._coef = coef


class PNDMScheduler(_SchedulerBase):
    """`PNDMScheduler(skip_prk_steps=True)` = PLMS with the SD-1.5 checkpoint config (`leading` spacing, steps_offset = 1,
    set_alpha_to_one = False, epsilon prediction): what the reference's v1 app runs when no scheduler is chosen.
    N inference steps are N + 1 entries in `.timesteps` (the second one repeats): the pipelines loop over
    `scheduler.timesteps`, so nothing else changes.  Host side: one table row per evaluation (linear-multistep weights,
    transfer coefficients, history ring slots); the tensor math runs in `pp_cfg_sched_step` (kind 2)."""
    kind = 2
    state_slots = 5

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1,
                 set_alpha_to_one=False, skip_prk_steps=True, timestep_spacing="leading", **kw):
        _check_config("PNDMScheduler", kw)
        if timestep_spacing != "leading":
            raise L.PPError(f"PNDMScheduler: timestep_spacing={timestep_spacing!r} is not implemented (leading only)")
        if not skip_prk_steps:
            raise NotImplementedError("only the PLMS form (skip_prk_steps=True, the SD-1.5 config) is on the hot path")
        super().__init__(num_train_timesteps, beta_start, beta_end, steps_offset=steps_offset,
                         set_alpha_to_one=set_alpha_to_one, skip_prk_steps=True, timestep_spacing="leading",
                         prediction_type="epsilon")
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]

    def _transfer(self, t, prev_t):
        a_t = self.alphas_cumprod[t]
        a_p = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        b_t, b_p = 1 - a_t, 1 - a_p
        sample_coeff = (a_p / a_t) ** 0.5
        denom = a_t * b_p ** 0.5 + (a_t * b_t * a_p) ** 0.5
        return float(sample_coeff), float(-(a_p - a_t) / denom)

    def set_timesteps(self, num_inference_steps: int, device=None):
        T = self.config.num_train_timesteps
        self.num_inference_steps = num_inference_steps
        ratio = T // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round().astype(np.int64) + self.config.steps_offset
        plms = np.concatenate([ts[:-1], ts[-2:-1], ts[-1:]])[::-1].copy()
        self._ts_host = torch.from_numpy(plms)
        self.timesteps = self._ts_host.clone()
        self._begin = 0
        self._fill_table()
        self._upload(device)

    def _fill_table(self):
        """One row per evaluation, keyed on the evaluation COUNT since the loop entered the schedule (the library's
        `counter`): entered late (`set_begin_index`), the second call is still treated as the repeat evaluation."""
        plms = self._ts_host.numpy()
        ratio = self.config.num_train_timesteps // self.num_inference_steps
        rows = len(plms)
        coef = torch.zeros(rows, 16, dtype=torch.float32)
        n_hist, head = 0, 0                       # stored predictions so far, ring slot of the next push
        for k, t in enumerate(plms.tolist()[self._begin:]):
            r = self._begin + k
            slot = lambda back: float((head - back) % 4)          # noqa: E731  (slot of the prediction `back` pushes ago)
            if k == 1:
                # second evaluation at the repeated timestep: redo the first transfer from the saved sample with the
                # average of the two predictions; this prediction is not stored
                a, b = self._transfer(t + ratio, t)
                coef[r, :6] = torch.tensor([0.5, 0.5, 0.0, 0.0, a, b])
                coef[r, 6:9] = torch.tensor([slot(1), slot(1), slot(1)])
                coef[r, 9], coef[r, 10], coef[r, 11] = -1.0, 1.0, 0.0
                continue
            n_hist = min(n_hist + 1, 4)
            w = {1: (1.0, 0.0, 0.0, 0.0), 2: (1.5, -0.5, 0.0, 0.0), 3: (23 / 12, -16 / 12, 5 / 12, 0.0),
                 4: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}[n_hist]
            a, b = self._transfer(t, t - ratio)
            coef[r, :6] = torch.tensor([w[0], w[1], w[2], w[3], a, b])
            coef[r, 6:9] = torch.tensor([slot(1), slot(2), slot(3)])      # h1, h2, h3 = previous pushes
            coef[r, 9] = float(head)                                      # this prediction goes to ring slot `head`
            coef[r, 10], coef[r, 11] = 0.0, (1.0 if k == 0 else 0.0)      # the first evaluation saves its input sample
            head = (head + 1) % 4
        self._coef = coef


class UniPCMultistepScheduler(_SchedulerBase):
    """UniPC (arXiv:2302.04867) as diffusers' `UniPCMultistepScheduler` runs it -- the scheduler app.py:197 installs on
    the ppt-v2 pipeline: predict_x0, solver_type "bh2", solver_order 2 (3 supported), lower_order_final, corrector on
    every step after the first (minus `disable_corrector`).

    Every step is linear in (sample, eps, last_sample, m1, m2, m3): the host solves the small UniPC systems per step
    in float64 and uploads one 16-float row; `pp_cfg_sched_step` (kind 3) evaluates
        x0 = (x - c0 eps) / c1
        xc = use_corr ? c3 last + c4 m1 + c5 m2 + c6 m3 + c7 x0 : x          (UniC on the previous transition)
        x' = c8 xc + c9 x0 + c10 m1 + c11 m2                                  (UniP to the next time step)
        (last, m1, m2, m3) <- (xc, x0, m1, m2)
    on the state [4][n] kept between steps."""
    kind = 3
    state_slots = 4

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, solver_order=2,
                 solver_type="bh2", lower_order_final=True, disable_corrector=(), timestep_spacing="linspace",
                 steps_offset=0, predict_x0=True, prediction_type="epsilon", **kw):
        super().__init__(num_train_timesteps, beta_start, beta_end, solver_order=solver_order, solver_type=solver_type,
                         lower_order_final=lower_order_final, disable_corrector=list(disable_corrector),
                         timestep_spacing=timestep_spacing, steps_offset=steps_offset, predict_x0=predict_x0,
                         prediction_type=prediction_type)
        _check_config("UniPCMultistepScheduler", dict(kw, prediction_type=prediction_type,
                                                      lower_order_final=lower_order_final), self._CHECKED)
        if solver_order not in (1, 2, 3) or solver_type not in ("bh1", "bh2") or not predict_x0 or \
                prediction_type != "epsilon":
            raise NotImplementedError("UniPC: solver_order 1-3, bh1 / bh2, predict_x0, epsilon prediction")

    # arithmetic options of diffusers-0.27 `UniPCMultistepScheduler.__init__` that the fused step does not implement (a
    # donor config's keys outside that constructor -- algorithm_type, euler_at_final, clip_sample ... -- never reach it;
    # `solver_type` has its own rule below)
    _CHECKED = ("prediction_type", "beta_schedule", "thresholding", "use_karras_sigmas", "trained_betas",
                "final_sigmas_type", "lower_order_final")

    @classmethod
    def from_config(cls, config, **kw):
        """`UniPCMultistepScheduler.from_config(pipe.scheduler.config)` (app.py:197): the keys this class shares with
        the donor scheduler's config are taken over (betas, timestep_spacing, steps_offset), the rest keep defaults."""
        src = dict(config) if isinstance(config, dict) else dict(vars(config))
        # refuse what would change the arithmetic (beta_schedule, thresholding, Karras sigmas, trained_betas,
        # final_sigmas_type ...) instead of dropping it: the donor's config is what app.py:197 hands over
        _check_config(cls.__name__, {**src, **kw}, cls._CHECKED)
        take = ("num_train_timesteps", "beta_start", "beta_end", "timestep_spacing", "steps_offset", "prediction_type",
                "lower_order_final")
        args = {k: src[k] for k in take if k in src}
        if src.get("solver_order") in (1, 2, 3):
            args["solver_order"] = src["solver_order"]
        # a donor's solver_type outside bh1 / bh2 (DPM-Solver's midpoint / heun, logrho) becomes bh2, as in diffusers
        if src.get("solver_type") in ("bh1", "bh2"):
            args["solver_type"] = src["solver_type"]
        args.update(kw)
        if args.get("solver_type") in ("midpoint", "heun", "logrho"):
            args["solver_type"] = "bh2"
        return cls(**args)

    def _grid(self, N):
        T, sp = self.config.num_train_timesteps, self.config.timestep_spacing
        if sp == "linspace":
            return np.linspace(0, T - 1, N + 1).round()[::-1][:-1].copy().astype(np.int64)
        if sp == "leading":
            return (np.arange(0, N + 1) * (T // (N + 1))).round()[::-1][:-1].copy().astype(np.int64) + \
                self.config.steps_offset
        if sp == "trailing":
            return (np.arange(T, 0, -T / N).round() - 1).astype(np.int64)
        raise ValueError(f"unknown timestep_spacing {sp}")

    def _system(self, order, rks, hh):
        """b / R of the UniPC conditions and h*phi_1, B(h); float64."""
        h_phi_1 = np.expm1(hh)
        h_phi_k = h_phi_1 / hh - 1.0
        B_h = hh if self.config.solver_type == "bh1" else np.expm1(hh)
        R, b, fact = [], [], 1.0
        for i in range(1, order + 1):
            R.append(rks ** (i - 1))
            b.append(h_phi_k * fact / B_h)
            fact *= i + 1
            h_phi_k = h_phi_k / hh - 1.0 / fact
        return np.stack(R), np.array(b), h_phi_1, B_h

    def set_timesteps(self, num_inference_steps: int, device=None):
        N = num_inference_steps
        self.num_inference_steps = N
        ts = self._grid(N)
        sig_all = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()      # fp32, as the library does
        sig = np.concatenate([np.interp(ts, np.arange(0, len(sig_all)), sig_all), [sig_all[0]]]).astype(np.float32)
        self.sigmas = torch.from_numpy(sig)
        sg = sig.astype(np.float64)                     # the library keeps the grid in fp32; coefficients from it in f64
        alpha = 1.0 / np.sqrt(sg ** 2 + 1.0)
        sigma = sg * alpha
        lam = np.log(alpha) - np.log(sigma)
        self._ts_host = torch.from_numpy(ts)
        self.timesteps = self._ts_host.clone()
        self._grid_f64 = (alpha, sigma, lam)
        self._begin = 0
        self._fill_table()
        self._upload(device)

    def _fill_table(self):
        alpha, sigma, lam = self._grid_f64
        N, b0 = self.num_inference_steps, self._begin
        K = self.config.solver_order
        coef = np.zeros((N, 16), dtype=np.float64)
        lower, prev_order = 0, 1
        for i in range(b0, N):
            c = coef[i]
            c[0], c[1] = sigma[i], alpha[i]
            # ---- UniC: re-estimate x_i from x_{i-1} (order = the order the previous predictor ran at); not on the step
            # the loop enters at (the library's `last_sample is None`).  `disable_corrector` lists step indices of the
            # full schedule, as the library's `step_index` does
            if i > b0 and (i - 1) not in self.config.disable_corrector:
                order = prev_order
                h = lam[i] - lam[i - 1]
                rks = np.array([(lam[i - (k + 1)] - lam[i - 1]) / h for k in range(1, order)] + [1.0])
                R, b, h_phi_1, B_h = self._system(order, rks, -h)
                rhos = np.array([0.5]) if order == 1 else np.linalg.solve(R, b)
                c[2] = 1.0
                c[3] = sigma[i] / sigma[i - 1]                                   # last_sample
                m0 = -alpha[i] * h_phi_1 + alpha[i] * B_h * rhos[-1]
                for k in range(1, order):                                         # D1s_k = (m_{-k} - m0) / rk_k
                    w = -alpha[i] * B_h * rhos[k - 1] / rks[k - 1]
                    c[4 + k] = w                                                  # m2 (k = 1), m3 (k = 2)
                    m0 -= w
                c[4] = m0                                                         # m1 = x0_{i-1}
                c[7] = -alpha[i] * B_h * rhos[-1]                                 # x0_i  (D1_t = x0_i - m0)
            # ---- UniP: x_{i+1} from the corrected x_i
            order = min(K, N - i) if self.config.lower_order_final else K
            order = min(order, lower + 1)
            h = lam[i + 1] - lam[i]
            rks = np.array([(lam[i - k] - lam[i]) / h for k in range(1, order)] + [1.0])
            R, b, h_phi_1, B_h = self._system(order, rks, -h)
            c[8] = sigma[i + 1] / sigma[i]
            m0 = -alpha[i + 1] * h_phi_1
            if order > 1:
                rhos = np.array([0.5]) if order == 2 else np.linalg.solve(R[:-1, :-1], b[:-1])
                for k in range(1, order):
                    w = -alpha[i + 1] * B_h * rhos[k - 1] / rks[k - 1]
                    c[9 + k] = w                                                  # m1 (k = 1), m2 (k = 2): older x0's
                    m0 -= w
            c[9] = m0                                                             # x0_i
            prev_order = order
            if lower < K:
                lower += 1
        self._coef = torch.from_numpy(coef.astype(np.float32))


class LCMScheduler(_SchedulerBase):
    """Latent consistency sampling (arXiv:2310.04378) as diffusers-0.27 `LCMScheduler` runs it: the sampler LCM-LoRA and
    LCM-distilled UNets are trained for, 1 to 8 network evaluations per image.  Epsilon prediction, scaled-linear betas, no
    clipping or thresholding.  `steps_offset`, `timestep_spacing` and `set_alpha_to_one` are kept in `config` and have no
    effect on the arithmetic, as in the library (its schedule never reaches a previous timestep below 0).

    One step (fp32):  x0 = (x - sqrt(1-a_t) e) / sqrt(a_t);  den = c_out x0 + c_skip x  with the boundary scalings at
    s = t * timestep_scaling, c_skip = 0.25 / (s^2 + 0.25), c_out = s / sqrt(s^2 + 0.25);  x' = sqrt(a_prev) den +
    sqrt(1-a_prev) z with fresh Gaussian z, a_prev at the NEXT entry of `timesteps` -- on the last step of the full schedule
    x' = den and nothing is drawn.  Table row = (sqrt(1-a_t), sqrt(a_t), c_out, c_skip, sqrt(a_prev), sqrt(1-a_prev), 0, 0),
    the last row with (1, 0) in columns 4 and 5; the tensor math runs in `pp_cfg_lcm_step`."""
    kind = 4
    _step_fields = {"denoised": None}

    # arithmetic options of diffusers-0.27 `LCMScheduler.__init__` that the fused step does not implement
    _CHECKED = ("prediction_type", "beta_schedule", "clip_sample", "thresholding", "rescale_betas_zero_snr", "trained_betas")

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, original_inference_steps=50,
                 set_alpha_to_one=True, steps_offset=0, timestep_spacing="leading", timestep_scaling=10.0, **kw):
        _check_config("LCMScheduler", kw, self._CHECKED)
        super().__init__(num_train_timesteps, beta_start, beta_end, original_inference_steps=original_inference_steps,
                         set_alpha_to_one=set_alpha_to_one, steps_offset=steps_offset, timestep_spacing=timestep_spacing,
                         timestep_scaling=timestep_scaling, prediction_type="epsilon", clip_sample=False)
        self.custom_timesteps = False

    @classmethod
    def from_config(cls, config, **kw):
        """`LCMScheduler.from_config(pipe.scheduler.config)`: the keys this class's constructor names are taken over; of the
        donor's other keys only those the library's LCM constructor names as well can change the arithmetic and are
        checked (a PNDM config's `skip_prk_steps`, a DPM config's `algorithm_type` ... never reach it)."""
        import inspect
        src = dict(config) if isinstance(config, dict) else dict(vars(config))
        src.update(kw)
        _check_config(cls.__name__, src, cls._CHECKED)
        names = set(inspect.signature(cls.__init__).parameters) - {"self", "kw"}
        return cls(**{k: v for k, v in src.items() if k in names or k in cls._CHECKED})

    step_noise = True        # (a constant in place of the base's property)

    def draws_noise_at(self, row: int) -> bool:
        return int(row) != len(self._ts_host) - 1

    def set_timesteps(self, num_inference_steps=None, device=None, original_inference_steps=None, timesteps=None,
                      strength: float = 1.0):
        T = self.config.num_train_timesteps
        if num_inference_steps is None and timesteps is None:
            raise ValueError("Must pass exactly one of `num_inference_steps` or `custom_timesteps`.")
        if num_inference_steps is not None and timesteps is not None:
            raise ValueError("Can only pass one of `num_inference_steps` or `custom_timesteps`.")
        original_steps = original_inference_steps if original_inference_steps is not None else \
            self.config.original_inference_steps
        if original_steps > T:
            raise ValueError(f"`original_steps`: {original_steps} cannot be larger than `num_train_timesteps`: {T}")
        k = T // original_steps
        origin = np.asarray(list(range(1, int(original_steps * strength) + 1)), dtype=np.int64) * k - 1
        if timesteps is not None:
            ts = [int(t) for t in timesteps]
            if any(float(a) != b for a, b in zip(timesteps, ts)):
                raise ValueError("`custom_timesteps` must be integers.")
            if len(ts) == 0 or any(b >= a for a, b in zip(ts, ts[1:])):
                raise ValueError("`custom_timesteps` must be in descending order.")
            if ts[0] >= T or ts[-1] < 0:
                raise ValueError(f"`timesteps` must start before `num_train_timesteps`: {T} and stay non-negative.")
            n = len(ts)
            ts = np.array(ts, dtype=np.int64)
            ts = ts[max(n - min(int(n * strength), n), 0) * self.order:]
            if len(ts) == 0:
                raise ValueError(f"strength {strength} leaves none of the {n} custom timesteps")
            self.custom_timesteps = True
        else:
            if num_inference_steps > T:
                raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than "
                                 f"`num_train_timesteps`: {T}")
            if num_inference_steps < 1:
                raise ValueError(f"`num_inference_steps`: {num_inference_steps} must be at least 1")
            if len(origin) // num_inference_steps < 1:
                raise ValueError(f"The combination of `original_steps x strength`: {original_steps} x {strength} is smaller"
                                 f" than `num_inference_steps`: {num_inference_steps}")
            if num_inference_steps > original_steps:
                raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than "
                                 f"`original_inference_steps`: {original_steps}")
            origin = origin[::-1].copy()
            idx = np.floor(np.linspace(0, len(origin), num=num_inference_steps, endpoint=False)).astype(np.int64)
            ts = origin[idx]
            self.custom_timesteps = False
        self.num_inference_steps = len(ts)
        self._ts_host = torch.from_numpy(np.ascontiguousarray(ts))
        self.timesteps = self._ts_host.clone()
        self._begin = 0
        self._fill_table()
        self._upload(device)

    def _fill_table(self):
        """(rows do not depend on where the loop enters: LCM keeps no history.  fp32 torch in the library's operation order.)"""
        ts = self._ts_host.tolist()
        n = len(ts)
        coef = torch.zeros(n, 8, dtype=torch.float32)
        for i, t in enumerate(ts):
            a_t = self.alphas_cumprod[t]
            s = torch.tensor(t) * self.config.timestep_scaling           # get_scalings_for_boundary_condition_discrete,
            c_skip = 0.5 ** 2 / (s ** 2 + 0.5 ** 2)                      # sigma_data = 0.5
            c_out = s / (s ** 2 + 0.5 ** 2) ** 0.5
            coef[i, 0], coef[i, 1] = (1 - a_t).sqrt(), a_t.sqrt()
            coef[i, 2], coef[i, 3] = c_out, c_skip
            if i < n - 1:
                a_p = self.alphas_cumprod[ts[i + 1]]
                coef[i, 4], coef[i, 5] = a_p.sqrt(), (1 - a_p).sqrt()
            else:
                coef[i, 4], coef[i, 5] = 1.0, 0.0                        # prev_sample = denoised, no noise drawn
        self._coef = coef

    def step_launch(self, eps, cfg, guidance, lat, state, noise, n, step, ticket):
        """Guidance combine, consistency transition, noise term and counter advance in one launch (no state)."""
        return ("cfg_lcm_step", L.lib().pp_cfg_lcm_step, eps, cfg, guidance, lat, noise, n, self._coef_dev.data_ptr(), step,
                ticket)

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True, **kw):
        """`_SchedulerBase.step` without `eta` in its signature, which `prepare_extra_step_kwargs` reads."""
        return super().step(model_output, timestep, sample, generator=generator, return_dict=return_dict)


class _SigmaScheduler(_SchedulerBase):
    """The sigma-space family (Karras et al., arXiv:2206.00364; k-diffusion `sample_euler` / `sample_euler_ancestral`) as
    diffusers 0.27 runs it on a variance-preserving checkpoint: the latents are x = x0 + sigma eps with
    sigma = sqrt((1 - abar) / abar), the network sees x / sqrt(sigma^2 + 1) (`scale_model_input`; in the fused loop
    pp_step_head_scaled with `in_div_table()`), and the initial noise is multiplied by `init_noise_sigma` > 1.

    Grid: fp32 timesteps per `timestep_spacing`, sigmas interpolated linearly over the training table, 0 appended.
    use_karras_sigmas: the rho = 7 ramp between the ends of that inference grid, timesteps = the fractional `sigma_to_t`.
    Table row = (sigma_i, dt, s_up, 0 ...), evaluated in fp32 torch in the library's operation order; the tensor math
    x' = x + dt e + s_up z runs in `pp_cfg_sigma_step`.  No state between steps."""
    scales_input = True
    _step_fields = {"pred_original_sample": None}
    _ALLOWED = ("use_karras_sigmas",)
    # arithmetic options of the library's constructors that the fused step does not implement at another value
    _CHECKED = ("prediction_type", "beta_schedule", "trained_betas", "rescale_betas_zero_snr", "interpolation_type",
                "timestep_type", "final_sigmas_type", "timestep_spacing", "sigma_min", "sigma_max")

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, timestep_spacing="linspace",
                 steps_offset=0, use_karras_sigmas=False, **kw):
        _check_config(type(self).__name__, dict(kw, timestep_spacing=timestep_spacing), self._CHECKED)
        super().__init__(num_train_timesteps, beta_start, beta_end, timestep_spacing=timestep_spacing,
                         steps_offset=steps_offset, use_karras_sigmas=bool(use_karras_sigmas), prediction_type="epsilon",
                         interpolation_type="linear", timestep_type="discrete", final_sigmas_type="zero")
        self._sig_all = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()        # fp32, as the library's
        self._in_div_dev = None

    @classmethod
    def from_config(cls, config, **kw):
        """`EulerAncestralDiscreteScheduler.from_config(pipe.scheduler.config)`: betas, `timestep_spacing` and `steps_offset`
        of the donor (an SD-1.5 checkpoint: `leading`, 1) are taken over; of its other keys only those the library's Euler
        constructors name as well can change the arithmetic and are checked."""
        import inspect
        src = dict(config) if isinstance(config, dict) else dict(vars(config))
        src.update(kw)
        _check_config(cls.__name__, src, cls._CHECKED)
        names = set(inspect.signature(cls.__init__).parameters) - {"self", "kw"}
        return cls(**{k: v for k, v in src.items() if k in names})

    @property
    def init_noise_sigma(self):
        """The library's property: the largest sigma of the current grid (of the training table before `set_timesteps`),
        sqrt(max^2 + 1) with `leading` spacing."""
        m = float(self.sigmas.max()) if self.timesteps is not None else float(self._sig_all.max())
        return m if self.config.timestep_spacing in ("linspace", "trailing") else (m ** 2 + 1) ** 0.5

    def _base_grid(self, n):
        """(timesteps [n], sigmas [n]) as numpy, before the 0 is appended: the grid every class of the family starts from."""
        T = self.config.num_train_timesteps
        sp = self.config.timestep_spacing
        if sp == "linspace":
            ts = np.linspace(0, T - 1, n, dtype=np.float32)[::-1].copy()
        elif sp == "leading":
            ts = (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.float32) + self.config.steps_offset
        else:
            ts = np.arange(T, 0, -T / n).round().copy().astype(np.float32) - 1
        sig = np.interp(ts, np.arange(0, len(self._sig_all)), self._sig_all)
        if self.config.use_karras_sigmas:
            log_sig = np.log(self._sig_all)
            sig = karras_sigmas(sig[-1], sig[0], n)
            ts = np.array([sigma_to_t(v, log_sig) for v in sig])
        return ts, sig

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        ts, sig = self._base_grid(num_inference_steps)
        self.sigmas = torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32))
        self._set_rows(ts)
        self.timesteps = self._ts_host.clone()
        self._begin = 0
        self._fill_table()
        self._upload(device)

    def _set_rows(self, ts):
        """`_ts_host`, one entry per table row, from the base grid's timesteps (the two-stage samplers interleave here)."""
        self._ts_host = torch.from_numpy(ts.astype(np.float32))

    def _sigma_up(self, s_from, s_to):
        return torch.zeros(())

    def _fill_table(self):
        """(rows do not depend on where the loop enters: no history)"""
        n = self.num_inference_steps
        coef = torch.zeros(n, 8, dtype=torch.float32)
        for i in range(n):
            s_from, s_to = self.sigmas[i], self.sigmas[i + 1]
            s_up = self._sigma_up(s_from, s_to)
            s_down = (s_to ** 2 - s_up ** 2) ** 0.5
            coef[i, 0], coef[i, 1], coef[i, 2] = s_from, s_down - s_from, s_up
        self._coef = coef
        self._set_row_sigmas(self.sigmas[:-1])

    def _set_row_sigmas(self, row_sigma):
        """The noise level each row's evaluation happens at -> `in_div_table`, `scale_model_input`, `add_noise`."""
        self._row_sigma = row_sigma.to(torch.float32).contiguous()
        self._in_div = (self._row_sigma ** 2 + 1) ** 0.5

    def _upload(self, device):
        super()._upload(device)
        if self._device is not None and self._device.type == "cuda":
            cur = self._in_div_dev
            if cur is not None and cur.shape == self._in_div.shape and cur.device == self._coef_dev.device:
                cur.copy_(self._in_div)            # (stable address: a captured step graph reads it)
            else:
                self._in_div_dev = self._in_div.to(self._coef_dev.device).contiguous()

    def in_div_table(self) -> torch.Tensor:
        """[rows] fp32 on the scheduler's device, indexed by the step counter: sqrt(sigma_i^2 + 1), what
        `scale_model_input` divides the latents by at step i (pp_step_head_scaled)."""
        return self._in_div_dev

    def scale_model_input(self, sample, timestep=None):
        i = self._peek_index(timestep)
        return sample / self._in_div[i].to(sample.device)          # (the divisor of the fused head launch, to the bit)

    def _peek_index(self, timestep) -> int:
        idx = (self._ts_host == float(timestep)).nonzero().flatten().tolist()
        if not idx:
            raise ValueError(f"timestep {float(timestep)} is not in the schedule")
        return idx[0]

    def _renoise_rows(self) -> torch.Tensor:
        """(1, sigma of row i + 1) after row i, (1, 0) after the last one: `add_noise(x0, noise, timesteps[i + 1])` in sigma
        space, in the layout pp_latent_blend reads."""
        nxt = torch.cat([self._row_sigma[1:], torch.zeros(1)])
        return torch.stack([torch.ones(len(self._ts_host)), nxt], 1).contiguous()

    def add_noise(self, original_samples, noise, timesteps):
        sig = self._row_sigma.to(device=original_samples.device, dtype=original_samples.dtype)
        s = sig[[self._peek_index(t) for t in timesteps.reshape(-1)]].flatten()
        while s.dim() < original_samples.dim():
            s = s.unsqueeze(-1)
        return original_samples + noise * s

    def draws_noise_at(self, row: int) -> bool:
        return True          # the library's step calls randn_tensor on every step, the last one included

    def step_launch(self, eps, cfg, guidance, lat, state, noise, n, step, ticket):
        """x' = x + dt e + s_up z (no state; plain Euler has s_up = 0 in every row and never reads the noise)."""
        return ("cfg_sigma_step", L.lib().pp_cfg_sigma_step, eps, cfg, guidance, lat, noise, n, self._coef_dev.data_ptr(), step,
                ticket)

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True, **kw):
        """`_SchedulerBase.step` without `eta` in its signature.  The Euler classes draw on every step, also where the noise is
        not used (plain Euler: `discards_draw`; the last ancestral step); DPM2 ancestral on every call, both stages."""
        return super().step(model_output, timestep, sample, generator=generator, return_dict=return_dict)


class EulerDiscreteScheduler(_SigmaScheduler):
    """diffusers-0.27 `EulerDiscreteScheduler` ("Euler", with use_karras_sigmas "Euler Karras") at s_churn = 0:
    x' = x + (sigma_{i+1} - sigma_i) e.  The library's step draws `randn_tensor` on every step even though gamma = 0 makes
    it unused; `discards_draw` tells the loop to advance the caller's generator the same way (host only, no upload)."""
    kind = 5
    discards_draw = True

    def step(self, model_output, timestep, sample, s_churn: float = 0.0, s_tmin: float = 0.0,
             s_tmax: float = float("inf"), s_noise: float = 1.0, generator=None, return_dict: bool = True, **kw):
        if float(s_churn) != 0.0:
            raise L.PPError(f"EulerDiscreteScheduler: s_churn={s_churn!r} is not implemented on the HIP path (0 only)")
        return super().step(model_output, timestep, sample, generator=generator, return_dict=return_dict)


class EulerAncestralDiscreteScheduler(_SigmaScheduler):
    """diffusers-0.27 `EulerAncestralDiscreteScheduler` ("Euler a"): s_up = sqrt(s_to^2 (s_from^2 - s_to^2) / s_from^2),
    s_down = sqrt(s_to^2 - s_up^2), x' = x + (s_down - s_from) e + s_up z with fresh Gaussian z on every step (on the last
    one s_up = 0 and the drawn z is not read)."""
    kind = 6

    step_noise = True        # (a constant in place of the base's property)

    def _sigma_up(self, s_from, s_to):
        return (s_to ** 2 * (s_from ** 2 - s_to ** 2) / s_from ** 2) ** 0.5


class _KSampler(_SigmaScheduler):
    """The sigma-space samplers that keep state between network evaluations (k-diffusion `sample_heun`, `sample_dpm_2`,
    `sample_dpm_2_ancestral`, `sample_lms` at s_churn = 0, as diffusers 0.27 schedules them).  One table row per
    evaluation, 16 floats laid out like the PLMS row:
        (c_e, c_h1, c_h2, c_h3, s_up, sigma of the evaluation, slot1, slot2, slot3, push_slot | -1, use_saved, save, 0...)
    evaluated in fp32 torch in the library's operation order; `pp_cfg_ksampler_step` computes
        x' = (use_saved ? saved : x) + c_e e + c_h1 H[slot1] + c_h2 H[slot2] + c_h3 H[slot3] + s_up z
    on the state [4][n] = three derivative slots and the saved sample.  State and table restart where the loop enters the
    schedule (`set_begin_index`).  The two-stage classes have `order = 2`: `timesteps` interleaves both evaluations of a
    step, 2N - 1 entries (the last step, to sigma = 0, is a single Euler row)."""
    state_slots = 4

    def _peek_index(self, timestep) -> int:
        """Row of the NEXT `step` call that carries `timestep`: of a repeated timestep (Heun's pairs; a DPM2 ancestral
        midpoint that lands on the next grid point) the occurrence after those `step` has consumed, counted from the row the
        loop entered at -- at an even begin index the first call carries the SECOND occurrence of its timestep."""
        t = float(timestep)
        idx = [i for i in (self._ts_host == t).nonzero().flatten().tolist() if i >= self._begin]
        if not idx:
            raise ValueError(f"timestep {t} is not in the schedule from row {self._begin} on")
        return idx[min(self._dup_calls.get(t, 0), len(idx) - 1)]

    def _index_of(self, timestep) -> int:
        i = self._peek_index(timestep)
        self._dup_calls[float(timestep)] = self._dup_calls.get(float(timestep), 0) + 1
        return i

    def draws_noise_at(self, row: int) -> bool:
        return self.step_noise   # DPM2 ancestral: the library's step draws on every call, both stages; the others never

    @staticmethod
    def _row(c_e, c_h=(0.0, 0.0, 0.0), s_up=0.0, sigma=0.0, slots=(0, 0, 0), push=-1, use_saved=False, save=False):
        r = torch.zeros(16, dtype=torch.float32)
        r[0], r[1], r[2], r[3], r[4], r[5] = c_e, c_h[0], c_h[1], c_h[2], s_up, sigma
        r[6], r[7], r[8], r[9] = float(slots[0]), float(slots[1]), float(slots[2]), float(push)
        r[10], r[11] = float(use_saved), float(save)
        return r

    def _two_stage_table(self, mid, down, up, heun=False):
        """Rows A_k (at sigma_k: save, step to `mid[k]`) and B_k (at `mid[k]`, from the saved sample) for k < N - 1, then the
        Euler row to 0.  Heun: B_k averages its derivative with A_k's (slot 0)."""
        sg, n = self.sigmas, self.num_inference_steps
        rows = []
        for k in range(n - 1):
            if heun:
                dt = sg[k + 1] - sg[k]
                rows.append(self._row(dt, sigma=sg[k], push=0, save=True))
                rows.append(self._row(dt / 2, (dt / 2, 0.0, 0.0), sigma=sg[k + 1], use_saved=True))
            else:
                rows.append(self._row(mid[k] - sg[k], sigma=sg[k], save=True))
                rows.append(self._row(down[k] - sg[k], s_up=up[k], sigma=mid[k], use_saved=True))
        # (entered at a B row -- an odd begin index, which no pipeline produces -- that row would read an empty state)
        rows.append(self._row(-sg[n - 1], sigma=sg[n - 1]))
        self._coef = torch.stack(rows)
        self._set_row_sigmas(self._coef[:, 5])

    def step_launch(self, eps, cfg, guidance, lat, state, noise, n, step, ticket):
        """One table row on the state [4][n] (s_up = 0 in every row of Heun, DPM2 and LMS: the noise is never read)."""
        return ("cfg_ksampler_step", L.lib().pp_cfg_ksampler_step, eps, cfg, guidance, lat, state, noise, n,
                self._coef_dev.data_ptr(), step, ticket)


class HeunDiscreteScheduler(_KSampler):
    """diffusers-0.27 `HeunDiscreteScheduler` ("Heun", with use_karras_sigmas "Heun Karras"; Karras et al. algorithm 1 at
    s_churn = 0): x~ = x + (s' - s) e(x, s), then x' = x + (s' - s) (e(x, s) + e(x~, s')) / 2; the last step is Euler.
    `timesteps` = [t_0, t_1, t_1, ..., t_{N-1}, t_{N-1}].  Nothing is drawn."""
    kind = 7
    order = 2

    def _set_rows(self, ts):
        t = torch.from_numpy(ts.astype(np.float32))
        self._ts_host = torch.cat([t[:1], t[1:].repeat_interleave(2)])

    def _fill_table(self):
        self._two_stage_table(None, None, None, heun=True)


class KDPM2DiscreteScheduler(_KSampler):
    """diffusers-0.27 `KDPM2DiscreteScheduler` ("DPM2", "DPM2 Karras"; DPM-Solver-2 as k-diffusion's `sample_dpm_2`):
    s_mid = exp((ln s + ln s') / 2), x~ = x + (s_mid - s) e(x, s), x' = x + (s' - s) e(x~, s_mid).  `timesteps` =
    [t_0, tau_0, t_1, tau_1, ..., t_{N-1}] with tau_k = sigma_to_t(s_mid,k), fractional.  Karras timesteps are rounded, as
    in the library's class.  Nothing is drawn."""
    kind = 8
    order = 2
    blend_refused = "the library's add_noise at a midpoint timestep is not pinned"

    def _base_grid(self, n):
        ts, sig = super()._base_grid(n)
        return (ts.round() if self.config.use_karras_sigmas else ts), sig

    def _split(self):
        """(mid, down, up) per step of the base grid, fp32 torch: plain DPM2 steps to sigma_{k+1} without noise."""
        sg = self.sigmas
        mid = sg.log().lerp(sg.roll(1).log(), 0.5).exp()[1:]      # mid[k]: between sigma_k and sigma_{k+1}
        return mid, sg[1:], torch.zeros_like(sg[1:])

    def _set_rows(self, ts):
        mid = self._split()[0].numpy()
        log_sig = np.log(self._sig_all)
        tau = np.array([sigma_to_t(v, log_sig) for v in mid[:-1]]).reshape(-1)
        t = torch.from_numpy(ts.astype(np.float32))
        tau = torch.from_numpy(tau.astype(np.float32))
        self._ts_host = torch.cat([t[:1], torch.stack((tau, t[1:]), dim=-1).flatten()])

    def _fill_table(self):
        self._two_stage_table(*self._split())


class KDPM2AncestralDiscreteScheduler(KDPM2DiscreteScheduler):
    """diffusers-0.27 `KDPM2AncestralDiscreteScheduler` ("DPM2 a", "DPM2 a Karras"; `sample_dpm_2_ancestral`): DPM2 towards
    s_down of the ancestral split (s_up as Euler ancestral's), s_mid between s and s_down, then + s_up z.  The library's
    step draws z on every call and uses it on the second stage only; the loop draws per row the same way, so the caller's
    generator ends where the library leaves it.  The last step has s_down = 0: Euler, no noise added."""
    kind = 9

    step_noise = True        # (a constant in place of the base's property)

    _sigma_up = EulerAncestralDiscreteScheduler._sigma_up

    def _split(self):
        sg = self.sigmas
        nxt = sg.roll(-1)
        nxt[-1] = 0.0
        up = self._sigma_up(sg, nxt)
        down = (nxt ** 2 - up ** 2) ** 0.5
        mid = sg.log().lerp(down.log(), 0.5).exp()
        mid[-2:] = 0.0
        return mid[:-1], down[:-1], up[:-1]


class LMSDiscreteScheduler(_KSampler):
    """diffusers-0.27 `LMSDiscreteScheduler` ("LMS", "LMS Karras"; k-diffusion `sample_lms`), order 4: x' = x + sum_j C_j e_{i-j}
    with C_j the integral over [sigma_i, sigma_{i+1}] of the Lagrange basis polynomial through sigma_i, sigma_{i-1}, ... of
    e_{i-j}'s node.  The library integrates numerically (`scipy.integrate.quad`, epsrel 1e-4); here the polynomial is
    integrated exactly in float64.  The order follows the ABSOLUTE step index, min(i + 1, 4), while the derivative list
    starts empty where the loop enters: entered late, the first rows use the leading coefficients of the higher-order basis
    (the library's `zip` truncation).  History = a ring over the 3 slots, each row pushing e into the slot of the oldest
    entry it read.  Nothing is drawn."""
    kind = 10
    order = 1
    lms_order = 4

    def lms_coefficient(self, order, i, j):
        P = np.polynomial.Polynomial
        sg = self.sigmas.numpy().astype(np.float64)
        prod = P([1.0])
        for k in range(order):
            if k != j:
                prod = prod * P([-sg[i - k], 1.0]) / (sg[i - j] - sg[i - k])
        integ = prod.integ()
        return float(integ(sg[i + 1]) - integ(sg[i]))

    def _fill_table(self):
        n, b0 = self.num_inference_steps, self._begin
        rows = [self._row(0.0) for _ in range(n)]
        for i in range(b0, n):
            r = i - b0                                            # evaluations since the loop entered
            order = min(i + 1, self.lms_order)
            have = min(r + 1, order)                              # derivatives in the list, this row's included
            c = [self.lms_coefficient(order, i, j) if j < have else 0.0 for j in range(4)]
            rows[i] = self._row(c[0], c[1:], sigma=self.sigmas[i], slots=[(r - j) % 3 for j in (1, 2, 3)], push=r % 3)
        self._coef = torch.stack(rows)
        self._set_row_sigmas(self.sigmas[:-1])

    def step(self, model_output, timestep, sample, order: int = 4, generator=None, return_dict: bool = True, **kw):
        if int(order) != self.lms_order:
            raise L.PPError(f"LMSDiscreteScheduler: step(order={order!r}) is not implemented on the HIP path (4 only)")
        return super().step(model_output, timestep, sample, generator=generator, return_dict=return_dict)


SCHEDULERS = {"DDIMScheduler": DDIMScheduler, "DPMSolverMultistepScheduler": DPMSolverMultistepScheduler,
              "PNDMScheduler": PNDMScheduler, "UniPCMultistepScheduler": UniPCMultistepScheduler,
              "LCMScheduler": LCMScheduler, "EulerAncestralDiscreteScheduler": EulerAncestralDiscreteScheduler,
              "HeunDiscreteScheduler": HeunDiscreteScheduler, "KDPM2DiscreteScheduler": KDPM2DiscreteScheduler,
              "KDPM2AncestralDiscreteScheduler": KDPM2AncestralDiscreteScheduler,
              "LMSDiscreteScheduler": LMSDiscreteScheduler}
