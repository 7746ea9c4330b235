"""Shared by tests/test_sigma.py, tests/test_sigma_gpu.py, tests/test_diffusers_pin_sigma.py and
tests/golden/make_ref_sigma.py: diffusers-0.27 `EulerDiscreteScheduler` (s_churn = 0), `EulerAncestralDiscreteScheduler` and
the Karras noise levels (also of `DPMSolverMultistepScheduler`) restated in plain torch / numpy from their published form
(Karras et al., arXiv:2206.00364; k-diffusion `sample_euler`, `sample_euler_ancestral`, `get_sigmas_karras`),
independently of the product's coefficient tables.  Works on CPU tensors and on device tensors with a CPU generator (the
noise is drawn on the generator's device, as `randn_tensor` does).  TEST INFRASTRUCTURE: nothing here is imported by the
product."""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import schedulers as OS

RHO = 7.0


def train_sigmas(T=1000, beta_start=0.00085, beta_end=0.012):
    """sqrt((1 - abar) / abar) over the training timesteps, fp32 numpy as the library holds it."""
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float32) ** 2
    ac = torch.cumprod(1.0 - betas, dim=0)
    return (((1 - ac) / ac) ** 0.5).numpy()


def convert_to_karras(in_sigmas, n):
    """n levels from in_sigmas[0] (largest) to in_sigmas[-1], uniform in sigma^(1/rho); float64."""
    sigma_min, sigma_max = float(in_sigmas[-1]), float(in_sigmas[0])
    ramp = np.linspace(0, 1, n)
    min_inv_rho, max_inv_rho = sigma_min ** (1 / RHO), sigma_max ** (1 / RHO)
    return (max_inv_rho + ramp * (min_inv_rho - max_inv_rho)) ** RHO


def sigma_to_t(sigma, log_sigmas):
    """The fractional training timestep of a noise level: piecewise-linear interpolation in log sigma."""
    log_sigma = np.log(np.maximum(sigma, 1e-10))
    dists = log_sigma - log_sigmas[:, np.newaxis]
    low_idx = np.cumsum((dists >= 0), axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
    high_idx = low_idx + 1
    low, high = log_sigmas[low_idx], log_sigmas[high_idx]
    w = np.clip((low - log_sigma) / (low - high), 0, 1)
    return ((1 - w) * low_idx + w * high_idx).reshape(np.shape(sigma))


def spaced_timesteps(T, n, spacing, steps_offset):
    if spacing == "linspace":
        return np.linspace(0, T - 1, n, dtype=np.float32)[::-1].copy()
    if spacing == "leading":
        return (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.float32) + steps_offset
    if spacing == "trailing":
        return (np.arange(T, 0, -T / n)).round().copy().astype(np.float32) - 1
    raise ValueError(spacing)


class _Sigma:
    order = 1
    ancestral = False

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, timestep_spacing="linspace",
                 steps_offset=0, use_karras_sigmas=False, generator=None):
        """`generator`: the scheduler's own source of noise for callers that hand none to `step` (oracle.loops.loop_v2)."""
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      timestep_spacing=timestep_spacing, steps_offset=steps_offset,
                                      use_karras_sigmas=use_karras_sigmas, prediction_type="epsilon")
        self._train = train_sigmas(num_train_timesteps, beta_start, beta_end)
        self.sigmas = torch.from_numpy(np.concatenate([self._train[::-1], [0.0]]).astype(np.float32))
        self.generator = generator
        self.timesteps = None
        self.draws = 0

    @property
    def init_noise_sigma(self):
        m = self.sigmas.max()
        return m if self.config.timestep_spacing in ("linspace", "trailing") else (m ** 2 + 1) ** 0.5

    def set_timesteps(self, num_inference_steps, device=None):
        c = self.config
        ts = spaced_timesteps(c.num_train_timesteps, num_inference_steps, c.timestep_spacing, c.steps_offset)
        sig = np.interp(ts, np.arange(0, len(self._train)), self._train)
        if c.use_karras_sigmas:
            sig = convert_to_karras(sig, num_inference_steps)
            ts = np.array([sigma_to_t(s, np.log(self._train)) for s in sig])
        self.sigmas = torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(ts.astype(np.float32))
        self.num_inference_steps = num_inference_steps
        self.draws = 0

    def index_of(self, timestep):
        return int((self.timesteps == float(timestep)).nonzero()[0])

    def scale_model_input(self, sample, timestep):
        sigma = self.sigmas[self.index_of(timestep)].to(sample.device)
        return sample / ((sigma ** 2 + 1) ** 0.5)

    def _draw(self, model_output, generator, noise):
        if noise is not None:
            return noise
        g = generator if generator is not None else self.generator
        gdev = g.device if g is not None else model_output.device
        self.draws += 1
        return torch.randn(model_output.shape, generator=g, device=gdev, dtype=model_output.dtype).to(model_output.device)

    def step(self, model_output, timestep, sample, generator=None, return_dict=False, noise=None):
        """`noise`: use this tensor instead of drawing (the audits that replay a step on recorded inputs)."""
        i = self.index_of(timestep)
        sigma, sigma_to = self.sigmas[i].to(sample.device), self.sigmas[i + 1].to(sample.device)
        sample = sample.to(torch.float32)
        x0 = sample - sigma * model_output                        # epsilon prediction
        derivative = (sample - x0) / sigma
        if self.ancestral:
            sigma_up = (sigma_to ** 2 * (sigma ** 2 - sigma_to ** 2) / sigma ** 2) ** 0.5
            sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
            prev = sample + derivative * (sigma_down - sigma)
            prev = prev + self._draw(model_output, generator, noise) * sigma_up
        else:
            self._draw(model_output, generator, noise)            # gamma = 0: drawn by the library, never used
            prev = sample + derivative * (sigma_to - sigma)
        prev = prev.to(model_output.dtype)
        return (prev, x0) if not return_dict else SimpleNamespace(prev_sample=prev, pred_original_sample=x0)

    def add_noise(self, original_samples, noise, timesteps):
        sig = self.sigmas.to(device=original_samples.device, dtype=original_samples.dtype)
        s = sig[[self.index_of(t) for t in timesteps.reshape(-1)]].flatten()
        while s.dim() < original_samples.dim():
            s = s.unsqueeze(-1)
        return original_samples + noise * s


class EulerDiscreteScheduler(_Sigma):
    pass


class EulerAncestralDiscreteScheduler(_Sigma):
    ancestral = True


class DPMKarras(OS.DPMSolverMultistepScheduler):
    """The oracle's DPM-Solver++ 2M with the library's `use_karras_sigmas=True` grid: levels between the ends of the
    (flipped) training table, timesteps = rounded sigma_to_t; the spacing options have no effect."""

    def set_timesteps(self, num_inference_steps, device=None):
        super().set_timesteps(num_inference_steps)
        train = train_sigmas(self.config.num_train_timesteps)
        sig = convert_to_karras(np.flip(train).copy(), num_inference_steps)
        ts = np.array([sigma_to_t(s, np.log(train)) for s in sig]).round()
        self.sigmas = torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(ts).to(torch.int64)


# ------------------------------------------------------------------------------------------------ float64 forms
def row_f64(sigmas, i, ancestral):
    """(sigma_i, dt, s_up) of step i in float64 from the fp32 grid `sigmas` (the library's own state), widened."""
    s = np.asarray(sigmas, dtype=np.float64)
    s_from, s_to = s[i], s[i + 1]
    s_up = np.sqrt(s_to ** 2 * (s_from ** 2 - s_to ** 2) / s_from ** 2) if ancestral else 0.0
    s_down = np.sqrt(s_to ** 2 - s_up ** 2)
    return np.array([s_from, s_down - s_from, s_up])


def step_f64(x, eu, ec, z, g, dt, s_up):
    """One step in float64 on numpy arrays: e = eu + g (ec - eu) (ec None: e = eu), x' = x + dt e + s_up z; `z` is not
    touched where s_up == 0."""
    e = eu if ec is None else eu + g * (ec - eu)
    out = x + dt * e
    return out + s_up * z if s_up != 0 else out
