"""Shared by tests/test_ksamplers.py, tests/test_ksamplers_gpu.py, tests/test_diffusers_pin_ksamplers.py and
tests/golden/make_ref_ksamplers.py: diffusers-0.27 `HeunDiscreteScheduler`, `KDPM2DiscreteScheduler`,
`KDPM2AncestralDiscreteScheduler` and `LMSDiscreteScheduler` restated in plain torch / numpy from their published form (Karras
et al., arXiv:2206.00364; k-diffusion `sample_heun`, `sample_dpm_2`, `sample_dpm_2_ancestral`, `sample_lms` at s_churn = 0), the
way the library schedules them: interleaved sigma / timestep lists, a step index that the first `step` call finds from its
timestep, first-order / second-order state.  Independent of the product's coefficient tables: nothing here builds a row.
The LMS coefficients are `scipy.integrate.quad(..., epsrel=1e-4)` over the Lagrange basis, as the library computes them; the
module skips where scipy is absent.  Works on CPU tensors and on device tensors with a CPU generator.  TEST INFRASTRUCTURE:
nothing here is imported by the product."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

integrate = pytest.importorskip("scipy.integrate")

from sigma_cases import convert_to_karras, sigma_to_t, spaced_timesteps, train_sigmas  # noqa: E402


class _K:
    order = 2
    karras_round = False        # the two KDPM2 classes round their Karras timesteps

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

    # -- grid
    def _base(self, n):
        c = self.config
        ts = spaced_timesteps(c.num_train_timesteps, n, c.timestep_spacing, c.steps_offset)
        sig = np.interp(ts, np.arange(0, len(self._train)), self._train)
        if c.use_karras_sigmas:
            sig = convert_to_karras(sig, n)
            ts = np.array([sigma_to_t(s, np.log(self._train)) for s in sig])
            if self.karras_round:
                ts = ts.round()
        sig = torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32))
        return torch.from_numpy(ts.astype(np.float32)), sig

    def _t_of(self, sig):
        """(the library hands `_sigma_to_t` its fp32 tensor elements: the logarithm and the interpolation run in fp32)"""
        return torch.from_numpy(np.array([sigma_to_t(s.numpy(), np.log(self._train)) for s in sig]).reshape(-1).astype(np.float32))

    @staticmethod
    def _pairs(v):
        return torch.cat([v[:1], v[1:].repeat_interleave(2), v[-1:]])

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        self._build(*self._base(num_inference_steps))
        self.step_index = None
        self.begin_index = None
        self.sample = None
        self.draws = 0
        self._stepped = {}

    def set_begin_index(self, begin_index=0):
        self.begin_index = begin_index

    # -- index bookkeeping
    def index_for_timestep(self, timestep):
        """Before the first step: the SECOND of several matches (a schedule entered in the middle starts at a first stage);
        later: as many matches on as `step` has been called with this timestep."""
        idx = (self.timesteps == float(timestep)).nonzero().flatten().tolist()
        pos = (1 if len(idx) > 1 else 0) if not self._stepped else self._stepped.get(float(timestep), 0)
        return idx[min(pos, len(idx) - 1)]

    def _init_step_index(self, timestep):
        if self.step_index is None:
            self.step_index = self.begin_index if self.begin_index is not None else self.index_for_timestep(timestep)

    @property
    def state_in_first_order(self):
        return self.sample is None

    def _draw(self, model_output, generator):
        g = generator if generator is not None else self.generator
        gdev = g.device if g is not None else model_output.device
        self.draws += 1
        return torch.randn(model_output.shape, generator=g, device=gdev, dtype=model_output.dtype).to(model_output.device)

    def _eval_sigma(self):
        raise NotImplementedError

    def scale_model_input(self, sample, timestep):
        self._init_step_index(timestep)
        sigma = self._eval_sigma().to(sample.device)
        return sample / ((sigma ** 2 + 1) ** 0.5)

    def add_noise(self, original_samples, noise, timesteps):
        sig = self.sigmas.to(device=original_samples.device, dtype=original_samples.dtype)
        if self.begin_index is None:
            s = sig[[self.index_for_timestep(t) for t in timesteps.reshape(-1)]].flatten()
        else:
            s = sig[[self.begin_index] * timesteps.numel()].flatten()
        while s.dim() < original_samples.dim():
            s = s.unsqueeze(-1)
        return original_samples + noise * s

    def _done(self, timestep, prev, x0, model_output, return_dict):
        self._stepped[float(timestep)] = self._stepped.get(float(timestep), 0) + 1
        self.step_index += 1
        prev = prev.to(model_output.dtype)
        return (prev, x0) if not return_dict else SimpleNamespace(prev_sample=prev, pred_original_sample=x0)


class HeunDiscreteScheduler(_K):
    def _build(self, ts, sig):
        self.sigmas = torch.cat([sig[:1], sig[1:-1].repeat_interleave(2), sig[-1:]])
        self.timesteps = torch.cat([ts[:1], ts[1:].repeat_interleave(2)])
        self.prev_derivative = self.dt = None

    def _eval_sigma(self):
        return self.sigmas[self.step_index]

    def step(self, model_output, timestep, sample, generator=None, return_dict=False):
        self._init_step_index(timestep)
        i, dev = self.step_index, sample.device
        if self.state_in_first_order:
            sigma, sigma_next = self.sigmas[i].to(dev), self.sigmas[i + 1].to(dev)
            x0 = sample - sigma * model_output
            derivative = (sample - x0) / sigma
            dt = sigma_next - sigma
            self.prev_derivative, self.dt, self.sample = derivative, dt, sample
        else:
            sigma_next = self.sigmas[i].to(dev)
            x0 = sample - sigma_next * model_output
            derivative = (sample - x0) / sigma_next
            derivative = (self.prev_derivative + derivative) / 2
            dt, sample = self.dt, self.sample
            self.prev_derivative = self.dt = self.sample = None
        return self._done(timestep, sample + derivative * dt, x0, model_output, return_dict)


class KDPM2DiscreteScheduler(_K):
    karras_round = True

    def _build(self, ts, sig):
        interpol = sig.log().lerp(sig.roll(1).log(), 0.5).exp()
        self.sigmas = self._pairs(sig)
        self.sigmas_interpol = self._pairs(interpol)
        t_interpol = self._t_of(interpol)
        self.timesteps = torch.cat([ts[:1], torch.stack((t_interpol[1:-1, None], ts[1:, None]), dim=-1).flatten()])

    def _eval_sigma(self):
        return self.sigmas[self.step_index] if self.state_in_first_order else self.sigmas_interpol[self.step_index]

    def step(self, model_output, timestep, sample, generator=None, return_dict=False):
        self._init_step_index(timestep)
        i, dev = self.step_index, sample.device
        if self.state_in_first_order:
            sigma, sigma_interpol = self.sigmas[i].to(dev), self.sigmas_interpol[i + 1].to(dev)
            x0 = sample - sigma * model_output
            derivative = (sample - x0) / sigma
            dt = sigma_interpol - sigma
            self.sample = sample
        else:
            sigma, sigma_interpol, sigma_next = (self.sigmas[i - 1].to(dev), self.sigmas_interpol[i].to(dev),
                                                 self.sigmas[i].to(dev))
            x0 = sample - sigma_interpol * model_output
            derivative = (sample - x0) / sigma_interpol
            dt = sigma_next - sigma
            sample, self.sample = self.sample, None
        return self._done(timestep, sample + derivative * dt, x0, model_output, return_dict)


class KDPM2AncestralDiscreteScheduler(_K):
    karras_round = True

    def _build(self, ts, sig):
        nxt = sig.roll(-1)
        nxt[-1] = 0.0
        up = (nxt ** 2 * (sig ** 2 - nxt ** 2) / sig ** 2) ** 0.5
        down = (nxt ** 2 - up ** 2) ** 0.5
        down[-1] = 0.0
        interpol = sig.log().lerp(down.log(), 0.5).exp()
        interpol[-2:] = 0.0
        self.sigmas, self.sigmas_interpol = self._pairs(sig), self._pairs(interpol)
        self.sigmas_up, self.sigmas_down = self._pairs(up), self._pairs(down)
        t_interpol = self._t_of(interpol)
        self.timesteps = torch.cat([ts[:1], torch.stack((t_interpol[:-2, None], ts[1:, None]), dim=-1).flatten()])

    def _eval_sigma(self):
        return self.sigmas[self.step_index] if self.state_in_first_order else self.sigmas_interpol[self.step_index - 1]

    def step(self, model_output, timestep, sample, generator=None, return_dict=False):
        self._init_step_index(timestep)
        i, dev = self.step_index, sample.device
        noise = self._draw(model_output, generator)             # every call, both stages
        if self.state_in_first_order:
            sigma, sigma_interpol = self.sigmas[i].to(dev), self.sigmas_interpol[i].to(dev)
            x0 = sample - sigma * model_output
            derivative = (sample - x0) / sigma
            dt = sigma_interpol - sigma
            self.sample = sample
            prev = sample + derivative * dt
        else:
            sigma, sigma_interpol = self.sigmas[i - 1].to(dev), self.sigmas_interpol[i - 1].to(dev)
            sigma_up, sigma_down = self.sigmas_up[i - 1].to(dev), self.sigmas_down[i - 1].to(dev)
            x0 = sample - sigma_interpol * model_output
            derivative = (sample - x0) / sigma_interpol
            dt = sigma_down - sigma
            sample, self.sample = self.sample, None
            prev = sample + derivative * dt
            prev = prev + noise * sigma_up
        return self._done(timestep, prev, x0, model_output, return_dict)


class LMSDiscreteScheduler(_K):
    order = 1

    def _build(self, ts, sig):
        self.sigmas, self.timesteps = sig, ts
        self.derivatives = []

    def _eval_sigma(self):
        return self.sigmas[self.step_index]

    def get_lms_coefficient(self, order, t, current_order):
        def lms_derivative(tau):
            prod = 1.0
            for k in range(order):
                if current_order == k:
                    continue
                prod *= (tau - self.sigmas[t - k]) / (self.sigmas[t - current_order] - self.sigmas[t - k])
            return prod
        return integrate.quad(lms_derivative, self.sigmas[t], self.sigmas[t + 1], epsrel=1e-4)[0]

    def step(self, model_output, timestep, sample, order=4, generator=None, return_dict=False):
        self._init_step_index(timestep)
        i = self.step_index
        sigma = self.sigmas[i].to(sample.device)
        x0 = sample - sigma * model_output
        self.derivatives.append((sample - x0) / sigma)
        if len(self.derivatives) > order:
            self.derivatives.pop(0)
        order = min(i + 1, order)
        coeffs = [self.get_lms_coefficient(order, i, k) for k in range(order)]
        prev = sample + sum(c * d for c, d in zip(coeffs, reversed(self.derivatives)))
        return self._done(timestep, prev, x0, model_output, return_dict)


CLASSES = dict(HeunDiscreteScheduler=HeunDiscreteScheduler, KDPM2DiscreteScheduler=KDPM2DiscreteScheduler,
               KDPM2AncestralDiscreteScheduler=KDPM2AncestralDiscreteScheduler, LMSDiscreteScheduler=LMSDiscreteScheduler)


def eval_sigmas(sch):
    """The noise level of every evaluation of the schedule `sch` has set, by walking its step index the way a loop does."""
    out = []
    sch.step_index, sch.sample = 0, None
    for i in range(len(sch.timesteps)):
        sch.step_index = i
        sch.sample = None if (sch.order == 1 or i % 2 == 0) else 0
        out.append(float(sch._eval_sigma()))
    sch.step_index = sch.sample = None
    return out


# ------------------------------------------------------------------------------------------------ float64 row formula
def row_f64(x, saved, H, e, z, row):
    """The row formula of pp_cfg_ksampler_step in float64 on numpy arrays.  row = the 16 table floats.  Returns (x', saved',
    H') without touching its arguments; `z` is not looked at where s_up == 0."""
    c_e, c1, c2, c3, s_up = (float(v) for v in row[:5])
    s1, s2, s3, push = (int(v) for v in row[6:10])
    use_saved, save = row[10] != 0, row[11] != 0
    out = (saved if use_saved else x) + c_e * e + c1 * H[s1] + c2 * H[s2] + c3 * H[s3]
    if s_up != 0:
        out = out + s_up * z
    H2 = [h.copy() for h in H]
    if push >= 0:
        H2[push] = e.copy()
    return out, (x.copy() if save else saved.copy()), H2
