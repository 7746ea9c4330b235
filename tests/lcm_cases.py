"""Shared by tests/test_lcm.py, tests/test_lcm_gpu.py and tests/golden/make_ref_lcm.py: diffusers-0.27 `LCMScheduler`
restated in plain torch from its published form (arXiv:2310.04378 + the library's step), independently of the product's
coefficient tables.  Works on CPU tensors and on device tensors with a CPU generator (the noise is drawn on the generator's
device, as `randn_tensor` does).  TEST INFRASTRUCTURE: nothing here is imported by the product."""
from types import SimpleNamespace

import numpy as np
import torch


class LCMScheduler:
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, original_inference_steps=50,
                 timestep_scaling=10.0, steps_offset=0, generator=None):
        """`generator`: the scheduler's own source of noise for callers that hand none to `step` (oracle.loops.loop_v2).
        `steps_offset` is kept in `config` and has no effect, as in the library."""
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      original_inference_steps=original_inference_steps, timestep_scaling=timestep_scaling,
                                      steps_offset=steps_offset, prediction_type="epsilon")
        self.betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0)
        self.sigma_data = 0.5
        self.generator = generator
        self.timesteps = None
        self.num_inference_steps = None
        self.draws = 0

    def scale_model_input(self, sample, timestep=None):
        return sample

    def set_timesteps(self, num_inference_steps=None, device=None, original_inference_steps=None, timesteps=None,
                      strength=1.0):
        T = self.config.num_train_timesteps
        original_steps = original_inference_steps or self.config.original_inference_steps
        if original_steps > T:
            raise ValueError("original_steps > num_train_timesteps")
        k = T // original_steps
        origin = np.asarray(list(range(1, int(original_steps * strength) + 1))) * k - 1
        if timesteps is not None:
            n = len(timesteps)
            ts = np.array(timesteps, dtype=np.int64)
            ts = ts[max(n - min(int(n * strength), n), 0):]
        else:
            if num_inference_steps > T or num_inference_steps > original_steps or len(origin) // num_inference_steps < 1:
                raise ValueError("num_inference_steps does not fit the schedule")
            origin = origin[::-1].copy()
            idx = np.floor(np.linspace(0, len(origin), num=num_inference_steps, endpoint=False)).astype(np.int64)
            ts = origin[idx]
        self.num_inference_steps = len(ts)
        self.timesteps = torch.from_numpy(ts.copy()).long()
        self.draws = 0

    def scalings(self, timestep):
        s = timestep * self.config.timestep_scaling
        c_skip = self.sigma_data ** 2 / (s ** 2 + self.sigma_data ** 2)
        c_out = s / (s ** 2 + self.sigma_data ** 2) ** 0.5
        return c_skip, c_out

    def step(self, model_output, timestep, sample, generator=None, return_dict=False, noise=None):
        """`noise`: use this tensor instead of drawing (the audits that replay a step on recorded inputs)."""
        t = torch.as_tensor(timestep).cpu().long()
        i = int((self.timesteps == t).nonzero()[0])
        prev_t = self.timesteps[i + 1] if i + 1 < len(self.timesteps) else t
        a_t = self.alphas_cumprod[t].to(sample.device)
        a_p = (self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod).to(sample.device)
        c_skip, c_out = self.scalings(t.to(sample.device))
        x0 = (sample - (1 - a_t).sqrt() * model_output) / a_t.sqrt()
        den = c_out * x0 + c_skip * sample
        if i != self.num_inference_steps - 1:
            if noise is None:
                g = generator if generator is not None else self.generator
                gdev = g.device if g is not None else model_output.device
                noise = torch.randn(model_output.shape, generator=g, device=gdev, dtype=den.dtype).to(model_output.device)
                self.draws += 1
            prev = a_p.sqrt() * den + (1 - a_p).sqrt() * noise
        else:
            prev = den
        return (prev, den) if not return_dict else SimpleNamespace(prev_sample=prev, denoised=den)

    def add_noise(self, original_samples, noise, timesteps):
        a = self.alphas_cumprod.to(original_samples.device)[timesteps.to(original_samples.device).long()]
        sa, s1 = (a ** 0.5).flatten(), ((1 - a) ** 0.5).flatten()
        while sa.dim() < original_samples.dim():
            sa, s1 = sa.unsqueeze(-1), s1.unsqueeze(-1)
        return sa.to(original_samples.dtype) * original_samples + s1.to(original_samples.dtype) * noise


def alphas_cumprod_f64(T=1000, beta_start=0.00085, beta_end=0.012):
    """The library's fp32 betas / cumulative product (its own state), widened: the float64 forms start from the same table."""
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0).double().numpy()


def row_f64(t, prev_t, last, timestep_scaling=10.0, ac=None):
    """The eight table entries of one step in float64: sqrt(1-a_t), sqrt(a_t), c_out, c_skip, sqrt(a_prev), sqrt(1-a_prev), 0, 0."""
    ac = alphas_cumprod_f64() if ac is None else ac
    s = float(t) * timestep_scaling
    c_skip, c_out = 0.25 / (s * s + 0.25), s / np.sqrt(s * s + 0.25)
    a_t = ac[t]
    tail = (1.0, 0.0) if last else (np.sqrt(ac[prev_t]), np.sqrt(1.0 - ac[prev_t]))
    return np.array([np.sqrt(1.0 - a_t), np.sqrt(a_t), c_out, c_skip, tail[0], tail[1], 0.0, 0.0])


def step_f64(x, e, z, t, prev_t, last, timestep_scaling=10.0, ac=None):
    """One LCM step in float64 on numpy arrays; `z` is not touched on the last step."""
    c = row_f64(t, prev_t, last, timestep_scaling, ac)
    x0 = (x - c[0] * e) / c[1]
    den = c[2] * x0 + c[3] * x
    return den if last else c[4] * den + c[5] * z
