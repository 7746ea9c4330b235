"""The pin for the LCM restatement on a machine that has `diffusers` (it is not installed where the suite usually runs, so
this module skips there): tests/lcm_cases.LCMScheduler -- what the LCM tests and tests/golden/ref_lcm.pt are built on --
against `diffusers.LCMScheduler` on the same inputs.  CPU only, seconds."""
import os
import sys

import pytest
import torch

diffusers = pytest.importorskip("diffusers")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lcm_cases as LC  # noqa: E402


@pytest.mark.parametrize("kw", [dict(num_inference_steps=4), dict(num_inference_steps=8), dict(num_inference_steps=1),
                                dict(num_inference_steps=4, original_inference_steps=100),
                                dict(num_inference_steps=4, strength=0.5), dict(timesteps=[999, 600, 301, 7])])
def test_restated_lcm_scheduler_equals_the_library(kw):
    cfg = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000)
    lib, mine = diffusers.LCMScheduler(**cfg), LC.LCMScheduler()
    lib.set_timesteps(**kw)
    mine.set_timesteps(**kw)
    assert lib.timesteps.tolist() == mine.timesteps.tolist()
    assert lib.order == mine.order and float(lib.init_noise_sigma) == mine.init_noise_sigma
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, 8, 8, generator=g)
    assert torch.equal(lib.scale_model_input(x, lib.timesteps[0]), mine.scale_model_input(x, mine.timesteps[0]))
    noise = torch.randn(2, 4, 8, 8, generator=g)
    t0 = lib.timesteps[:1].repeat(2)
    assert torch.allclose(lib.add_noise(x, noise, t0), mine.add_noise(x, noise, t0), rtol=1e-6, atol=1e-6)
    ga, gb = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    xa = xb = x
    for t in lib.timesteps:
        e = torch.randn(2, 4, 8, 8, generator=g)
        xa = lib.step(e, t, xa, generator=ga, return_dict=False)[0]
        xb = mine.step(e, t, xb, generator=gb, return_dict=False)[0]
        assert torch.allclose(xa, xb, rtol=1e-5, atol=1e-5), (int(t), float((xa - xb).abs().max()))
    assert torch.equal(torch.randn(3, generator=ga), torch.randn(3, generator=gb))      # same number of draws


def test_timestep_scaling_reaches_the_boundary_terms():
    lib, mine = diffusers.LCMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                       timestep_scaling=0.001), LC.LCMScheduler(timestep_scaling=0.001)
    lib.set_timesteps(4)
    mine.set_timesteps(4)
    g = torch.Generator().manual_seed(1)
    x, e = torch.randn(1, 4, 8, 8, generator=g), torch.randn(1, 4, 8, 8, generator=g)
    t = lib.timesteps[-1]                                   # the last step: no noise, the boundary terms alone
    assert torch.allclose(lib.step(e, t, x, return_dict=False)[0], mine.step(e, t, x)[0], rtol=1e-5, atol=1e-5)
