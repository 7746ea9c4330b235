"""Parity pin: the restated sigma-space schedulers of tests/sigma_cases.py against diffusers itself (0.27.0 is the version the
reference pins).  Skipped where diffusers is not installed -- tests/golden/README_sigma.md says "parity unpinned" until this
file has run somewhere."""
import inspect
import os
import sys

import pytest
import torch

diffusers = pytest.importorskip("diffusers")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sigma_cases as SC  # noqa: E402

SPACINGS = [dict(timestep_spacing="linspace"), dict(timestep_spacing="leading", steps_offset=1),
            dict(timestep_spacing="trailing")]
BASE = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


@pytest.mark.parametrize("karras", [False, True], ids=["plain", "karras"])
@pytest.mark.parametrize("opts", SPACINGS, ids=["linspace", "leading", "trailing"])
@pytest.mark.parametrize("name", ["EulerDiscreteScheduler", "EulerAncestralDiscreteScheduler"])
def test_restatement_equals_the_library(name, opts, karras):
    cls = getattr(diffusers, name)
    kw = dict(BASE, **opts)
    if karras:
        if "use_karras_sigmas" not in inspect.signature(cls.__init__).parameters:
            pytest.skip(f"this diffusers' {name} has no use_karras_sigmas")
        kw["use_karras_sigmas"] = True
    lib, r = cls(**kw), getattr(SC, name)(use_karras_sigmas=karras, **opts)
    assert float(lib.init_noise_sigma) == pytest.approx(float(r.init_noise_sigma), rel=1e-6)
    for N in (1, 6, 25):
        lib.set_timesteps(N)
        r.set_timesteps(N)
        assert torch.equal(lib.timesteps.float(), r.timesteps), (N, lib.timesteps, r.timesteps)
        assert torch.equal(lib.sigmas.float(), r.sigmas)
        assert float(lib.init_noise_sigma) == pytest.approx(float(r.init_noise_sigma), rel=1e-6)
        g = torch.Generator().manual_seed(N)
        x = torch.randn(2, 4, 8, 8, generator=g) * float(r.init_noise_sigma)
        gl, gr = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
        xl = xr = x
        for t in r.timesteps:
            e = torch.randn(2, 4, 8, 8, generator=g)
            assert torch.allclose(lib.scale_model_input(xl, t), r.scale_model_input(xr, t), rtol=1e-6, atol=1e-6)
            xl = lib.step(e, t, xl, generator=gl, return_dict=False)[0]
            xr = r.step(e, t, xr, generator=gr)[0]
            assert torch.allclose(xl, xr, rtol=1e-5, atol=1e-5 * float(r.sigmas[0])), float((xl - xr).abs().max())
        assert r.draws == N
        assert torch.equal(torch.randn(3, generator=gl), torch.randn(3, generator=gr)), "number of generator draws"
        tt = r.timesteps[N // 2:N // 2 + 1].repeat(2)
        lib.set_timesteps(N)
        assert torch.allclose(lib.add_noise(x, 2 * x, tt), r.add_noise(x, 2 * x, tt), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("N", [6, 25, 100])
def test_dpm_karras_grid_equals_the_library(N):
    lib = diffusers.DPMSolverMultistepScheduler(use_karras_sigmas=True, **BASE)
    r = SC.DPMKarras()
    lib.set_timesteps(N)
    r.set_timesteps(N)
    assert torch.equal(lib.timesteps.long(), r.timesteps)
    assert torch.equal(lib.sigmas.float(), r.sigmas)
