"""Parity pin: the restated Heun / DPM2 / DPM2 ancestral / LMS schedulers of tests/ksampler_cases.py against diffusers itself
(0.27.0 is the version the reference pins).  Skipped where diffusers is not installed -- tests/golden/README_ksamplers.md says
"parity unpinned" until this file has run somewhere.  Two questions in particular are answered here: DPM2 ancestral's draw
schedule (one `randn_tensor` per `step` call, both stages, is what the restatement assumes) and LMS entered at a begin index > 0
(the order follows the absolute step index while the derivative list starts empty)."""
import os
import sys

import pytest
import torch

diffusers = pytest.importorskip("diffusers")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ksampler_cases as KC  # noqa: E402

SPACINGS = [dict(timestep_spacing="linspace"), dict(timestep_spacing="leading", steps_offset=1),
            dict(timestep_spacing="trailing")]
BASE = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
NAMES = list(KC.CLASSES)


def _pair(name, opts, karras):
    return getattr(diffusers, name)(use_karras_sigmas=karras, **dict(BASE, **opts)), KC.CLASSES[name](use_karras_sigmas=karras, **opts)


@pytest.mark.parametrize("karras", [False, True], ids=["plain", "karras"])
@pytest.mark.parametrize("opts", SPACINGS, ids=["linspace", "leading", "trailing"])
@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_library(name, opts, karras):
    lib, r = _pair(name, opts, karras)
    assert lib.order == r.order
    assert float(lib.init_noise_sigma) == pytest.approx(float(r.init_noise_sigma), rel=1e-6)
    for N in (1, 2, 7):
        lib.set_timesteps(N)
        r.set_timesteps(N)
        assert torch.equal(lib.timesteps.float(), r.timesteps), (N, lib.timesteps, r.timesteps)
        assert torch.equal(lib.sigmas.float(), r.sigmas)
        for extra in ("sigmas_interpol", "sigmas_up", "sigmas_down"):
            if hasattr(r, extra):
                assert torch.equal(getattr(lib, extra).float().nan_to_num(), getattr(r, extra).nan_to_num()), extra
        assert float(lib.init_noise_sigma) == pytest.approx(float(r.init_noise_sigma), rel=1e-6)
        g = torch.Generator().manual_seed(N)
        x = torch.randn(2, 4, 8, 8, generator=g) * float(r.init_noise_sigma)
        gl, gr = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
        xl = xr = x
        for k, t in enumerate(r.timesteps):
            e = torch.randn(2, 4, 8, 8, generator=g)
            assert torch.allclose(lib.scale_model_input(xl, t), r.scale_model_input(xr, t), rtol=1e-6, atol=1e-6)
            kw = dict(generator=gl) if name == "KDPM2AncestralDiscreteScheduler" else {}
            xl = lib.step(e, t, xl, return_dict=False, **kw)[0]
            xr = r.step(e, t, xr, generator=gr)[0]
            assert torch.allclose(xl, xr, rtol=1e-5, atol=1e-5 * float(r.sigmas[0])), (k, float((xl - xr).abs().max()))
            # the generator's position after EVERY call: DPM2 ancestral's draw schedule
            a, b = gl.get_state(), gr.get_state()
            assert torch.equal(a, b), f"generator position after call {k}"
        assert r.draws == (len(r.timesteps) if name == "KDPM2AncestralDiscreteScheduler" else 0)


@pytest.mark.parametrize("name", NAMES)
def test_entering_the_schedule_late(name):
    """`strength < 1`: the pipelines hand `timesteps[t_start * order:]` to the loop and noise the init image to its first entry.
    For LMS this is the begin-index question: order min(step_index + 1, 4) with one derivative in the list."""
    lib, r = _pair(name, SPACINGS[1], False)
    N, t_start = 6, 3
    lib.set_timesteps(N)
    r.set_timesteps(N)
    ts = r.timesteps[t_start * r.order:]
    g = torch.Generator().manual_seed(3)
    x0, nz = torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 4, 8, 8, generator=g)
    xl = lib.add_noise(x0, nz, lib.timesteps[t_start * lib.order:][:1].repeat(2))
    xr = r.add_noise(x0, nz, ts[:1].repeat(2))
    assert torch.allclose(xl, xr, rtol=1e-6, atol=1e-6)
    gl, gr = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    for k, t in enumerate(ts):
        e = torch.randn(2, 4, 8, 8, generator=g)
        assert torch.allclose(lib.scale_model_input(xl, t), r.scale_model_input(xr, t), rtol=1e-6, atol=1e-6)
        kw = dict(generator=gl) if name == "KDPM2AncestralDiscreteScheduler" else {}
        xl = lib.step(e, t, xl, return_dict=False, **kw)[0]
        xr = r.step(e, t, xr, generator=gr)[0]
        assert torch.allclose(xl, xr, rtol=1e-5, atol=1e-5 * float(r.sigmas[0])), (k, float((xl - xr).abs().max()))
    assert torch.equal(gl.get_state(), gr.get_state())
