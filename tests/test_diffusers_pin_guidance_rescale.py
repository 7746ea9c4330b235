"""Parity pin: the restated rule of `guidance_rescale` (powerpaint_amd/guidance.py, tests/guidance_cases.py) against diffusers'
own `rescale_noise_cfg`.  Skipped where diffusers does not import -- README.md says "parity unpinned until this runs"."""
import os
import sys

import numpy as np
import pytest
import torch

pytest.importorskip("diffusers")
from diffusers.pipelines.stable_diffusion.pipeline_stable_diffusion import rescale_noise_cfg  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import guidance_cases as GC  # noqa: E402
from powerpaint_amd import guidance as GDM  # noqa: E402


@pytest.mark.parametrize("segs", [2, 3])
@pytest.mark.parametrize("phi", [0.3, 0.7, 1.0])
def test_rescale_is_rescale_noise_cfg(segs, phi):
    gq = torch.Generator().manual_seed(segs)
    B, shape = 3, (4, 6, 10)
    e = torch.randn(segs, B, *shape, generator=gq, dtype=torch.float64) * 2 + 0.5
    g, s = 7.5, 2.5
    noise_cfg = e[0] + g * (e[1] - e[0]) + (s * (e[1] - e[2]) if segs == 3 else 0.0)
    want = rescale_noise_cfg(noise_cfg, e[1], guidance_rescale=phi)
    got = GC.rescale_f64(e.reshape(segs, B, -1).numpy(), segs, g, s, phi)
    assert np.allclose(got, want.reshape(B, -1).numpy(), rtol=1e-12, atol=0)
    assert torch.allclose(GDM.rescale_noise_cfg(noise_cfg, e[1], phi), want, rtol=1e-12, atol=0)
    assert torch.allclose(GC.rescale_tensor(noise_cfg, e[1], phi), want, rtol=1e-12, atol=0)
