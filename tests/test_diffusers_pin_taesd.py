"""Pin of tests/taesd_cases.py (the restatement every AutoencoderTiny test compares with) to the library itself: skipped where
diffusers does not import; elsewhere the restatement must agree with `diffusers.AutoencoderTiny` on one state dict -- keys and
shapes, encode, decode and forward -- in fp32."""
import pytest
import torch

import taesd_cases as TC

diffusers = pytest.importorskip("diffusers")


def test_restatement_matches_the_library():
    torch.manual_seed(0)
    m = diffusers.AutoencoderTiny().eval()
    with torch.no_grad():
        for p in m.parameters():                      # biases away from their initial values
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    sp = TC.spec(TC.DEFAULT)
    assert set(sp) == set(sd) and all(tuple(sd[k].shape) == sp[k] for k in sp)
    assert tuple(m.config.block_out_channels) == (64,) * 4 and m.config.scaling_factor == 1.0
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 3, 24, 40, generator=g) * 2 - 1
    z = torch.randn(2, 4, 3, 5, generator=g) * 3
    with torch.no_grad():
        assert torch.allclose(TC.encode(sd, TC.DEFAULT, x), m.encode(x).latents, atol=2e-5, rtol=1e-4)
        assert torch.allclose(TC.decode(sd, TC.DEFAULT, z), m.decode(z).sample, atol=2e-5, rtol=1e-4)
        assert torch.allclose(TC.forward(sd, TC.DEFAULT, x), m(x).sample, atol=2e-5, rtol=1e-4)
        assert torch.equal(TC.scale_latents(z), m.scale_latents(z)) and torch.equal(TC.unscale_latents(z), m.unscale_latents(z))
