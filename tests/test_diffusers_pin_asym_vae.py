"""Pin of tests/asym_vae_cases.py (the restatement every AsymmetricAutoencoderKL test compares with) to the library itself:
skipped where diffusers does not import; elsewhere the restatement must agree with `diffusers.AsymmetricAutoencoderKL` on
the tiny config -- state-dict keys and shapes, encode, unconditioned and conditioned decode -- in fp32."""
import pytest
import torch

import asym_vae_cases as AC

diffusers = pytest.importorskip("diffusers")


def _library_model():
    c = AC.TINY
    torch.manual_seed(0)
    m = diffusers.AsymmetricAutoencoderKL(
        in_channels=c["in_channels"], out_channels=c["out_channels"], latent_channels=c["latent_channels"],
        down_block_types=("DownEncoderBlock2D",) * len(c["down"]), down_block_out_channels=c["down"],
        layers_per_down_block=c["layers_down"], up_block_types=("UpDecoderBlock2D",) * len(c["up"]),
        up_block_out_channels=c["up"], layers_per_up_block=c["layers_up"], norm_num_groups=c["groups"]).eval()
    with torch.no_grad():
        for p in m.parameters():                      # biases and norm affines away from their (0, 1) initial values
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    return m


def test_restatement_matches_the_library():
    m = _library_model()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    got = [tuple(sd[f"decoder.condition_encoder.layers.{l}.weight"].shape) for l in range(5)]
    assert got == AC.condition_encoder_weight_shapes(AC.TINY)
    try:
        from powerpaint_amd.vae_asym import AsymVAENet
        c = AC.TINY
        sp = AsymVAENet(3, 3, 4, c["down"], c["layers_down"], c["up"], c["layers_up"], c["groups"]).state_dict_spec()
        assert set(sp) == set(sd) and all(tuple(sd[k].shape) == sp[k] for k in sp)
    except ImportError:
        pass
    g = torch.Generator().manual_seed(1)
    z = torch.randn(2, 4, 3, 5, generator=g)
    img = torch.rand(2, 3, 24, 40, generator=g) * 2 - 1
    for mask in (AC.two_masks(2, 24, 40), AC.two_masks(2, 24, 40, fractional=True)):
        with torch.no_grad():
            want = m.decode(z, image=img, mask=mask).sample
            assert torch.allclose(AC.decode(sd, AC.TINY, z, img, mask), want, atol=2e-5, rtol=1e-4)
    with torch.no_grad():
        assert torch.allclose(AC.decode(sd, AC.TINY, z), m.decode(z).sample, atol=2e-5, rtol=1e-4)
        x = torch.rand(2, 3, 24, 40, generator=g) * 2 - 1
        assert torch.allclose(AC.encode_moments(sd, AC.TINY, x), m.encode(x).latent_dist.parameters, atol=2e-5, rtol=1e-4)
    assert m.config.block_out_channels == AC.TINY["up"] or tuple(m.config.block_out_channels) == AC.TINY["up"]
