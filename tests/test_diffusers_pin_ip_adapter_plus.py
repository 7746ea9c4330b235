"""Parity pin: IP-Adapter Plus's image projection against diffusers itself (0.27.0 is the version the reference pins).  Skipped
where diffusers is not installed -- tests/golden/README_ip_adapter_plus.md says "parity unpinned until this runs".  Three
questions: is the Resampler restated from the file format (tests/ip_plus_cases.Resampler) the arithmetic of diffusers'
`IPAdapterPlusImageProjection` once diffusers has converted the file's keys, does the package's module carry diffusers' parameter
names and values (powerpaint_amd.ip_adapter.IPAdapterPlusImageProjection, plus_key_conversion), and does
`MultiIPAdapterImageProjection` reshape 4-D embeds as ours does."""
import os
import sys

import pytest
import torch

diffusers = pytest.importorskip("diffusers")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ip_adapter_cases as IC  # noqa: E402
import ip_plus_cases as PC  # noqa: E402
from powerpaint_amd import ip_adapter as IPA  # noqa: E402

TINY = dict(block_out_channels=(320, 640), layers_per_block=1, cross_attention_dim=768, attention_head_dim=8,
            down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"))
SIZES = dict(Q=16, dim=128, E=64, depth=2, heads=2, ff=512)          # (diffusers derives ff = 4 dim from the file)


def _loaded():
    from oracle import sd_modules as OM
    u = diffusers.UNet2DConditionModel(in_channels=4, out_channels=4, **TINY)
    o = OM.UNet2DConditionModel(in_channels=4, **{k: v for k, v in TINY.items()})
    sd = PC.plus_state_dict(o, 5, **SIZES)
    u._load_ip_adapter_weights([sd])
    return u, sd


def test_restated_resampler_is_the_diffusers_projection():
    from diffusers.models.embeddings import IPAdapterPlusImageProjection
    u, sd = _loaded()
    (theirs,) = u.encoder_hid_proj.image_projection_layers
    assert isinstance(theirs, IPAdapterPlusImageProjection)
    mine = PC.Resampler.from_file(sd["image_proj"])
    x = torch.randn(3, 10, SIZES["E"], generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want, got = theirs(x), mine(x)
    assert torch.allclose(got, want, atol=1e-5, rtol=1e-5), float((got - want).abs().max())


def test_package_module_has_the_diffusers_names_and_values():
    from powerpaint_amd.engine import SDNet
    u, sd = _loaded()
    (theirs,) = u.encoder_hid_proj.image_projection_layers
    net = SDNet("unet", 4, block_out_channels=TINY["block_out_channels"], layers_per_block=1,
                down_block_types=TINY["down_block_types"], up_block_types=TINY["up_block_types"])
    net.load_state_dict(net.synthetic_state_dict(meta=True), "cpu", materialize=False)
    ours = IPA.plus_projection_module(IPA.check_ip_adapter(net, sd))
    a, b = ours.state_dict(), theirs.state_dict()
    assert set(a) == set(b)
    assert all(torch.equal(a[k], b[k]) for k in a)
    x = torch.randn(2, 10, SIZES["E"], generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        assert torch.allclose(ours(x), theirs(x), atol=1e-5, rtol=1e-5)


def test_multi_projection_reshapes_4d_embeds_as_diffusers_does():
    from diffusers.models.embeddings import MultiIPAdapterImageProjection
    u, sd = _loaded()
    theirs = u.encoder_hid_proj
    assert isinstance(theirs, MultiIPAdapterImageProjection)
    mine = IC.MultiProjection([PC.Resampler.from_file(sd["image_proj"])])
    e = [torch.randn(2, 2, 10, SIZES["E"], generator=torch.Generator().manual_seed(3))]
    with torch.no_grad():
        want, got = theirs(e), mine(e)
    assert got[0].shape == want[0].shape == (2, 32, 768) and torch.allclose(got[0], want[0], atol=1e-5, rtol=1e-5)
