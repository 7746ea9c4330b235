"""GPU: AsymmetricAutoencoderKL on the HIP path against its fp32 restatement (tests/asym_vae_cases.py), tiny config.

Gate: the one tests/test_vae.py holds the AutoencoderKL decode to against ITS restatement -- cosine >= 0.999 and
max-abs / max <= 0.05, fp32 reference with the matrix weights rounded to the 16-bit format the HIP path stores.

Structural checks (no tolerance): with mask = 0 the output does not depend on the latents (every blend takes the condition
tensor: 0 * sample + cond); with mask = 1 the blends hand the sample on unchanged AND the statistics of the five norms behind
them are summed on the same route by both plans (pp_mask_blend, with or without a condition tensor), so the conditioned decode
equals the unconditioned one BIT FOR BIT.
"""
import pytest
import torch
import torch.nn.functional as F

import asym_vae_cases as AC

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
CFG = AC.TINY


def _model(dt, seed=11):
    from powerpaint_amd.models import AsymmetricAutoencoderKL
    c = CFG
    vae = AsymmetricAutoencoderKL(
        in_channels=c["in_channels"], out_channels=c["out_channels"], latent_channels=c["latent_channels"],
        down_block_types=("DownEncoderBlock2D",) * len(c["down"]), down_block_out_channels=c["down"],
        layers_per_down_block=c["layers_down"], up_block_types=("UpDecoderBlock2D",) * len(c["up"]),
        up_block_out_channels=c["up"], layers_per_up_block=c["layers_up"], norm_num_groups=c["groups"], device="cuda",
        dtype=DT[dt])
    sd = vae.net.synthetic_state_dict(seed=seed)
    vae.load_state_dict(sd)
    return vae, AC.rounded_weights(sd, DT[dt])


_MODELS = {}


def model(dt):
    if dt not in _MODELS:
        _MODELS[dt] = _model(dt)
    return _MODELS[dt]


def _close(got, want, cos_min=0.999, rel_max=0.05):
    got, want = got.float().cpu().flatten(), want.float().cpu().flatten()
    cos = F.cosine_similarity(got, want, dim=0).item()
    rel = ((got - want).abs().max() / want.abs().max()).item()
    print(f"cos {cos:.6f} max-abs/max {rel:.4f}")
    assert cos >= cos_min and rel <= rel_max, f"cos {cos:.6f} (>= {cos_min}), max-abs/max {rel:.4f} (<= {rel_max})"


def _inputs(H, W, B=2, seed=5, fractional=False):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, 4, H // 8, W // 8, generator=g) * 3.0
    img = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    return z, img, AC.two_masks(B, H, W, fractional=fractional, seed=seed)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("H,W", [(32, 32), (24, 40)])
def test_decode_matches_the_restatement(dt, H, W):
    vae, sd = model(dt)
    z, img, mask = _inputs(H, W)
    zr = z.to(DT[dt]).float()
    with torch.no_grad():
        want_c = AC.decode(sd, CFG, zr, img, mask)
        want_u = AC.decode(sd, CFG, zr)
    got_c = vae.decode(z.cuda(), image=img.cuda(), mask=mask.cuda(), return_dict=False)[0]
    got_u = vae.decode(z.cuda(), return_dict=False)[0]
    assert got_c.shape == want_c.shape == (2, 3, H, W) and got_c.dtype == torch.float32
    _close(got_c, want_c)
    _close(got_u, want_u)
    assert not torch.equal(got_c, got_u)
    # (tests/test_asym_vae.py: the two restatements are less than 0.99 alike, so the gate tells which one the product follows)
    # deterministic replay, return_dict form, image OR mask missing = unconditioned (as the library)
    assert torch.equal(vae.decode(z.cuda(), image=img.cuda(), mask=mask.cuda()).sample, got_c)
    assert torch.equal(vae.decode(z.cuda(), image=img.cuda()).sample, got_u)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_fractional_mask_and_broadcast_batch(dt):
    vae, sd = model(dt)
    z, img, mask = _inputs(32, 32, fractional=True, seed=8)
    with torch.no_grad():
        want = AC.decode(sd, CFG, z.to(DT[dt]).float(), img[:1], mask)
    got = vae.decode(z.cuda(), image=img[:1].cuda(), mask=mask.cuda(), return_dict=False)[0]      # one image for the batch
    _close(got, want)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_mask_of_zeros_forgets_the_latents_and_mask_of_ones_is_the_unconditioned_decode(dt):
    vae, _ = model(dt)
    z, img, _ = _inputs(24, 40, seed=6)
    z2 = torch.randn(z.shape, generator=torch.Generator().manual_seed(77)) * 3.0
    zeros, ones = torch.zeros(2, 1, 24, 40), torch.ones(2, 1, 24, 40)
    a = vae.decode(z.cuda(), image=img.cuda(), mask=zeros.cuda(), return_dict=False)[0]
    b = vae.decode(z2.cuda(), image=img.cuda(), mask=zeros.cuda(), return_dict=False)[0]
    assert torch.equal(a, b)
    c = vae.decode(z.cuda(), image=img.cuda(), mask=ones.cuda(), return_dict=False)[0]
    u = vae.decode(z.cuda(), return_dict=False)[0]
    assert torch.equal(c, u)                                  # bitwise: same statistics route in both plans
    assert not torch.equal(u, vae.decode(z2.cuda(), return_dict=False)[0])


def test_one_plan_per_shape_and_chunking():
    from powerpaint_amd.models import autoencoder_asym_kl as M
    vae, _ = _model("bf16", seed=3)
    z, img, mask = _inputs(32, 32, B=3, seed=4)
    first = vae.decode(z.cuda(), image=img.cuda(), mask=mask.cuda(), return_dict=False)[0]
    plan, builds = vae._dec_cond.plan, vae._dec_cond.builds
    assert builds == 1
    img2, mask2 = img.flip(0).contiguous(), mask.flip(0).contiguous()
    second = vae.decode(z.cuda(), image=img2.cuda(), mask=mask2.cuda(), return_dict=False)[0]
    assert vae._dec_cond.plan is plan and vae._dec_cond.builds == 1          # new image / mask: nothing re-planned
    assert not torch.equal(first, second)
    assert torch.equal(vae.decode(z.cuda(), image=img.cuda(), mask=mask.cuda(), return_dict=False)[0], first)
    old = M.MAX_BYTES
    try:
        M.MAX_BYTES = 4 * CFG["up"][0] * 32 * 32                            # one image per plan run
        assert vae._chunks(3, 32 * 32) == [(0, 1), (1, 2), (2, 3)]
        parts = vae.decode(z.cuda(), image=img.cuda(), mask=mask.cuda(), return_dict=False)[0]
    finally:
        M.MAX_BYTES = old
    assert torch.equal(parts, first)
    with pytest.raises(ValueError):
        vae.decode(z.cuda(), image=img[:, :, :24].cuda(), mask=mask.cuda())
    with pytest.raises(ValueError):
        vae.decode(z.cuda(), image=img.cuda(), mask=mask[:2].cuda())
    with pytest.raises(ValueError):
        vae.decode(torch.zeros(1, 3, 4, 4, device="cuda"))


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_encode_and_forward(dt):
    vae, sd = model(dt)
    g = torch.Generator().manual_seed(12)
    img = torch.rand(2, 3, 32, 40, generator=g) * 2 - 1
    with torch.no_grad():
        want = AC.encode_moments(sd, CFG, img.to(DT[dt]).float())
    dist = vae.encode(img.cuda()).latent_dist
    assert dist.mean.shape == (2, 4, 16, 20)                               # a two-block encoder halves once
    _close(torch.cat([dist.mean, dist.logvar], 1), torch.cat([want[:, :4], want[:, 4:].clamp(-30, 20)], 1))
    # forward(sample, mask): encode, take the mode, decode conditioned on the sample itself.  The tiny decoder upsamples by 8,
    # the tiny encoder halves once, so the latents of a 32 x 40 image decode to 128 x 160 and the image must have that size:
    # the library fails there too (its blend cannot broadcast) -- the product refuses by name
    with pytest.raises(ValueError):
        vae(img.cuda(), mask=torch.ones(2, 1, 32, 40).cuda())
    out = vae(img.cuda()).sample                                            # no mask: the unconditioned decode of the mode
    assert torch.equal(out, vae.decode(dist.mode()).sample)
