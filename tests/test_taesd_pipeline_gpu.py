"""GPU: the pipelines with an AutoencoderTiny (synthetic weights) as `vae`, on the tiny components of
tests/test_asym_vae_pipeline_gpu.py: two steps, `output_type="pt"`.

  * the image is `vae.decode(latents / scaling_factor)` of the same call's `output_type="latent"` result, denormalised;
  * the encode draws nothing: the caller's generator ends where drawing the initial noise alone leaves it (an AutoencoderKL
    would draw the posterior's noise behind it), and the global RNG, which the BrushNet pipeline's encode samples from with a
    posterior, is not touched;
  * decoding the running latents in a step callback (the preview use) leaves the fused loop's result bitwise unchanged.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

pytestmark = pytest.mark.gpu

STEPS = 2


def tiny_vae(seed=21):
    from powerpaint_amd.models import AutoencoderTiny
    vae = AutoencoderTiny(device="cuda")
    vae.load_state_dict(vae.net.synthetic_state_dict(seed=seed))
    return vae


def text(M, enc):
    from powerpaint_amd import models as PM
    he = PM.CLIPTextModel(device="cuda", vocab_size=enc.config.vocab_size, num_hidden_layers=1,
                          eos_token_id=enc.config.eos_token_id)
    he.load_state_dict(enc.state_dict())
    return he


def expect_image(vae, latents):
    return (vae.decode(latents / vae.config.scaling_factor, return_dict=False)[0] / 2 + 0.5).clamp(0, 1)


def test_inpaint_pipeline_with_the_tiny_vae():
    import make_ref_pipeline_call as M
    from powerpaint_amd import models as PM, pipelines as PP, schedulers as PS
    tok, enc, unet, _ = M.components()
    hu = PM.UNet2DConditionModel(in_channels=9, device="cuda", **M.TINY).load_state_dict(unet.state_dict())
    vae = tiny_vae()
    pipe = PP.StableDiffusionInpaintPipeline(vae=vae, text_encoder=text(M, enc), tokenizer=tok, unet=hu,
                                             scheduler=PS.DDIMScheduler())
    assert pipe.vae_scale_factor == 8
    img, mask, _ = M.inputs()
    kw = dict(M.CALL, image=img, mask=mask, num_inference_steps=STEPS, return_dict=False)
    gen = lambda: torch.Generator().manual_seed(5)      # noqa: E731
    g1 = gen()
    lat = pipe(generator=g1, output_type="latent", **kw)[0]
    assert lat.shape == (1, 4, 16, 16)
    out = pipe(generator=gen(), output_type="pt", **kw)[0]
    assert out.shape == (1, 3, 128, 128)
    assert torch.equal(out, expect_image(vae, lat))
    # the generator: only the initial noise was drawn (the masked image's encode has no posterior to sample)
    g2 = gen()
    torch.randn(1, 4, 16, 16, generator=g2)
    assert torch.equal(g1.get_state(), g2.get_state())
    # a preview in every step: the result of the loop is the same, bit for bit
    seen = []
    lat_cb = pipe(generator=gen(), output_type="latent", **kw,
                  callback=lambda i, t, l: seen.append(vae.decode(l / vae.config.scaling_factor).sample.clone()))[0]
    assert torch.equal(lat_cb, lat)
    assert len(seen) == STEPS and all(s.shape == (1, 3, 128, 128) for s in seen) and not torch.equal(seen[0], seen[-1])
    assert torch.equal((seen[-1] / 2 + 0.5).clamp(0, 1), out)                   # the last preview is the final image


def test_brushnet_pipeline_with_the_tiny_vae():
    import make_ref_pipeline_call as M
    from powerpaint_amd import models as PM, pipelines as PP, schedulers as PS
    tok, enc, unet, bn, _ = M.components_v2()
    hu = PM.UNet2DConditionModel(in_channels=4, device="cuda", **M.TINY).load_state_dict(unet.state_dict())
    hb = PM.BrushNetModel(in_channels=4, conditioning_channels=5, device="cuda", **M.TINY).load_state_dict(bn.state_dict())
    he = text(M, enc)
    vae = tiny_vae()
    pipe = PP.StableDiffusionPowerPaintBrushNetPipeline(vae=vae, text_encoder=he, text_encoder_brushnet=he, tokenizer=tok,
                                                        unet=hu, brushnet=hb, scheduler=PS.DPMSolverMultistepScheduler())
    assert pipe.vae_scale_factor == 8
    img, mask3, _ = M.inputs_v2()
    kw = dict(M.CALL_V2, image=img, mask=mask3, num_inference_steps=STEPS, return_dict=False)
    gen = lambda: torch.Generator().manual_seed(6)      # noqa: E731
    torch.manual_seed(9)
    rng = torch.get_rng_state().clone()
    g1 = gen()
    lat = pipe(generator=g1, output_type="latent", **kw)[0]
    assert lat.shape == (1, 4, 16, 16)
    assert torch.equal(torch.get_rng_state(), rng)                              # (a posterior would have been sampled from it)
    out = pipe(generator=gen(), output_type="pt", **kw)[0]
    assert out.shape == (1, 3, 128, 128)
    assert torch.equal(out, expect_image(vae, lat))
    g2 = gen()
    torch.randn(1, 4, 16, 16, generator=g2)
    assert torch.equal(g1.get_state(), g2.get_state())
    seen = []

    def preview(p, i, t, kwargs):
        seen.append(p.vae.decode(kwargs["latents"] / p.vae.config.scaling_factor).sample.clone())
        return {}

    lat_cb = pipe(generator=gen(), output_type="latent", callback_on_step_end=preview, **kw)[0]
    assert torch.equal(lat_cb, lat)
    assert len(seen) == STEPS and not torch.equal(seen[0], seen[-1])
    assert torch.equal((seen[-1] / 2 + 0.5).clamp(0, 1), out)
