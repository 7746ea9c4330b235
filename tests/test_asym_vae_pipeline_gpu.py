"""GPU: what the pipelines hand to `vae.decode` when the VAE is an AsymmetricAutoencoderKL, against what the reference's own
`__call__`s hand over (tests/golden/ref_asym_vae.json, recorded by tests/golden/make_ref_asym_vae.py with a recording VAE):
the same `image` and `mask` bytes, shapes and dtypes, and the caller's generator left in the same state.

v1 (`StableDiffusionInpaintPipeline`) conditions the decode.  The ControlNet pipeline's reference `__call__` does not -- the
fixture records a decode without keyword arguments -- and neither does the product's."""
import hashlib
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

pytestmark = pytest.mark.gpu

VAE_KW = dict(down_block_types=("DownEncoderBlock2D",) * 4, down_block_out_channels=(64, 128, 256, 256),
              layers_per_down_block=1, up_block_types=("UpDecoderBlock2D",) * 4, up_block_out_channels=(64, 128, 256, 256),
              layers_per_up_block=1)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def recording(base, **kw):
    """A stand-in of class `base` (no weights): encodes to a zero-mean unit posterior, records what decode receives."""
    from powerpaint_amd.models._base import Output
    from powerpaint_amd.models.autoencoder_kl import DiagonalGaussianDistribution

    class Recording(base):
        seen = None

        def encode(self, x, return_dict=True):
            B, _, H, W = x.shape
            return Output(latent_dist=DiagonalGaussianDistribution(torch.zeros(B, 8, H // 8, W // 8, device="cuda")))

        def decode(self, z, return_dict=True, **kwargs):
            self.seen = dict(latents=list(z.shape), kwargs=kwargs)
            return (torch.zeros(z.shape[0], 3, 8 * z.shape[2], 8 * z.shape[3], device="cuda"),)

    return Recording(device="cuda", **kw)


def components(M, cn=False):
    from powerpaint_amd import models as PM
    tok, enc, unet, *rest = M.components_cn() if cn else M.components()
    hu = PM.UNet2DConditionModel(in_channels=9, device="cuda", **M.TINY).load_state_dict(unet.state_dict())
    he = PM.CLIPTextModel(device="cuda", vocab_size=enc.config.vocab_size, num_hidden_layers=1,
                          eos_token_id=enc.config.eos_token_id)
    he.load_state_dict(enc.state_dict())
    out = dict(text_encoder=he, tokenizer=tok, unet=hu)
    if cn:
        no_up = {k: v for k, v in M.TINY.items() if k != "up_block_types"}
        out["controlnet"] = PM.ControlNetModel(in_channels=4, device="cuda", **no_up).load_state_dict(rest[0].state_dict())
    return out


def check(seen, gold, generator):
    assert seen is not None, "vae.decode was not called"
    assert seen["latents"] == gold["latents"] and sorted(seen["kwargs"]) == gold["kwargs"]
    for k in gold["kwargs"]:
        t = seen["kwargs"][k]
        assert t.is_cuda and list(t.shape) == gold[k]["shape"] and str(t.dtype) == gold[k]["dtype"], k
        assert sha(t) == gold[k]["sha256"], f"{k}: other bytes than the reference hands over"
    gens = generator if isinstance(generator, list) else [generator]
    assert [sha(g.get_state()) for g in gens] == gold["generator"], "the generator is left in another state"


@pytest.mark.parametrize("name", ["v1", "v1_generator_list", "v1_strength"])
def test_v1_pipeline_hands_decode_what_the_reference_does(name):
    import make_ref_asym_vae as G
    import make_ref_pipeline_call as M
    from powerpaint_amd import models as PM, pipelines as PP, schedulers as PS
    gold = json.load(open(os.path.join(HERE, "golden", "ref_asym_vae.json")))[name]
    kind, gen, mask, extra = G.cases()[name]
    vae = recording(PM.AsymmetricAutoencoderKL, **VAE_KW)
    pipe = PP.StableDiffusionInpaintPipeline(vae=vae, scheduler=PS.DDIMScheduler(), **components(M))
    img, _, lat = M.inputs()
    kw = dict(M.CALL, image=img, mask=mask, latents=lat.cuda())
    kw.update(extra)
    generator = gen()
    out = pipe(generator=generator, output_type="pt", return_dict=False, **kw)[0]
    assert out.shape == (1, 3, 128, 128)
    check(vae.seen, gold, generator)
    # output_type="latent": nothing is decoded, nothing is drawn
    vae.seen, g2 = None, gen()
    before = [sha(g.get_state()) for g in (g2 if isinstance(g2, list) else [g2])]
    pipe(generator=g2, output_type="latent", return_dict=False, **kw)
    assert vae.seen is None
    if name == "v1":                        # (latents given, strength 1: the only draw left is the masked image's posterior)
        g3 = gen()
        torch.randn(1, 4, 16, 16, generator=g3)
        assert [sha(g2.get_state())] == [sha(g3.get_state())] != before


def test_controlnet_pipeline_and_plain_vae_decode_unconditioned():
    import make_ref_asym_vae as G
    import make_ref_pipeline_call as M
    from powerpaint_amd import models as PM, pipelines as PP, schedulers as PS
    gold = json.load(open(os.path.join(HERE, "golden", "ref_asym_vae.json")))["controlnet"]
    kind, gen, mask, extra = G.cases()["controlnet"]
    assert gold["kwargs"] == []                # the reference's ControlNet __call__ has no AsymmetricAutoencoderKL branch
    vae = recording(PM.AsymmetricAutoencoderKL, **VAE_KW)
    pipe = PP.StableDiffusionControlNetInpaintPipeline(vae=vae, scheduler=PS.DDIMScheduler(), **components(M, cn=True))
    img, _, lat = M.inputs()
    generator = gen()
    pipe(image=img, mask=mask, control_image=M.control_image(), latents=lat.cuda(), generator=generator, output_type="pt",
         return_dict=False, **M.CALL_CN)
    check(vae.seen, gold, generator)
    # a plain AutoencoderKL in the v1 pipeline: decode gets nothing extra, the generator is where the ControlNet call leaves
    # it (the same draws up to the decode: latents given, one posterior sample of the masked image)
    plain = recording(PM.AutoencoderKL, block_out_channels=(64, 128, 256, 256), layers_per_block=1)
    comp = components(M)
    pipe = PP.StableDiffusionInpaintPipeline(vae=plain, scheduler=PS.DDIMScheduler(), **comp)
    generator = gen()
    pipe(image=img, mask=mask, latents=lat.cuda(), generator=generator, output_type="pt", return_dict=False, **M.CALL)
    check(plain.seen, gold, generator)
