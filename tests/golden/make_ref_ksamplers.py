#!/usr/bin/env python
"""Generate tests/golden/ref_ksamplers.pt (data only; run where the reference sources are): what the REFERENCE'S OWN pipeline
`__call__`s produce when they are driven by a second-order or multistep sigma-space scheduler.

Through oracle/ref_pipeline.py (unchanged) the reference's `StableDiffusionInpaintPipeline.__call__` and
`StableDiffusionPowerPaintBrushNetPipeline.__call__` run with the restated diffusers-0.27 schedulers of
tests/ksampler_cases.py, on the reduced SD-1.5 nets, inputs and calls of make_ref_lcm (the nets of
make_ref_wiring.oracle_models(); 16x16 latents, batch 2, guidance 7.5, a CPU generator seeded 5); the schedulers carry the
SD-1.5 checkpoint's `leading` spacing with steps_offset 1, so init_noise_sigma = sqrt(sigma_max^2 + 1).
  heun                  v1, 9-channel UNet, Heun, 5 steps (9 network evaluations)
  heun_karras_strength  v1, Heun with Karras sigmas at strength 0.5 with 6 steps: the loop runs entries 6..10 of the 11
  dpm2                  BrushNet + 4-channel UNet, DPM2, 5 steps (fractional midpoint timesteps)
  dpm2_a                v1, DPM2 ancestral, 5 steps (one draw per evaluation)
  lms_karras            BrushNet + 4-channel UNet, LMS with Karras sigmas, 6 steps
Stored per case: the final latents and the generator's next draw after the call.

`oracle_run(name)` is the same call through the oracle's restated loop bodies (oracle/loops.py) -- tests/test_ksamplers.py
checks them against the fixture on the CPU at make_ref_lcm's ATOL / RTOL.  `oracle_run("lms_karras", exact=True)` swaps the
quadrature of the LMS coefficients for the product's exact polynomial integral."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import ksampler_cases as KC  # noqa: E402
import make_ref_lcm as ML  # noqa: E402
import make_ref_pipeline_call as MP  # noqa: E402

ATOL, RTOL = ML.ATOL, ML.RTOL
SEED, NB = ML.SEED, ML.NB
SD15 = dict(timestep_spacing="leading", steps_offset=1)
# name -> (pipeline of make_ref_lcm.components, scheduler class, its options, the call)
CASES = dict(
    heun=("v1", KC.HeunDiscreteScheduler, SD15, dict(MP.CALL, num_inference_steps=5, num_images_per_prompt=NB)),
    heun_karras_strength=("v1", KC.HeunDiscreteScheduler, dict(SD15, use_karras_sigmas=True),
                          dict(MP.CALL, num_inference_steps=6, strength=0.5, num_images_per_prompt=NB)),
    dpm2=("v2", KC.KDPM2DiscreteScheduler, SD15, dict(MP.CALL_V2, num_inference_steps=5, num_images_per_prompt=NB)),
    dpm2_a=("v1", KC.KDPM2AncestralDiscreteScheduler, SD15, dict(MP.CALL, num_inference_steps=5, num_images_per_prompt=NB)),
    lms_karras=("v2", KC.LMSDiscreteScheduler, dict(SD15, use_karras_sigmas=True),
                dict(MP.CALL_V2, num_inference_steps=6, num_images_per_prompt=NB)))


def ref_run(name):
    from oracle import ref_pipeline
    from oracle import sd_modules as OM
    kind, cls, opts, c = CASES[name]
    g = torch.Generator().manual_seed(SEED)
    with torch.no_grad():
        if kind == "v2":
            Pipe = ref_pipeline.load_reference_brushnet_pipeline_class(OM.BrushNetModel)
            tok, enc, unet, bn, vae = ML.components("v2")
            pipe = Pipe(vae=vae, text_encoder=enc, text_encoder_brushnet=enc, tokenizer=tok, unet=unet, brushnet=bn,
                        scheduler=cls(**opts), safety_checker=None, feature_extractor=None, requires_safety_checker=False)
            img, mask3, _ = MP.inputs_v2()
            torch.manual_seed(9)                            # the conditioning latents are sampled from the global RNG
            out = pipe(image=img, mask=mask3, latents=ML.start_latents(), generator=g, output_type="latent",
                       return_dict=False, **c)[0]
        else:
            Pipe, _ = ref_pipeline.load_reference_pipeline_class()
            tok, enc, unet, vae = ML.components("v1")
            pipe = Pipe(vae=vae, text_encoder=enc, tokenizer=tok, unet=unet, scheduler=cls(**opts), safety_checker=None,
                        feature_extractor=None, requires_safety_checker=False)
            img, mask, _ = MP.inputs()
            kw = dict(latents=ML.start_latents()) if "strength" not in c else {}
            out = pipe(image=img, mask=mask, generator=g, output_type="latent", return_dict=False, **kw, **c)[0]
    return out, torch.randn(4, generator=g)


class _ExactLMS(KC.LMSDiscreteScheduler):
    """The restated LMS with the product's closed-form coefficient in place of the quadrature."""

    def set_timesteps(self, num_inference_steps, device=None):
        from powerpaint_amd import schedulers as PS
        super().set_timesteps(num_inference_steps, device)
        c = self.config
        self._exact = PS.LMSDiscreteScheduler(timestep_spacing=c.timestep_spacing, steps_offset=c.steps_offset,
                                              use_karras_sigmas=c.use_karras_sigmas)
        self._exact.set_timesteps(num_inference_steps)

    def get_lms_coefficient(self, order, t, current_order):
        return self._exact.lms_coefficient(order, t, current_order)


def oracle_run(name, exact=False):
    """The same call through oracle/loops.py with the restated scheduler -> (final latents, the generator's next draw)."""
    from oracle import loops as OL
    kind, cls, opts, c = CASES[name]
    if exact:
        cls = _ExactLMS
    g = torch.Generator().manual_seed(SEED)
    with torch.no_grad():
        if kind == "v2":
            tok, enc, unet, bn, vae = ML.components("v2")
            img, mask3, _ = MP.inputs_v2()
            pe, peU = ML.prompts(tok, enc, c)
            torch.manual_seed(9)
            rep = torch.cat([img.repeat(NB, 1, 1, 1)] * 2)
            cl = vae.encode(rep).latent_dist.sample() * vae.config.scaling_factor
            keep = (torch.cat([mask3.repeat(NB, 1, 1, 1)] * 2).sum(1)[:, None] < 0).float()
            cond = torch.cat([cl, torch.nn.functional.interpolate(keep, size=cl.shape[-2:])], 1)
            sch = cls(generator=g, **opts)                              # (loop_v2 hands no generator to `step`)
            out = OL.loop_v2(unet, bn, sch, ML.start_latents(), cond, pe, peU, c["num_inference_steps"],
                             c["guidance_scale"], c["brushnet_conditioning_scale"])
        else:
            tok, enc, unet, vae = ML.components("v1")
            img, mask, _ = MP.inputs()
            pe, _ = ML.prompts(tok, enc, c)
            sch = cls(**opts)
            sch.set_timesteps(c["num_inference_steps"])
            t_start = 0
            if "strength" in c:
                t_start = c["num_inference_steps"] - int(c["num_inference_steps"] * c["strength"])
                il = vae.encode(img).latent_dist.sample(g) * vae.config.scaling_factor
                noise = torch.randn(NB, 4, 16, 16, generator=g)
                first = sch.timesteps[t_start * sch.order:t_start * sch.order + 1]
                lat = sch.add_noise(il, noise, first.repeat(NB))
            else:
                lat = ML.start_latents()
            mil = (vae.encode(img * (mask < 0.5)).latent_dist.sample(g) * vae.config.scaling_factor).repeat(NB, 1, 1, 1)
            m = torch.nn.functional.interpolate(mask, size=(16, 16)).repeat(NB, 1, 1, 1)
            out = OL.loop_v1(unet, sch, lat, torch.cat([m] * 2), torch.cat([mil] * 2), pe, c["num_inference_steps"],
                             c["guidance_scale"], t_start=t_start, generator=g)
    return out, torch.randn(4, generator=g)


def main():
    gold = {}
    for name in CASES:
        out, nxt = ref_run(name)
        gold[name] = dict(latents=out, next_draw=nxt)
        o, n2 = oracle_run(name)
        print(name, tuple(out.shape), "max|ref|", float(out.abs().max()), "oracle loop max err", float((o - out).abs().max()),
              "next draw equal", bool(torch.equal(nxt, n2)))
    o, _ = oracle_run("lms_karras", exact=True)
    ref = gold["lms_karras"]["latents"]
    print("lms_karras with the exact LMS coefficients: max err vs the quadrature run", float((o - ref).abs().max()),
          "worst err / (ATOL + RTOL |ref|)", float(((o - ref).abs() / (ATOL + RTOL * ref.abs())).max()))
    path = os.path.join(HERE, "ref_ksamplers.pt")
    torch.save(gold, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
