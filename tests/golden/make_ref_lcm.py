#!/usr/bin/env python
"""Generate tests/golden/ref_lcm.pt (data only; run where the reference sources are): what the REFERENCE'S OWN pipeline
`__call__`s produce when they are driven by an LCM scheduler, and what its own `get_guidance_scale_embedding` returns.

Through oracle/ref_pipeline.py (unchanged) the reference's `StableDiffusionInpaintPipeline.__call__` and
`StableDiffusionPowerPaintBrushNetPipeline.__call__` run with the restated diffusers-0.27 `LCMScheduler` of
tests/lcm_cases.py as their scheduler, on the reduced SD-1.5 nets of make_ref_wiring.oracle_models() (the text encoder,
tokenizer and VAE are make_ref_pipeline_call's): 16x16 latents, batch 2 (num_images_per_prompt), guidance 7.5, a CPU
generator seeded 5.
  v1           9-channel UNet, 4 steps
  v1_strength  the same at strength 0.5 with 8 steps: the loop runs entries 4..7 of the schedule
  v2           BrushNet + 4-channel UNet, 4 steps
Stored per case: the final latents and the generator's next draw after the call (3 draws by the schedule's steps but the
last, whatever the entry point); plus `w_embedding[w]` = the reference function on [w, w], d = 256.

`oracle_run(name)` is the same call through the oracle's restated loop bodies (oracle/loops.py) -- tests/test_lcm.py
checks them against the fixture on the CPU at ATOL / RTOL, the bounds of the neighbouring oracle-loop tests of
tests/test_golden.py (2e-4 / 1e-4 of the BrushNet and ControlNet loops)."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import lcm_cases as LC  # noqa: E402
import make_ref_pipeline_call as MP  # noqa: E402
import make_ref_wiring as MW  # noqa: E402
from oracle import sd_modules as OM  # noqa: E402

ATOL, RTOL = 2e-4, 1e-4
SEED = 5
NB = 2
CALLS = dict(v1=dict(MP.CALL, num_inference_steps=4, num_images_per_prompt=NB),
             v1_strength=dict(MP.CALL, num_inference_steps=8, strength=0.5, num_images_per_prompt=NB),
             v2=dict(MP.CALL_V2, num_inference_steps=4, num_images_per_prompt=NB))
W_VALUES = (0.0, 0.5, 6.5)
SD15 = dict(steps_offset=1)          # LCMScheduler.from_config(<SD-1.5 scheduler config>); no effect on the arithmetic
CFG = {k: v for k, v in MW.OCFG.items() if k != "attention_head_dim"}      # constructor arguments of the HIP models


def start_latents():
    return torch.randn(NB, 4, 16, 16, generator=torch.Generator().manual_seed(43))


def components(name):
    """tok, enc, vae of make_ref_pipeline_call; the UNets of make_ref_wiring; BrushNet = from_unet + seeded zero convs."""
    tok, enc, _, vae = MP.components()
    u9, u4 = MW.oracle_models()
    if name == "v2":
        bn = OM.randomize_zero_convs(OM.BrushNetModel.from_unet(u4), seed=11).eval()
        return tok, enc, u4, bn, vae
    return tok, enc, u9, vae


def ref_run(name):
    from oracle import ref_pipeline
    c = CALLS[name]
    g = torch.Generator().manual_seed(SEED)
    with torch.no_grad():
        if name == "v2":
            Pipe = ref_pipeline.load_reference_brushnet_pipeline_class(OM.BrushNetModel)
            tok, enc, unet, bn, vae = components(name)
            pipe = Pipe(vae=vae, text_encoder=enc, text_encoder_brushnet=enc, tokenizer=tok, unet=unet, brushnet=bn,
                        scheduler=LC.LCMScheduler(**SD15), safety_checker=None, feature_extractor=None,
                        requires_safety_checker=False)
            img, mask3, _ = MP.inputs_v2()
            torch.manual_seed(9)                            # the conditioning latents are sampled from the global RNG
            out = pipe(image=img, mask=mask3, latents=start_latents(), generator=g, output_type="latent",
                       return_dict=False, **c)[0]
            emb = {w: pipe.get_guidance_scale_embedding(torch.tensor([w, w]), embedding_dim=256) for w in W_VALUES}
        else:
            Pipe, _ = ref_pipeline.load_reference_pipeline_class()
            tok, enc, unet, vae = components(name)
            pipe = Pipe(vae=vae, text_encoder=enc, tokenizer=tok, unet=unet, scheduler=LC.LCMScheduler(**SD15),
                        safety_checker=None, feature_extractor=None, requires_safety_checker=False)
            img, mask, _ = MP.inputs()
            kw = dict(latents=start_latents()) if "strength" not in c else {}
            out = pipe(image=img, mask=mask, generator=g, output_type="latent", return_dict=False, **kw, **c)[0]
            emb = None
    return out, torch.randn(4, generator=g), emb


def prompts(tok, enc, c):
    def emb(p):
        ids = tok(p, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
        return enc(ids)[0]
    pos = emb(c["promptA"]) * c["tradoff"] + (1 - c["tradoff"]) * emb(c["promptB"])
    neg = emb(c["negative_promptA"]) * c["tradoff_nag"] + (1 - c["tradoff_nag"]) * emb(c["negative_promptB"])
    pe = torch.cat([neg.repeat(NB, 1, 1), pos.repeat(NB, 1, 1)])
    peU = None
    if "promptU" in c:
        peU = torch.cat([emb(c["negative_promptU"]).repeat(NB, 1, 1), emb(c["promptU"]).repeat(NB, 1, 1)])
    return pe, peU


def oracle_run(name):
    """The same call through oracle/loops.py with the restated scheduler -> (final latents, the generator's next draw)."""
    from oracle import loops as OL
    c = CALLS[name]
    g = torch.Generator().manual_seed(SEED)
    with torch.no_grad():
        if name == "v2":
            tok, enc, unet, bn, vae = components(name)
            img, mask3, _ = MP.inputs_v2()
            pe, peU = prompts(tok, enc, c)
            torch.manual_seed(9)
            rep = torch.cat([img.repeat(NB, 1, 1, 1)] * 2)              # prepare_image: per image, then the CFG twin
            cl = vae.encode(rep).latent_dist.sample() * vae.config.scaling_factor
            keep = (torch.cat([mask3.repeat(NB, 1, 1, 1)] * 2).sum(1)[:, None] < 0).float()
            cond = torch.cat([cl, torch.nn.functional.interpolate(keep, size=cl.shape[-2:])], 1)
            sch = LC.LCMScheduler(generator=g)                          # (loop_v2 hands no generator to `step`)
            out = OL.loop_v2(unet, bn, sch, start_latents(), cond, pe, peU, c["num_inference_steps"], c["guidance_scale"],
                             c["brushnet_conditioning_scale"])
        else:
            tok, enc, unet, vae = components(name)
            img, mask, _ = MP.inputs()
            pe, _ = prompts(tok, enc, c)
            sch = LC.LCMScheduler()
            sch.set_timesteps(c["num_inference_steps"])
            t_start = 0
            if "strength" in c:
                t_start = c["num_inference_steps"] - int(c["num_inference_steps"] * c["strength"])
                il = vae.encode(img).latent_dist.sample(g) * vae.config.scaling_factor
                noise = torch.randn(NB, 4, 16, 16, generator=g)
                lat = sch.add_noise(il, noise, sch.timesteps[t_start:t_start + 1].repeat(NB))
            else:
                lat = start_latents()
            mil = (vae.encode(img * (mask < 0.5)).latent_dist.sample(g) * vae.config.scaling_factor).repeat(NB, 1, 1, 1)
            m = torch.nn.functional.interpolate(mask, size=(16, 16)).repeat(NB, 1, 1, 1)
            out = OL.loop_v1(unet, sch, lat, torch.cat([m] * 2), torch.cat([mil] * 2), pe, c["num_inference_steps"],
                             c["guidance_scale"], t_start=t_start, generator=g)
    return out, torch.randn(4, generator=g)


def main():
    gold = {}
    for name in CALLS:
        out, nxt, emb = ref_run(name)
        gold[name] = dict(latents=out, next_draw=nxt)
        if emb is not None:
            gold["w_embedding"] = emb
        o, n2 = oracle_run(name)
        print(name, tuple(out.shape), "max|ref|", float(out.abs().max()), "oracle loop max err", float((o - out).abs().max()),
              "next draw equal", bool(torch.equal(nxt, n2)))
    path = os.path.join(HERE, "ref_lcm.pt")
    torch.save(gold, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
