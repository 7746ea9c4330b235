#!/usr/bin/env python
"""Generate tests/golden/ref_ip_adapter_plus.pt (data only; run where the reference sources are): what the REFERENCE'S OWN
`StableDiffusionPowerPaintBrushNetPipeline.__call__` produces with IP-Adapter Plus image prompts.

The call, the reduced nets and the geometry are make_ref_ip_adapter's (16x16 latents, batch 2, guidance 7.5, 4 DPM-Solver++
steps, a CPU generator seeded 5), through oracle/ref_pipeline.py (unchanged).  What runs of the reference: its `check_inputs`,
`encode_image` -- for case `plus_image` the `output_hidden_states` branch: `hidden_states[-2]` of the image and of
`torch.zeros_like(image)` -- `prepare_ip_adapter_image_embeds`, which picks that branch because the layer is no
`ImageProjection`, and the `added_cond_kwargs` plumbing to the UNet.  What is restated: the UNet component is the oracle UNet
with the restated IPAttention in every attn2 (tests/ip_adapter_cases.py) and, per adapter, the restated Resampler (Plus) or
ImageProjection (base) in front (tests/ip_plus_cases.PlusIPUNet) -- the reference imports `IPAdapterPlusImageProjection` from
diffusers and carries no copy of it, so there is nothing of its own to check the Resampler against.
Cases (ip_plus_cases.CASES): `plus` -- one Plus adapter, precomputed [2, 1, 10, 32] embeds; `plus_image` -- `ip_adapter_image`
through a stand-in encoder with `.hidden_states`; `mixed` -- a base adapter at 0.7 and a Plus adapter at 0.4, the Plus one with
two images per prompt (32 tokens); `plus_b` -- case `plus` with other embeds (the per-call-state test's second call).
Stored per case: the final latents, the adapter-free latents of the same call, the generator's next draw; for `plus_image` also
the latents of the call whose negative hidden states are ZEROS (through the oracle loop) and their distance from the truth.
For every case the adapter-free latents must FAIL the GPU loop gate against the adapter's (asserted here).

`oracle_run(name)` is the same call through oracle/loops.py -- tests/test_ip_adapter_plus.py checks it against the fixture."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import ip_adapter_cases as IC  # noqa: E402
import ip_plus_cases as PC  # noqa: E402
import make_ref_ip_adapter as MB  # noqa: E402
import make_ref_lcm as ML  # noqa: E402
import make_ref_pipeline_call as MP  # noqa: E402

NB = MB.NB
CALL = MB.CALL
NAMES = ("plus", "plus_image", "mixed", "plus_b")
base = MB.base


def check_base_layers(proj):
    """The base layers of a mixed list against the reference's own ImageProjection (make_ref_ip_adapter.check_projection)."""
    keep = [m for m in proj.image_projection_layers if isinstance(m, IC.ImageProjection)]
    if keep:
        MB.check_projection(IC.MultiProjection(keep))


def ref_run(name, with_adapter=True):
    from oracle import ref_pipeline
    from oracle import sd_modules as OM
    case, variant = base(name)
    c = PC.CASES[case]
    g = torch.Generator().manual_seed(IC.SEED)
    with torch.no_grad():
        Pipe = ref_pipeline.load_reference_brushnet_pipeline_class(OM.BrushNetModel)
        tok, enc, unet, bn, vae = ML.components("v2")
        ipu = PC.PlusIPUNet(unet, PC.case_adapters(unet, case), c["scales"]).eval()
        check_base_layers(ipu.encoder_hid_proj)
        Pipe.prepare_ip_adapter_image_embeds.__globals__["ImageProjection"] = IC.ImageProjection
        if not with_adapter:
            proj = ipu.encoder_hid_proj
            ipu = IC.PlainTupleUNet(ML.components("v2")[2]).eval()
            ipu.encoder_hid_proj = proj               # (the pipeline's length check looks at it; the forward ignores the prompt)
        pipe = Pipe(vae=vae, text_encoder=enc, text_encoder_brushnet=enc, tokenizer=tok, unet=ipu, brushnet=bn,
                    scheduler=MB.scheduler(), safety_checker=None, feature_extractor=None,
                    image_encoder=PC.HiddenStateEncoder().eval() if c["encoder"] else None, requires_safety_checker=False)
        img, mask3, _ = MP.inputs_v2()
        torch.manual_seed(9)                            # the conditioning latents are sampled from the global RNG
        out = pipe(image=img, mask=mask3, latents=ML.start_latents(), generator=g, output_type="latent",
                   return_dict=False, **PC.case_prompt(case, variant), **CALL)[0]
    return out, torch.randn(4, generator=g)


def prepared_embeds(name, zero_negative=False):
    """What prepare_ip_adapter_image_embeds hands the UNet for this case: per adapter [2 NB, n, D] or [2 NB, n, S, E]."""
    case, variant = base(name)
    p = PC.case_prompt(case, variant)
    if "ip_adapter_image" in p:
        img = p["ip_adapter_image"]
        with torch.no_grad():
            e = PC.HiddenStateEncoder().eval()
            pos = e(img, output_hidden_states=True).hidden_states[-2]
            neg = e(torch.zeros_like(img), output_hidden_states=True).hidden_states[-2]
        if zero_negative:
            neg = torch.zeros_like(pos)
        return [torch.cat([torch.stack([neg] * NB, dim=0), torch.stack([pos] * NB, dim=0)])]
    out = []
    for e in p["ip_adapter_image_embeds"]:
        neg, pos = e.chunk(2)
        ones = [1] * (e.dim() - 1)
        out.append(torch.cat([neg.repeat(NB, *ones), pos.repeat(NB, *ones)]))
    return out


def oracle_run(name, zero_negative=False):
    """The same call through oracle/loops.py -> (final latents, the generator's next draw)."""
    from oracle import loops as OL
    case, _ = base(name)
    c = PC.CASES[case]
    g = torch.Generator().manual_seed(IC.SEED)
    with torch.no_grad():
        tok, enc, unet, bn, vae = ML.components("v2")
        ipu = PC.PlusIPUNet(unet, PC.case_adapters(unet, case), c["scales"]).eval()
        img, mask3, _ = MP.inputs_v2()
        pe, peU = ML.prompts(tok, enc, CALL)
        torch.manual_seed(9)
        rep = torch.cat([img.repeat(NB, 1, 1, 1)] * 2)
        cl = vae.encode(rep).latent_dist.sample() * vae.config.scaling_factor
        keep = (torch.cat([mask3.repeat(NB, 1, 1, 1)] * 2).sum(1)[:, None] < 0).float()
        cond = torch.cat([cl, torch.nn.functional.interpolate(keep, size=cl.shape[-2:])], 1)
        out = OL.loop_v2(MB._Bound(ipu, prepared_embeds(name, zero_negative)), bn, MB.scheduler(), ML.start_latents(), cond, pe,
                         peU, CALL["num_inference_steps"], CALL["guidance_scale"], CALL["brushnet_conditioning_scale"])
    return out, torch.randn(4, generator=g)


def main():
    gold = {}
    for name in NAMES:
        out, nxt = ref_run(name)
        plain, _ = ref_run(name, with_adapter=False)
        cos, err, ok = IC.loop_gate(plain, out)
        print(f"{name}: max|ref| {float(out.abs().max()):.4g}; adapter-free latents against it: cos {cos:.5f} "
              f"max err {err:.4g} of max|ref| (gate: cos >= {IC.LOOP_COS}, err <= {IC.LOOP_ERR})")
        assert not ok, f"{name}: the adapter-free latents pass the loop gate -- the fixture would not notice a missing adapter"
        o, n2 = oracle_run(name)
        print(f"   oracle loop max err {float((o - out).abs().max()):.3g}; next draw equal {bool(torch.equal(nxt, n2))}")
        gold[name] = dict(latents=out, plain=plain, next_draw=nxt, cos_plain=cos, err_plain=err)
        if PC.CASES[base(name)[0]]["encoder"]:
            z, _ = oracle_run(name, zero_negative=True)
            gold[name]["latents_zero_negative"] = z
            gold[name]["err_zero_negative"] = float((z - out).abs().max())
            print(f"   zeros as the negative hidden states: max err {gold[name]['err_zero_negative']:.4g}; passes the loop gate: "
                  f"{IC.loop_gate(z, out)[2]}")
    path = os.path.join(HERE, "ref_ip_adapter_plus.pt")
    torch.save(gold, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
