#!/usr/bin/env python
"""Generate tests/golden/ref_ip_adapter_masks.pt (data only; run where the reference sources are): what the REFERENCE'S OWN
`StableDiffusionPowerPaintBrushNetPipeline.__call__` produces with IP-Adapter image prompts confined by `ip_adapter_masks`.

As make_ref_ip_adapter.py: through oracle/ref_pipeline.py (unchanged) the reference's `__call__` runs on the reduced SD-1.5
nets (16x16 latents, batch 2, guidance 7.5, 4 DPM-Solver++ steps, a CPU generator seeded 5), and it is the reference's own
plumbing that carries `cross_attention_kwargs={"ip_adapter_masks": m}` to the UNet and to nothing else
(pipeline_PowerPaint_Brushnet_CA.py:1430-1441).  The UNet component is tests/ip_mask_cases.MaskedIPUNet: the oracle UNet with the
restated IPAdapterAttnProcessor2_0 INCLUDING its mask branch, which takes the masks out of `cross_attention_kwargs`.
Cases (ip_mask_cases.CASES / case_masks; adapters, scales and embeds of ip_adapter_cases): `one` -- one adapter, a rectangle;
`two` -- two adapters, scales 0.7 / 0.4, the left and the right half; `one_b` -- case `one` with another rectangle (the second
call of the graph re-use test).
Stored per case: the final latents, the latents of the same call WITHOUT masks (`unmasked`), the generator's next draw.  For
every case the unmasked latents must FAIL the GPU loop gate against the masked ones (asserted here): an implementation that
drops the masks cannot pass.

`oracle_run(name)` is the same call through oracle/loops.py -- tests/test_ip_adapter_masks.py checks it against the fixture."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import ip_adapter_cases as IC  # noqa: E402
import ip_mask_cases as MC  # noqa: E402
import make_ref_ip_adapter as M  # noqa: E402
import make_ref_lcm as ML  # noqa: E402
import make_ref_pipeline_call as MP  # noqa: E402

NB, CALL = M.NB, M.CALL
NAMES = tuple(MC.CASES)


def ref_run(name, masked=True):
    from oracle import ref_pipeline
    from oracle import sd_modules as OM
    case, _ = MC.CASES[name]
    c = IC.CASES[case]
    g = torch.Generator().manual_seed(IC.SEED)
    with torch.no_grad():
        Pipe = ref_pipeline.load_reference_brushnet_pipeline_class(OM.BrushNetModel)
        tok, enc, unet, bn, vae = ML.components("v2")
        ipu = MC.MaskedIPUNet(unet, IC.case_adapters(unet, case), c["scales"]).eval()
        Pipe.prepare_ip_adapter_image_embeds.__globals__["ImageProjection"] = IC.ImageProjection
        pipe = Pipe(vae=vae, text_encoder=enc, text_encoder_brushnet=enc, tokenizer=tok, unet=ipu, brushnet=bn,
                    scheduler=M.scheduler(), safety_checker=None, feature_extractor=None, image_encoder=None,
                    requires_safety_checker=False)
        img, mask3, _ = MP.inputs_v2()
        assert tuple(img.shape[-2:]) == MC.MASK_HW
        kw = dict(cross_attention_kwargs={"ip_adapter_masks": MC.case_masks(name)}) if masked else {}
        torch.manual_seed(9)                            # the conditioning latents are sampled from the global RNG
        out = pipe(image=img, mask=mask3, latents=ML.start_latents(), generator=g, output_type="latent",
                   return_dict=False, **IC.case_prompt(case, 0), **kw, **CALL)[0]
    return out, torch.randn(4, generator=g)


class _Bound(torch.nn.Module):
    """MaskedIPUNet with the call's image embeds and masks bound (oracle/loops.py hands the UNet neither)."""

    def __init__(self, ipu, embeds, masks):
        super().__init__()
        self.inner, self.embeds, self.masks, self.config = ipu, embeds, masks, ipu.config

    def forward(self, sample, timestep, encoder_hidden_states, **kw):
        return self.inner(sample, timestep, encoder_hidden_states, added_cond_kwargs={"image_embeds": self.embeds},
                          cross_attention_kwargs={"ip_adapter_masks": self.masks}, **kw)


def oracle_run(name):
    """The same call through oracle/loops.py -> (final latents, the generator's next draw)."""
    from oracle import loops as OL
    case, _ = MC.CASES[name]
    c = IC.CASES[case]
    g = torch.Generator().manual_seed(IC.SEED)
    with torch.no_grad():
        tok, enc, unet, bn, vae = ML.components("v2")
        ipu = MC.MaskedIPUNet(unet, IC.case_adapters(unet, case), c["scales"]).eval()
        img, mask3, _ = MP.inputs_v2()
        pe, peU = ML.prompts(tok, enc, CALL)
        torch.manual_seed(9)
        rep = torch.cat([img.repeat(NB, 1, 1, 1)] * 2)
        cl = vae.encode(rep).latent_dist.sample() * vae.config.scaling_factor
        keep = (torch.cat([mask3.repeat(NB, 1, 1, 1)] * 2).sum(1)[:, None] < 0).float()
        cond = torch.cat([cl, torch.nn.functional.interpolate(keep, size=cl.shape[-2:])], 1)
        out = OL.loop_v2(_Bound(ipu, M.prepared_embeds(case), MC.case_masks(name)), bn, M.scheduler(), ML.start_latents(), cond,
                         pe, peU, CALL["num_inference_steps"], CALL["guidance_scale"], CALL["brushnet_conditioning_scale"])
    return out, torch.randn(4, generator=g)


def main():
    gold = {}
    for name in NAMES:
        out, nxt = ref_run(name)
        plain, nxt_p = ref_run(name, masked=False)
        cos, err, ok = IC.loop_gate(plain, out)
        print(f"{name}: max|ref| {float(out.abs().max()):.4g}; unmasked latents against it: cos {cos:.5f} "
              f"max err {err:.4g} of max|ref| (gate: cos >= {IC.LOOP_COS}, err <= {IC.LOOP_ERR})")
        assert not ok, f"{name}: the unmasked latents pass the loop gate -- the fixture would not notice dropped masks"
        assert torch.equal(nxt, nxt_p)
        o, n2 = oracle_run(name)
        print(f"   oracle loop max err {float((o - out).abs().max()):.3g}; next draw equal {bool(torch.equal(nxt, n2))}")
        gold[name] = dict(latents=out, unmasked=plain, next_draw=nxt)
    cos, err, ok = IC.loop_gate(gold["one_b"]["latents"], gold["one"]["latents"])
    print(f"one_b against one: cos {cos:.5f} max err {err:.4g}")
    assert not ok, "one_b passes the gate against one: the graph re-use test would not notice stale weights"
    path = os.path.join(HERE, "ref_ip_adapter_masks.pt")
    torch.save(gold, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
