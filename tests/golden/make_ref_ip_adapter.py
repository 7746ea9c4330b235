#!/usr/bin/env python
"""Generate tests/golden/ref_ip_adapter.pt (data only; run where the reference sources are): what the REFERENCE'S OWN
`StableDiffusionPowerPaintBrushNetPipeline.__call__` produces with IP-Adapter image prompts.

Through oracle/ref_pipeline.py (unchanged) the reference's `__call__` -- its `check_inputs`, `encode_image`,
`prepare_ip_adapter_image_embeds`, the `added_cond_kwargs` plumbing to the UNet and not to BrushNet -- runs on the reduced
SD-1.5 nets of make_ref_wiring.oracle_models() (components of make_ref_lcm): 16x16 latents, batch 2 (num_images_per_prompt),
guidance 7.5, 4 DPM-Solver++ steps, a CPU generator seeded 5.  The frozen ref_shim gives the reference's fork UNet no attention
processors to swap, so the UNet component is the ORACLE UNet with the restated IPAttention in every attn2 and the restated
multi-adapter projection in front (tests/ip_adapter_cases.IPUNet); the projection layers are checked here against the
reference's own `ImageProjection` (powerpaint/utils/utils.py:533-553, lifted by AST), and the name `ImageProjection` the
reference's `prepare_ip_adapter_image_embeds` tests its layers against is bound to the restated class.
Cases (ip_adapter_cases.CASES): `one` -- one adapter, precomputed embeds, scale 1; `two` -- two adapters, scales 0.7 / 0.4, the
second with two images per prompt (8 tokens); `image` -- `ip_adapter_image` through a stand-in image encoder (negative
embeds = zeros); `one_b` -- case `one` with other embeds (the per-call-state test's second call).
Stored per case: the final latents, the adapter-free latents of the same call, the generator's next draw.  For every case the
adapter-free latents must FAIL the GPU loop gate against the adapter's (asserted here): a no-op implementation cannot pass.

`oracle_run(name)` is the same call through oracle/loops.py -- tests/test_ip_adapter.py checks it against the fixture."""
import ast
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import ip_adapter_cases as IC  # noqa: E402
import make_ref_lcm as ML  # noqa: E402
import make_ref_pipeline_call as MP  # noqa: E402
from oracle import schedulers as OS  # noqa: E402

NB = ML.NB
CALL = dict(MP.CALL_V2, num_inference_steps=4, num_images_per_prompt=NB)
NAMES = ("one", "two", "image", "one_b")
REF_UTILS = "/root/reference/powerpaint/utils/utils.py"


def base(name):
    return (name[:-2], 1) if name.endswith("_b") else (name, 0)


def scheduler():
    return OS.DPMSolverMultistepScheduler(**MP.DPM_SD15)


def reference_image_projection():
    import torch.nn as nn
    tree = ast.parse(open(REF_UTILS).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ImageProjection"][0]
    ns = dict(nn=nn, torch=torch)
    exec(compile(ast.Module(body=[cls], type_ignores=[]), REF_UTILS, "exec"), ns)
    return ns["ImageProjection"]


def check_projection(proj):
    RP = reference_image_projection()
    g = torch.Generator().manual_seed(3)
    for lay in proj.image_projection_layers:
        D = lay.image_embeds.in_features
        r = RP(D, IC.CTX, lay.num_image_text_embeds)
        r.load_state_dict(lay.state_dict())
        x = torch.randn(3, D, generator=g)
        assert torch.equal(r(x), lay(x)), "restated ImageProjection differs from the reference's"


def ref_run(name, with_adapter=True):
    from oracle import ref_pipeline
    from oracle import sd_modules as OM
    case, variant = base(name)
    c = IC.CASES[case]
    g = torch.Generator().manual_seed(IC.SEED)
    with torch.no_grad():
        Pipe = ref_pipeline.load_reference_brushnet_pipeline_class(OM.BrushNetModel)
        tok, enc, unet, bn, vae = ML.components("v2")
        sds = IC.case_adapters(unet, case)
        ipu = IC.IPUNet(unet, sds, c["scales"]).eval()
        check_projection(ipu.encoder_hid_proj)
        Pipe.prepare_ip_adapter_image_embeds.__globals__["ImageProjection"] = IC.ImageProjection
        if not with_adapter:
            proj = ipu.encoder_hid_proj
            ipu = IC.PlainTupleUNet(ML.components("v2")[2]).eval()
            ipu.encoder_hid_proj = proj               # (the pipeline's length check looks at it; the forward ignores the prompt)
        pipe = Pipe(vae=vae, text_encoder=enc, text_encoder_brushnet=enc, tokenizer=tok, unet=ipu, brushnet=bn,
                    scheduler=scheduler(), safety_checker=None, feature_extractor=None,
                    image_encoder=IC.TinyImageEncoder().eval() if c["encoder"] else None, requires_safety_checker=False)
        img, mask3, _ = MP.inputs_v2()
        torch.manual_seed(9)                            # the conditioning latents are sampled from the global RNG
        out = pipe(image=img, mask=mask3, latents=ML.start_latents(), generator=g, output_type="latent",
                   return_dict=False, **IC.case_prompt(case, variant), **CALL)[0]
    return out, torch.randn(4, generator=g)


def prepared_embeds(name):
    """What prepare_ip_adapter_image_embeds hands the UNet for this case: one [2 NB, n, D] tensor per adapter."""
    case, variant = base(name)
    p = IC.case_prompt(case, variant)
    if "ip_adapter_image" in p:
        with torch.no_grad():
            pos = IC.TinyImageEncoder().eval()(p["ip_adapter_image"]).image_embeds
        pos = torch.stack([pos] * NB, dim=0)
        return [torch.cat([torch.zeros_like(pos), pos])]
    out = []
    for e in p["ip_adapter_image_embeds"]:
        neg, pos = e.chunk(2)
        out.append(torch.cat([neg.repeat(NB, 1, 1), pos.repeat(NB, 1, 1)]))
    return out


class _Bound(torch.nn.Module):
    """IPUNet with the call's image embeds bound (oracle/loops.py hands the UNet no added_cond_kwargs)."""

    def __init__(self, ipu, embeds):
        super().__init__()
        self.inner, self.embeds, self.config = ipu, embeds, ipu.config

    def forward(self, sample, timestep, encoder_hidden_states, **kw):
        return self.inner(sample, timestep, encoder_hidden_states, added_cond_kwargs={"image_embeds": self.embeds}, **kw)


def oracle_run(name):
    """The same call through oracle/loops.py -> (final latents, the generator's next draw)."""
    from oracle import loops as OL
    case, _ = base(name)
    c = IC.CASES[case]
    g = torch.Generator().manual_seed(IC.SEED)
    with torch.no_grad():
        tok, enc, unet, bn, vae = ML.components("v2")
        ipu = IC.IPUNet(unet, IC.case_adapters(unet, case), c["scales"]).eval()
        img, mask3, _ = MP.inputs_v2()
        pe, peU = ML.prompts(tok, enc, CALL)
        torch.manual_seed(9)
        rep = torch.cat([img.repeat(NB, 1, 1, 1)] * 2)
        cl = vae.encode(rep).latent_dist.sample() * vae.config.scaling_factor
        keep = (torch.cat([mask3.repeat(NB, 1, 1, 1)] * 2).sum(1)[:, None] < 0).float()
        cond = torch.cat([cl, torch.nn.functional.interpolate(keep, size=cl.shape[-2:])], 1)
        out = OL.loop_v2(_Bound(ipu, prepared_embeds(name)), bn, scheduler(), ML.start_latents(), cond, pe, peU,
                         CALL["num_inference_steps"], CALL["guidance_scale"], CALL["brushnet_conditioning_scale"])
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
    path = os.path.join(HERE, "ref_ip_adapter.pt")
    torch.save(gold, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
