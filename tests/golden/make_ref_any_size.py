#!/usr/bin/env python
"""Generate tests/golden/ref_any_size.pt (data only; run where the reference sources are): what the REFERENCE'S OWN networks
and pipeline `__call__`s produce at latent sizes that are no multiple of 2^(levels - 1) = 8.

The reference UNet and BrushNet set `forward_upsample_size` there and hand every up block but the last
`upsample_size = down_block_res_samples[-1].shape[2:]` (unet_2d_condition.py:1120-1126,1311-1312, BrushNet_CA.py:874): the
upsampler becomes F.interpolate(size=...).  The oracle's UNet does not pass `upsample_size` and cannot run these sizes, so
every UNet / BrushNet here is the reference's own class, imported unmodified through oracle/ref_shim.py; the oracle's
ControlNetModel (down path only), VAE and schedulers run them as they are.  Nets, seeds and bf16 rounding are those of
make_ref_wiring.oracle_models(): block widths 320/320/640/640, one layer per block.

  (a) nets[HxW].eps9 / eps4_plain       the reference UNet with in_channels = 9, and with in_channels = 4 on its own
  (b) nets[HxW].res_* / eps4_brush      reference BrushNet `from_unet` with randomised zero convs -> all 8 + 1 + 11 residual
                                        shapes and summaries, and epsilon of the reference UNet fed with them
      nets[HxW].eps9_freeu              the 9-channel UNet with FreeU enabled (freeu_cases.FREEU_FULL): the reference's up blocks
                                        call the restated filter of tests/freeu_cases.py, as in make_ref_freeu.py
  (d) nets[HxW].ctrl_* / eps9_ctrl      oracle ControlNetModel -> 8 + 1 residual summaries -> the reference 9-channel UNet
  (c) calls.v1_ddim / v1_dpm            the reference's own v1 `__call__` (oracle/ref_pipeline.py, unchanged) around the
      calls.v2_ddim / v2_dpm            reference UNet; its BrushNet `__call__` around the reference BrushNet and UNet
  (d) calls.cn_ddim                     its ControlNet `__call__`: oracle ControlNetModel into the reference UNet
      image 104x80 (13x10 latents), 4 steps, guidance 7.5, batch 2 (num_images_per_prompt); final latents.
Latent sizes: 13x10 (13 -> 7 -> 4 -> 2 and 10 -> 5 -> 3 -> 2: cropped and exact upsamples on both axes), 9x11, 10x12 (even,
no multiple of 8).  Full final tensors; (mean, std, max-abs, first 32 values) for the residual lists, as ref_wiring.pt.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import freeu_cases as FC  # noqa: E402
import make_ref_pipeline_call as MP  # noqa: E402
import make_ref_wiring as MW  # noqa: E402
from oracle import schedulers as OS, sd_modules as OM  # noqa: E402

SIZES = ((13, 10), (9, 11), (10, 12))
CHAINS = {(13, 10): [(13, 10), (7, 5), (4, 3), (2, 2)], (9, 11): [(9, 11), (5, 6), (3, 3), (2, 2)],
          (10, 12): [(10, 12), (5, 6), (3, 3), (2, 2)]}
CFG = {k: v for k, v in MW.OCFG.items() if k != "attention_head_dim"}      # constructor arguments of the HIP models
CN_CFG = {k: v for k, v in MW.OCFG.items() if k != "up_block_types"}
CN_HIP_CFG = {k: v for k, v in CFG.items() if k != "up_block_types"}
HEIGHT, WIDTH, NB, SEED, STEPS = 104, 80, 2, 5, 4
DPM_SD15 = MP.DPM_SD15
CALLS = dict(v1=dict(MP.CALL, height=HEIGHT, width=WIDTH, num_inference_steps=STEPS, num_images_per_prompt=NB),
             v2=dict(MP.CALL_V2, height=HEIGHT, width=WIDTH, num_inference_steps=STEPS, num_images_per_prompt=NB),
             cn=dict(MP.CALL_CN, height=HEIGHT, width=WIDTH, num_inference_steps=STEPS, num_images_per_prompt=NB))
CASES = ("v1_ddim", "v1_dpm", "v2_ddim", "v2_dpm", "cn_ddim")


def key(hw):
    return f"{hw[0]}x{hw[1]}"


def net_inputs(hw):
    h, w = hw
    g = torch.Generator("cpu").manual_seed(1000 * h + w)
    return dict(x9=torch.randn(2, 9, h, w, generator=g), x4=torch.randn(2, 4, h, w, generator=g),
                ehs=torch.randn(2, 77, 768, generator=g), ehs_b=torch.randn(2, 77, 768, generator=g),
                cond=torch.randn(2, 5, h, w, generator=g), ctrl=torch.rand(2, 3, 8 * h, 8 * w, generator=g),
                t=torch.tensor(681), scale=0.75, cn_scale=0.5)


def brushnet_of(u4):
    """The oracle BrushNet whose state dict the reference BrushNet (and the HIP one) load: from_unet + zero convs, seed 11."""
    return OM.randomize_zero_convs(OM.BrushNetModel.from_unet(u4), seed=11).eval()


def controlnet():
    torch.manual_seed(20240103)
    return OM.randomize_zero_convs(MW.bf16_(OM.ControlNetModel(in_channels=4, **CN_CFG)), seed=12).eval()


def call_inputs():
    g = torch.Generator().manual_seed(44)
    img = torch.rand(1, 3, HEIGHT, WIDTH, generator=g) * 2 - 1
    mask = torch.zeros(1, 1, HEIGHT, WIDTH)
    mask[:, :, 22:85, 14:61] = 1.0
    lat = torch.randn(NB, 4, HEIGHT // 8, WIDTH // 8, generator=g)
    ctrl = torch.rand(1, 3, HEIGHT, WIDTH, generator=g)
    return img, mask, lat, ctrl


def scheduler(case, S=OS):
    return S.DDIMScheduler() if case.endswith("ddim") else S.DPMSolverMultistepScheduler(**DPM_SD15)


def reference_nets():
    """(reference 9-channel UNet, reference 4-channel UNet, reference BrushNet, the class of the latter) carrying the weights
    of make_ref_wiring.oracle_models()."""
    from oracle import ref_shim
    RU, RB = ref_shim.load_reference_models()
    sys.modules["ref_powerpaint_models.unet_2d_blocks"].apply_freeu = FC.apply_freeu      # (the shim's stand-in raises)
    u9, u4 = MW.oracle_models()
    # (sample_size: a config entry the pipelines' constructors compare against 64; no part of the arithmetic)
    r9 = RU(in_channels=9, sample_size=64, **MW.CFG).eval()
    r9.load_state_dict(u9.state_dict())
    r4 = RU(in_channels=4, sample_size=64, **MW.CFG).eval()
    r4.load_state_dict(u4.state_dict())
    rb = RB.from_unet(r4).eval()
    rb.load_state_dict(brushnet_of(u4).state_dict())
    return r9, r4, rb, RB


def nets_at(hw, r9, r4, rb, cn):
    inp = net_inputs(hw)
    out = {}
    out["eps9"] = r9(inp["x9"], inp["t"], inp["ehs"], return_dict=False)[0]
    r9.enable_freeu(**FC.FREEU_FULL)
    out["eps9_freeu"] = r9(inp["x9"], inp["t"], inp["ehs"], return_dict=False)[0]
    r9.disable_freeu()
    assert not FC.close_gate(out["eps9"], out["eps9_freeu"])[2], "the plain output passes the gate: FreeU would go unnoticed"
    out["eps4_plain"] = r4(inp["x4"], inp["t"], inp["ehs"], return_dict=False)[0]
    dn, md, up = rb(inp["x4"], inp["t"], encoder_hidden_states=inp["ehs_b"], brushnet_cond=inp["cond"],
                    conditioning_scale=inp["scale"], return_dict=False)
    res = list(dn) + [md] + list(up)
    out["n_down"], out["n_up"] = len(dn), len(up)
    out["res_shapes"] = [tuple(t.shape) for t in res]
    out["res_summary"] = torch.stack([MW.summary(t) for t in res])
    out["eps4_brush"] = r4(inp["x4"], inp["t"], inp["ehs"], down_block_add_samples=list(dn), mid_block_add_sample=md,
                           up_block_add_samples=list(up), return_dict=False)[0]
    cd, cm = cn(inp["x9"][:, :4], inp["t"], inp["ehs"], inp["ctrl"], conditioning_scale=inp["cn_scale"], return_dict=False)
    out["ctrl_shapes"] = [tuple(t.shape) for t in list(cd) + [cm]]
    out["ctrl_summary"] = torch.stack([MW.summary(t) for t in list(cd) + [cm]])
    out["eps9_ctrl"] = r9(inp["x9"], inp["t"], inp["ehs"], down_block_additional_residuals=list(cd),
                          mid_block_additional_residual=cm, return_dict=False)[0]
    return out


def call(case, r9, r4, rb, RB, cn):
    from oracle import ref_pipeline
    tok, enc, _, vae = MP.components()
    img, mask, lat, ctrl = call_inputs()
    g = torch.Generator().manual_seed(SEED)
    common = dict(safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    if case.startswith("v1"):
        Pipe, _ = ref_pipeline.load_reference_pipeline_class()
        pipe = Pipe(vae=vae, text_encoder=enc, tokenizer=tok, unet=r9, scheduler=scheduler(case), **common)
        return pipe(image=img, mask=mask, latents=lat.clone(), generator=g, output_type="latent", return_dict=False,
                    **CALLS["v1"])[0]
    if case.startswith("v2"):
        Pipe = ref_pipeline.load_reference_brushnet_pipeline_class(RB)
        pipe = Pipe(vae=vae, text_encoder=enc, text_encoder_brushnet=enc, tokenizer=tok, unet=r4, brushnet=rb,
                    scheduler=scheduler(case), **common)
        torch.manual_seed(9)                                # the conditioning latents are sampled from the global RNG
        return pipe(image=img * (mask < 0.5), mask=(mask * 2 - 1).repeat(1, 3, 1, 1), latents=lat.clone(), generator=g,
                    output_type="latent", return_dict=False, **CALLS["v2"])[0]
    Pipe = ref_pipeline.load_reference_controlnet_pipeline_class(OM.ControlNetModel)
    pipe = Pipe(vae=vae, text_encoder=enc, tokenizer=tok, unet=r9, controlnet=cn, scheduler=scheduler(case), **common)
    return pipe(image=img, mask=mask, control_image=ctrl, latents=lat.clone(), generator=g, output_type="latent",
                return_dict=False, **CALLS["cn"])[0]


def generate():
    r9, r4, rb, RB = reference_nets()
    cn = controlnet()
    gold = {"nets": {}, "calls": {}}
    with torch.no_grad():
        for hw in SIZES:
            gold["nets"][key(hw)] = nets_at(hw, r9, r4, rb, cn)
        for case in CASES:
            gold["calls"][case] = call(case, r9, r4, rb, RB, cn)
    return gold


def main(path=None):
    gold = generate()
    for k, v in gold["nets"].items():
        print(k, "max|eps9|", float(v["eps9"].abs().max()), "max|eps4_brush|", float(v["eps4_brush"].abs().max()),
              "max|eps9_ctrl|", float(v["eps9_ctrl"].abs().max()), v["n_down"], "+ 1 +", v["n_up"], "residuals")
    for k, v in gold["calls"].items():
        print(k, tuple(v.shape), "max|latents|", float(v.abs().max()))
    path = path or os.path.join(HERE, "ref_any_size.pt")
    torch.save(gold, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)      # (an output path: tests/test_any_size.py re-runs the generator)
