"""-m gpu: `guidance_rescale` through the fused loop and the three pipelines, against the CPU oracle loops of
tests/pag_cases.py with the rescale behind their guidance combine (tests/guidance_cases.py).

Inputs.  On a randomly initialised tiny net the prompt moves the output little: e_u ~ e_c, the guided prediction keeps the
conditional one's deviation and the rescale would hide inside the gate.  The negative prompt embeds of this file are therefore
scaled by NEG (the same tensors on both sides), which spreads e_c - e_u until the float64 loops with and without the rescale
differ by 13 x the gate's bound or more after three steps (checked on the CPU; at NEG = 4 three of the cases stay below 10 x; every
case asserts >= 10 x first, on the references alone).  Networks: `make_tiny` / `boosted` of tests/test_pag_gpu.py.  3 steps, 8 x 8 latents, one 6 x 10 case.
Gates: `close` of tests/test_models_gpu.py with its defaults (cosine >= 0.999, max-abs <= 3e-2 max(1, max|ref|)).
"""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
import guidance_cases as GC  # noqa: E402
import pag_cases as PC  # noqa: E402
from oracle import schedulers as OS  # noqa: E402
from powerpaint_amd import pag as PAGM  # noqa: E402
from powerpaint_amd import pipelines as PP  # noqa: E402
from powerpaint_amd import schedulers as PS  # noqa: E402
from test_models_gpu import DEV, close, gen, make_tiny  # noqa: E402
from test_pag_gpu import SD15, _brushnet_kw, _names, boosted  # noqa: E402

NEG = 6.0          # the negative prompt embeds' scale (module docstring)
PHI = 0.7
G = 7.5


def visible(ref_on, ref_off, what):
    """The condition on the references alone: the rescale moves the result by >= 10 x the gate's bound."""
    bound = 3e-2 * max(1.0, float(ref_on.abs().max()))
    moved = float((ref_on - ref_off).abs().max())
    print(f"[guidance_rescale] {what}: reference with - without the rescale {moved:.4f} = {moved / bound:.1f} x the gate's bound")
    assert moved >= 10 * bound, f"{what}: the inputs do not make the rescale visible: choose others"


def scheduler_pair(name):
    import ksampler_cases as KC
    import lcm_cases as LC
    import sigma_cases as SC
    if name == "ddim":
        return PS.DDIMScheduler(), lambda: OS.DDIMScheduler()
    if name == "euler_a":
        return PS.EulerAncestralDiscreteScheduler(**SD15), lambda: SC.EulerAncestralDiscreteScheduler(**SD15)
    if name == "heun":
        return PS.HeunDiscreteScheduler(**SD15), lambda: KC.HeunDiscreteScheduler(**SD15)
    return PS.LCMScheduler(), lambda: LC.LCMScheduler()


# ------------------------------------------------------------------------------------------------ the BrushNet pipeline
@functools.lru_cache(maxsize=None)
def _brushnet_nets():
    return make_tiny("brushnet"), boosted("unet", seed=1, in_channels=4)


def brushnet_inputs(B, h, w, spread=False):
    """-> (lat, cl, pe, peU): [uncond, cond] pairs, the negative halves scaled by NEG.  spread: the second sample's prompts
    are the first one's scaled by 3 and negated -- two samples with very different conditional predictions."""
    lat = gen(B, 4, h, w, seed=0)
    mask = torch.zeros(B, 1, h, w)
    mask[:, :, 2:h - 2, 2:w - 2] = 1.0
    cl = torch.cat([gen(B, 4, h, w, seed=1, scale=0.5), mask], 1)
    pe, peU = gen(2 * B, 77, 768, seed=2), gen(2 * B, 77, 768, seed=3)
    if spread:
        for p in (pe, peU):
            p[B + 1] = -3.0 * p[B]
    pe[:B] *= NEG
    peU[:B] *= NEG
    return lat, cl, pe, peU


def brushnet_refs(name, B, h, w, spread=False, pag_names=(), pag_scale=0.0):
    """-> the float64-rescaled oracle loop with PHI and with 0 (nothing here needs a device)."""
    (ob, _), (ou, _) = _brushnet_nets()
    lat, cl, pe, peU = brushnet_inputs(B, h, w, spread)
    _, ref_sch = scheduler_pair(name)
    run = lambda phi: GC.loop_v2_rescale(ou, ob, ref_sch(), lat, torch.cat([cl] * 2), pe, peU, 3, G, phi,      # noqa: E731
                                         pag_names=pag_names, pag_scale=pag_scale, generator=torch.Generator().manual_seed(8))
    return run(PHI), run(0.0)


def _brushnet_pipe(sch, **kw):
    (_, hb), (_, hu) = _brushnet_nets()
    return PP.StableDiffusionPowerPaintBrushNetPipeline(unet=hu, brushnet=hb, scheduler=sch, **kw), hu


def _check_tail(loop, step_prefix="cfg_"):
    names = _names(loop.program.calls)
    assert names.count("cfg_rescale") == 1 and "pag_combine" not in names
    at = names.index("cfg_rescale") + 1
    assert names[at].startswith(step_prefix) and loop.program.calls[at][1][1] == 0, "the step launch runs with cfg = 0"


@pytest.mark.parametrize("name,B,h,w,spread", [("ddim", 1, 8, 8, False), ("euler_a", 1, 8, 8, False), ("heun", 1, 8, 8, False),
                                               ("lcm", 1, 8, 8, False), ("ddim", 1, 6, 10, False), ("ddim", 2, 8, 8, True)],
                         ids=["ddim", "euler_a", "heun", "lcm", "ddim_6x10", "ddim_two_prompts"])
def test_brushnet_pipeline_against_the_oracle_loop(name, B, h, w, spread):
    what = f"guidance_rescale BrushNet pipeline, {name}, B={B} {h}x{w}"
    ref, ref0 = brushnet_refs(name, B, h, w, spread)
    visible(ref, ref0, what)
    sch, _ = scheduler_pair(name)
    pipe, _ = _brushnet_pipe(sch)
    lat, cl, pe, peU = brushnet_inputs(B, h, w, spread)
    kw = _brushnet_kw(B, lat, cl, pe, peU, True, guidance_rescale=PHI)
    assert pipe.use_graph
    out = pipe(generator=torch.Generator().manual_seed(8), **kw)[0].clone()
    _check_tail(pipe._loop)
    assert pipe._loop.rt.B == 2 * B
    pipe.use_graph = False
    eager = pipe(generator=torch.Generator().manual_seed(8), **kw)[0].clone()
    assert torch.equal(out, eager), "graph replay and eager replay differ"
    close(out, ref, what)


def test_with_pag_the_rescale_launch_replaces_pag_combine():
    (_, hb), _ = _brushnet_nets()
    _, hu = boosted("unet", seed=1, in_channels=4)          # (its own UNet: the layer selection stays in this test)
    pipe = PP.StableDiffusionPowerPaintBrushNetPipeline(unet=hu, brushnet=hb, scheduler=PS.DDIMScheduler(),
                                                        pag_applied_layers=["down", "mid"])
    sel = PAGM.attn1_names(hu.pag_layers())
    assert len(sel) == 2
    ref, ref0 = brushnet_refs("ddim", 1, 8, 8, pag_names=tuple(sel), pag_scale=3.0)
    visible(ref, ref0, "guidance_rescale + PAG")
    lat, cl, pe, peU = brushnet_inputs(1, 8, 8)
    out = pipe(**_brushnet_kw(1, lat, cl, pe, peU, True, pag_scale=3.0, guidance_rescale=PHI))[0]
    _check_tail(pipe._loop)
    names = _names(pipe._loop.program.calls)
    assert names.count("attn_identity_v") == 2 and pipe._loop.rt.B == 3
    assert pipe._loop.program.calls[names.index("cfg_rescale")][1][1] == 3
    close(out, ref, "guidance_rescale + PAG, BrushNet pipeline, DDIM")


def test_a_new_value_reaches_the_graph_without_a_recapture():
    pipe, _ = _brushnet_pipe(PS.DDIMScheduler())
    lat, cl, pe, peU = brushnet_inputs(1, 8, 8)
    kw = _brushnet_kw(1, lat, cl, pe, peU, True)
    never = pipe(**kw)[0].clone()
    never_names = _names(pipe._loop.program.calls)
    assert "cfg_rescale" not in never_names
    out7 = pipe(guidance_rescale=0.7, **kw)[0].clone()
    loop = pipe._loop
    g0, program0, cell = loop.graph, loop.program, loop._phi_cell
    assert g0 is not None and float(cell.item()) == float(torch.tensor(0.7, dtype=torch.float32))
    out3 = pipe(guidance_rescale=0.3, **kw)[0].clone()
    assert loop.graph is g0 and loop.program is program0 and loop._phi_cell is cell, "a new guidance_rescale re-captured the step"
    assert float(cell.item()) == float(torch.tensor(0.3, dtype=torch.float32)) and not torch.equal(out3, out7)
    ref7, ref0 = brushnet_refs("ddim", 1, 8, 8)
    close(out7, ref7, "guidance_rescale 0.7, then")
    again7 = pipe(guidance_rescale=0.7, **kw)[0]
    assert loop.graph is g0 and torch.equal(again7, out7)
    # off is off: 0.0 is the never-enabled program and output
    off = pipe(guidance_rescale=0.0, **kw)[0]
    assert _names(pipe._loop.program.calls) == never_names and torch.equal(off, never)
    close(off, ref0, "guidance_rescale 0.0")
    # without CFG the argument has no effect: the plain program, the plain output
    kw1 = _brushnet_kw(1, lat, cl, pe, peU, False)
    plain = pipe(**kw1)[0].clone()
    plain_names = _names(pipe._loop.program.calls)
    same = pipe(guidance_rescale=0.7, **kw1)[0]
    assert _names(pipe._loop.program.calls) == plain_names and "cfg_rescale" not in plain_names and torch.equal(same, plain)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="guidance_rescale"):
            pipe(guidance_rescale=bad, **kw)


# ------------------------------------------------------------------------------------------------ the other two pipelines
@functools.lru_cache(maxsize=None)
def _controlnet_nets():
    return make_tiny("controlnet"), make_tiny("controlnet", seed=5), boosted("unet", seed=1, in_channels=9)


def controlnet_inputs():
    B, hh = 1, 8
    lat, mask, mil = gen(B, 4, hh, hh, seed=0), torch.zeros(B, 1, hh, hh), gen(B, 4, hh, hh, seed=1, scale=0.5)
    mask[:, :, 2:6, 2:6] = 1.0
    pe = gen(2 * B, 77, 768, seed=2)
    pe[:B] *= NEG
    imgs = [torch.rand(B, 3, 8 * hh, 8 * hh, generator=torch.Generator().manual_seed(3 + i)) for i in range(2)]
    return lat, mask, mil, pe, imgs


def controlnet_refs(rows):
    (oc1, _), (oc2, _), (ou, _) = _controlnet_nets()
    lat, mask, mil, pe, imgs = controlnet_inputs()
    run = lambda phi: GC.loop_v1_rescale(                                                                      # noqa: E731
        ou, OS.DDIMScheduler(), lat, mask, mil, pe, 3, G, phi,
        controlnet=PC.TwoControlNets([oc1, oc2], [torch.cat([i] * 3) for i in imgs], rows))
    return run(PHI), run(0.0)


def test_controlnet_pipeline_two_nets_one_window_closing():
    (_, hc1), (_, hc2), (_, hu) = _controlnet_nets()
    lat, mask, mil, pe, imgs = controlnet_inputs()
    pipe = PP.StableDiffusionControlNetInpaintPipeline(unet=hu, controlnet=[hc1, hc2], scheduler=PS.DDIMScheduler())
    scales, starts, ends = [0.5, 0.8], [0.0, 0.0], [1.0, 0.4]
    rows = pipe.control_schedule(3, scales, starts, ends)
    assert [r[1] != 0.0 for r in rows] == [True, False, False]
    ref, ref0 = controlnet_refs(rows)
    visible(ref, ref0, "guidance_rescale ControlNet pipeline")
    out = pipe(prompt_embeds=pe[1:].to(DEV), negative_prompt_embeds=pe[:1].to(DEV), height=64, width=64,
               control_image=[i.to(DEV) for i in imgs], controlnet_conditioning_scale=scales, control_guidance_start=starts,
               control_guidance_end=ends, num_inference_steps=3, guidance_scale=G, latents=lat.to(DEV),
               mask_latents=mask.to(DEV), masked_image_latents=mil.to(DEV), output_type="latent", return_dict=False,
               guidance_rescale=PHI)[0]
    for ent in pipe._loop._sets.values():                 # (one program per set of active nets: each has the launch)
        names = _names(ent.program[False].calls)
        assert names.count("cfg_rescale") == 1 and ent.program[False].calls[names.index("cfg_rescale") + 1][1][1] == 0
    assert len(pipe._loop._sets) == 2
    close(out, ref, "guidance_rescale ControlNet pipeline, two nets, one window closing")


def v1_blend_refs():
    """-> (ref with PHI, ref with 0, everything the pipeline call takes); the oracle side needs no device."""
    import make_ref_pipeline_call as M
    _, _, unet, vae = M.components_4ch()
    img, mask, _ = M.inputs()
    pe = gen(2, 77, 768, seed=2)
    pe[:1] *= NEG
    m = torch.nn.functional.interpolate(mask, size=(16, 16))
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        il = vae.encode(img).latent_dist.sample(g) * vae.config.scaling_factor
        noise = torch.randn(1, 4, 16, 16, generator=g)
    run = lambda phi: GC.loop_v1_rescale(unet, OS.DDIMScheduler(), noise, m, None, pe, 3, G, phi, image_latents=il,    # noqa: E731
                                         noise=noise)
    return run(PHI), run(0.0), (M, unet, vae, img, mask, pe)


def test_v1_pipeline_with_the_4_channel_blend_and_a_duck_typed_scheduler():
    from powerpaint_amd import models as PM
    ref, ref0, (M, unet, vae, img, mask, pe) = v1_blend_refs()
    visible(ref, ref0, "guidance_rescale v1 pipeline, 4-channel blend")
    hu = PM.UNet2DConditionModel(in_channels=4, device=DEV, **M.TINY).load_state_dict(unet.state_dict())
    hv = PM.AutoencoderKL(device=DEV, **M.VAE_CFG).load_state_dict(vae.state_dict())
    kw = dict(prompt_embeds=pe[1:].to(DEV), negative_prompt_embeds=pe[:1].to(DEV), image=img, mask=mask, height=128, width=128,
              num_inference_steps=3, guidance_scale=G, output_type="latent", return_dict=False, guidance_rescale=PHI)
    pipe = PP.StableDiffusionInpaintPipeline(vae=hv, unet=hu, scheduler=PS.DDIMScheduler())
    out = pipe(generator=torch.Generator().manual_seed(5), **kw)[0]
    assert _names(pipe._loop.program.calls)[-4:] == ["cfg_rescale", "cfg_sched_step", "latent_blend", "step_advance"]
    assert pipe._loop.program.calls[-3][1][1] == 0
    close(out, ref, "guidance_rescale v1 pipeline, 4-channel blend")
    # a duck-typed scheduler (the oracle's DDIM driven through its own .step): the same rule as tensor code
    pipe2 = PP.StableDiffusionInpaintPipeline(vae=hv, unet=hu, scheduler=OS.DDIMScheduler())
    out2 = pipe2(generator=torch.Generator().manual_seed(5), **kw)[0]
    assert pipe2._loop.foreign and "cfg_rescale" not in _names(pipe2._loop.program.calls)
    close(out2, ref, "guidance_rescale v1 pipeline, 4-channel blend, duck-typed scheduler")
    close(out2, out, "guidance_rescale v1 pipeline: duck-typed against native")
    off2 = pipe2(generator=torch.Generator().manual_seed(5), **dict(kw, guidance_rescale=0.0))[0]
    close(off2, ref0, "guidance_rescale 0.0 v1 pipeline, duck-typed scheduler")
