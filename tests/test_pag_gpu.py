"""-m gpu: perturbed-attention guidance through the engine, the fused loop and the three pipelines, against the CPU oracle with
`OM.BasicTransformerBlock.forward` patched by tests/pag_cases.py (OraclePAG) and the loops written there.

Inputs.  On a randomly initialised tiny net the self-attentions move the output little, so a wrong perturbed segment could
hide inside the network gate.  The nets of this file therefore get their self-attention value projections scaled by 4 and the
mid transformer's proj_out by 4 (`boosted`, the same weights on both sides); with that the oracle's perturbed and conditional
outputs differ by 14x the gate's bound or more for every case here (checked on the CPU; each case asserts >= 10x first).
Gates: `close` of tests/test_models_gpu.py with its defaults (cosine >= 0.999, max-abs <= 3e-2 max(1, max|ref|)).
"""
import ctypes
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
import pag_cases as PC  # noqa: E402
from oracle import schedulers as OS  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import pag as PAGM  # noqa: E402
from powerpaint_amd import pipelines as PP  # noqa: E402
from powerpaint_amd import schedulers as PS  # noqa: E402
from powerpaint_amd import tome  # noqa: E402
from test_models_gpu import DEV, close, gen, make_tiny  # noqa: E402

SD15 = dict(timestep_spacing="leading", steps_offset=1)


def boosted(kind="unet", seed=0, **extra):
    """make_tiny with the self-attentions made to matter (module docstring); the same weights on both sides."""
    o, h = make_tiny(kind, seed=seed, **extra)
    with torch.no_grad():
        for n, p in o.named_parameters():
            if n.endswith("attn1.to_v.weight") or n == "mid_block.attentions.0.proj_out.weight":
                p.copy_((p * 4.0).to(torch.bfloat16).float())
    h.load_state_dict(o.state_dict())
    return o, h


@functools.lru_cache(maxsize=None)
def _unet4():
    return boosted("unet", in_channels=4)


@functools.lru_cache(maxsize=None)
def _case_inputs(B, h, w):
    """-> (x [3B], e [3B], the oracle's output WITHOUT perturbation): computed once, shared, never modified."""
    o, _ = _unet4()
    x = torch.cat([gen(B, 4, h, w, seed=1)] * 3)
    e = PC.layout(gen(2 * B, 77, 768, seed=2), B, True)
    with torch.no_grad():
        plain = o(x, 500, e)[0]
    return x, e, plain


def _names(calls):
    return [c[2] for c in calls]


def plan_image(rt, *wired):
    """The step plan as (name, arguments) with arena addresses as offsets (a re-plan allocates a new arena; `wired`: the side
    runtimes whose residual buffers the plan reads, re-planned with it) and ctypes records spelled out."""
    arenas = [(k, r.arena.base, r.arena.size) for k, r in enumerate((rt,) + wired)]

    def norm(v):
        v = getattr(v, "_obj", v)
        if isinstance(v, bool) or v is None:
            return v
        if isinstance(v, int):
            return next((("arena", k, v - base) for k, base, size in arenas if base <= v <= base + size), v)
        if isinstance(v, ctypes.Structure):
            return tuple((f[0], norm(getattr(v, f[0]))) for f in v._fields_)
        if isinstance(v, ctypes.Array):
            return tuple(norm(x) for x in v)
        if isinstance(v, ctypes._SimpleCData):
            return norm(v.value)
        return v

    return [(name, tuple(norm(a) for a in args)) for _, args, name in rt.step_plan.calls]


# ------------------------------------------------------------------------------------------------ the tiny UNet
@pytest.mark.parametrize("layers", ["mid", "down", ["down", "mid", "up"]], ids=["mid", "down", "all"])
@pytest.mark.parametrize("h,w", [(8, 8), (6, 10), (16, 16)])
@pytest.mark.parametrize("B", [1, 2])
def test_tiny_unet_against_the_patched_oracle(B, h, w, layers):
    o, hnet = _unet4()
    x, e, plain = _case_inputs(B, h, w)
    assert sorted(hnet.pag_attn1_names()) == sorted(PC.attn1_names(o))
    hnet.set_pag_applied_layers(layers)
    sel = PAGM.attn1_names(hnet.pag_layers())
    assert sorted(sel) == sorted(PC.resolve(layers, PC.attn1_names(o)))
    with torch.no_grad(), PC.OraclePAG(o, sel, B) as orc:
        ref = o(x, 500, e)[0]
    assert all(v == 1 for v in orc.hits.values())
    # the condition, on the oracle alone: perturbing must move the last segment by >= 10x the gate's bound, and nothing else
    bound = 3e-2 * max(1.0, float(ref.abs().max()))
    moved = float((ref[2 * B:] - plain[2 * B:]).abs().max())
    print(f"[pag] B={B} {h}x{w} {layers}: perturbed - conditional reference {moved:.4f} = {moved / bound:.1f} x the gate's bound")
    assert moved >= 10 * bound, "the inputs do not make the perturbation visible: choose others"
    assert torch.equal(ref[:2 * B], plain[:2 * B])
    rt = hnet.prepare((3 * B, 4, h, w), e.to(DEV), pag_batch=B)
    rt.load_input([(x.to(DEV), 0)])
    rt.set_timestep(500)
    rt.run_step()
    out = rt.eps_tensor().float().cpu()
    what = f"pag unet tiny B={B} {h}x{w} {layers}"
    close(out[:B], ref[:B], what + " (uncond)")
    close(out[B:2 * B], ref[B:2 * B], what + " (cond)")
    close(out[2 * B:], ref[2 * B:], what + " (perturbed)")
    # the plan: one pp_attn_identity_v per selected block, behind that block's attention launch on the reduced batch
    calls = rt.step_plan.calls
    names = _names(calls)
    idx = [i for i, n in enumerate(names) if n == "attn_identity_v"]
    assert len(idx) == len(sel)
    for i in idx:
        vt, ldvt, b0, nb, n, C, a, ldo = calls[i][1]
        att = calls[i - 1]
        assert att[2] == "attention" and att[1][6] == a and att[1][4] == vt, "the identity copy follows its block's attention launch"
        assert att[1][8] == 2 * B and (b0, nb) == (2 * B, B) and att[1][10] == att[1][11] == n
    self_att = [c for c in calls if c[2] == "attention" and c[1][10] == c[1][11] and c[1][10] in (h * w, ((h + 1) // 2) * ((w + 1) // 2))]
    assert sorted(c[1][8] for c in self_att) == sorted([2 * B] * len(sel) + [3 * B] * (4 - len(sel)))
    assert ("tfront" in names) == ((h, w) == (16, 16)) and ("transpose_v" in names) == ((h, w) == (6, 10))
    assert not rt.twin


def test_off_is_off_for_the_network():
    _, hnet = boosted("unet", seed=3, in_channels=4)
    B = 2
    x, e = gen(B, 4, 8, 8, seed=1).to(DEV), gen(B, 77, 768, seed=2).to(DEV)
    never = hnet(x, 500, e, return_dict=False)[0].clone()
    image = plan_image(hnet.rt)
    hnet.set_pag_applied_layers(["down", "mid"])
    rt = hnet.prepare((3 * B, 4, 8, 8), torch.cat([e] * 3), pag_batch=B)
    assert _names(rt.step_plan.calls).count("attn_identity_v") == 2
    rt.load_input([(torch.cat([x] * 3), 0)])
    rt.set_timestep(500)
    rt.run_step()
    assert bool(torch.isfinite(rt.eps_tensor()).all())
    again = hnet(x, 500, e, return_dict=False)[0]
    assert plan_image(hnet.rt) == image, "the plan after PAG was switched off is not the never-enabled plan"
    assert torch.equal(again, never)


def test_token_merging_with_pag_is_refused_by_name():
    _, hnet = boosted("unet", seed=3, in_channels=4)
    tome.apply_patch(hnet, ratio=0.5)
    try:
        with pytest.raises(L.PPError, match="ToMe"):
            hnet.prepare((3, 4, 8, 8), gen(3, 77, 768, seed=2).to(DEV), pag_batch=1)
    finally:
        tome.remove_patch(hnet)


# ------------------------------------------------------------------------------------------------ the BrushNet pipeline
def _brushnet_setup():
    ob, hb = make_tiny("brushnet")
    ou, hu = boosted("unet", seed=1, in_channels=4)
    B, hh = 1, 8
    lat = gen(B, 4, hh, hh, seed=0)
    mask = torch.zeros(B, 1, hh, hh)
    mask[:, :, 2:6, 2:6] = 1.0
    cl = torch.cat([gen(B, 4, hh, hh, seed=1, scale=0.5), mask], 1)
    pe, peU = gen(2 * B, 77, 768, seed=2), gen(2 * B, 77, 768, seed=3)
    return ob, hb, ou, hu, B, lat, cl, pe, peU


def _brushnet_kw(B, lat, cl, pe, peU, cfg, **more):
    kw = dict(prompt_embeds=pe[B:].to(DEV), prompt_embedsU=peU[B:].to(DEV), conditioning_latents=cl.to(DEV),
              num_inference_steps=3, guidance_scale=7.5 if cfg else 1.0, latents=lat.to(DEV), output_type="latent",
              return_dict=False)
    if cfg:
        kw.update(negative_prompt_embeds=pe[:B].to(DEV), negative_prompt_embedsU=peU[:B].to(DEV))
    kw.update(more)
    return kw


def _schedulers(name):
    import ksampler_cases as KC
    import lcm_cases as LC
    import sigma_cases as SC
    if name == "ddim":
        return PS.DDIMScheduler(), lambda: OS.DDIMScheduler(), True
    if name == "euler_a":
        return PS.EulerAncestralDiscreteScheduler(**SD15), lambda: SC.EulerAncestralDiscreteScheduler(**SD15), True
    if name == "heun":
        return PS.HeunDiscreteScheduler(**SD15), lambda: KC.HeunDiscreteScheduler(**SD15), True
    return PS.LCMScheduler(), lambda: LC.LCMScheduler(), False


@pytest.mark.parametrize("name", ["ddim", "euler_a", "heun", "lcm"])
def test_brushnet_pipeline_against_the_oracle_loop(name):
    ob, hb, ou, hu, B, lat, cl, pe, peU = _brushnet_setup()
    sch, ref_sch, cfg = _schedulers(name)
    pipe = PP.StableDiffusionPowerPaintBrushNetPipeline(unet=hu, brushnet=hb, scheduler=sch, pag_applied_layers=["down", "mid"])
    sel = PAGM.attn1_names(hu.pag_layers())
    assert len(sel) == 2
    kw = _brushnet_kw(B, lat, cl, pe, peU, cfg, pag_scale=3.0)
    assert pipe.use_graph
    out = pipe(generator=torch.Generator().manual_seed(8), **kw)[0].clone()
    names = _names(pipe._loop.program.calls)
    segs = 3 if cfg else 2
    assert pipe._loop.rt.B == segs * B and pipe._loop.side_rt.B == segs * B and not pipe._loop.rt.twin
    assert names.count("pag_combine") == 1 and names.count("attn_identity_v") == 2
    step_at = names.index("pag_combine") + 1
    assert names[step_at].startswith("cfg_") and pipe._loop.program.calls[step_at][1][1] == 0, "the step launch runs with cfg = 0"
    pipe.use_graph = False
    eager = pipe(generator=torch.Generator().manual_seed(8), **kw)[0].clone()
    assert torch.equal(out, eager), "graph replay and eager replay differ"
    p, pU = (pe, peU) if cfg else (pe[B:], peU[B:])
    ref = PC.loop_v2_pag(ou, ob, ref_sch(), sel, lat, cl if not cfg else torch.cat([cl] * 2), p, pU, 3, 7.5 if cfg else 1.0, 3.0,
                         generator=torch.Generator().manual_seed(8))
    plain = pipe(generator=torch.Generator().manual_seed(8), **dict(kw, pag_scale=0.0))[0]
    d = float((plain.float().cpu() - ref).abs().max())
    print(f"[pag] BrushNet pipeline {name}: the PAG-free call is {d:.3f} away from the PAG reference (max|ref| {float(ref.abs().max()):.3f})")
    close(out, ref, f"pag BrushNet pipeline, {name}, 3 steps")


def test_a_new_scale_pair_reaches_the_graph_without_a_recapture():
    ob, hb, ou, hu, B, lat, cl, pe, peU = _brushnet_setup()
    pipe = PP.StableDiffusionPowerPaintBrushNetPipeline(unet=hu, brushnet=hb, scheduler=PS.DDIMScheduler())
    pipe.set_pag_applied_layers(["down", "mid"])
    sel = PAGM.attn1_names(hu.pag_layers())
    kw = _brushnet_kw(B, lat, cl, pe, peU, True)
    never = pipe(**kw)[0].clone()
    never_names = _names(pipe._loop.program.calls)
    never_image = plan_image(hu.rt, hb.rt)
    out3 = pipe(pag_scale=3.0, **kw)[0].clone()
    loop = pipe._loop
    g0, program0, table = loop.graph, loop.program, loop._pag_table
    assert g0 is not None and table.cpu().tolist() == [3.0] * 3
    out1 = pipe(pag_scale=1.5, **kw)[0].clone()
    assert loop.graph is g0 and loop.program is program0 and loop._pag_table is table, "a new pag_scale re-captured the step"
    assert table.cpu().tolist() == [1.5] * 3 and not torch.equal(out1, out3)
    # adaptive: the last row's scale is 0, the first two are not
    ts = [float(t) for t in pipe.scheduler.timesteps.tolist()]
    a = 3.0 / (1000.0 - 0.5 * (ts[1] + ts[2]))
    want = [float(PC.scale_f64(3.0, a, t)) for t in ts]
    assert want[2] == 0.0 and want[0] > 0.0 and want[1] > 0.0
    outa = pipe(pag_scale=3.0, pag_adaptive_scale=a, **kw)[0].clone()
    assert loop.graph is g0
    assert table.cpu().tolist() == [float(torch.tensor(v, dtype=torch.float32)) for v in want] and float(table[2]) == 0.0
    ref = PC.loop_v2_pag(ou, ob, OS.DDIMScheduler(), sel, lat, torch.cat([cl] * 2), pe, peU, 3, 7.5, 3.0, pag_adaptive_scale=a)
    close(outa, ref, "pag BrushNet pipeline, DDIM, adaptive scale")
    # off is off: pag_scale = 0.0 is the never-enabled program, plan and output
    off = pipe(pag_scale=0.0, **kw)[0]
    assert _names(pipe._loop.program.calls) == never_names and "pag_combine" not in never_names
    assert plan_image(hu.rt, hb.rt) == never_image
    assert torch.equal(off, never)
    with pytest.raises(L.PPError, match="guess_mode"):
        pipe(pag_scale=3.0, guess_mode=True, **kw)
    with pytest.raises(ValueError, match="nonexistent"):
        pipe.set_pag_applied_layers("nonexistent")


# ------------------------------------------------------------------------------------------------ the other two pipelines
def test_controlnet_pipeline_two_nets_one_window_closing():
    oc1, hc1 = make_tiny("controlnet")
    oc2, hc2 = make_tiny("controlnet", seed=5)
    ou, hu = boosted("unet", seed=1, in_channels=9)
    B, hh, N = 1, 8, 3
    lat, mask, mil = gen(B, 4, hh, hh, seed=0), torch.zeros(B, 1, hh, hh), gen(B, 4, hh, hh, seed=1, scale=0.5)
    mask[:, :, 2:6, 2:6] = 1.0
    pe = gen(2 * B, 77, 768, seed=2)
    imgs = [torch.rand(B, 3, 8 * hh, 8 * hh, generator=torch.Generator().manual_seed(3 + i)) for i in range(2)]
    pipe = PP.StableDiffusionControlNetInpaintPipeline(unet=hu, controlnet=[hc1, hc2], scheduler=PS.DDIMScheduler(),
                                                       pag_applied_layers="mid")
    sel = PAGM.attn1_names(hu.pag_layers())
    scales, starts, ends = [0.5, 0.8], [0.0, 0.0], [1.0, 0.4]
    rows = pipe.control_schedule(N, scales, starts, ends)
    assert [r[1] != 0.0 for r in rows] == [True, False, False]
    out = pipe(prompt_embeds=pe[B:].to(DEV), negative_prompt_embeds=pe[:B].to(DEV), height=8 * hh, width=8 * hh,
               control_image=[i.to(DEV) for i in imgs], controlnet_conditioning_scale=scales, control_guidance_start=starts,
               control_guidance_end=ends, num_inference_steps=N, guidance_scale=7.5, latents=lat.to(DEV),
               mask_latents=mask.to(DEV), masked_image_latents=mil.to(DEV), output_type="latent", return_dict=False,
               pag_scale=3.0)[0]
    assert all(r.B == 3 * B for r in pipe._loop.side_rts) and pipe._loop.rt.B == 3 * B
    two = PC.TwoControlNets([oc1, oc2], [torch.cat([i] * 3) for i in imgs], rows)
    ref = PC.loop_v1_pag(ou, OS.DDIMScheduler(), sel, lat, mask, mil, pe, N, 7.5, 3.0, controlnet=two)
    assert bool(torch.isfinite(out).all())
    close(out, ref, "pag ControlNet pipeline, two nets, one window closing")


def test_v1_pipeline_with_the_4_channel_blend():
    import make_ref_pipeline_call as M
    from powerpaint_amd import models as PM
    _, _, unet, vae = M.components_4ch()
    img, mask, _ = M.inputs()
    hu = PM.UNet2DConditionModel(in_channels=4, device=DEV, **M.TINY).load_state_dict(unet.state_dict())
    hv = PM.AutoencoderKL(device=DEV, **M.VAE_CFG).load_state_dict(vae.state_dict())
    pe = gen(2, 77, 768, seed=2)
    pipe = PP.StableDiffusionInpaintPipeline(vae=hv, unet=hu, scheduler=PS.DDIMScheduler(), pag_applied_layers=["mid", "up"])
    sel = PAGM.attn1_names(hu.pag_layers())
    out = pipe(prompt_embeds=pe[1:].to(DEV), negative_prompt_embeds=pe[:1].to(DEV), image=img, mask=mask, height=128, width=128,
               num_inference_steps=3, guidance_scale=7.5, generator=torch.Generator().manual_seed(5), output_type="latent",
               return_dict=False, pag_scale=3.0)[0]
    names = _names(pipe._loop.program.calls)
    assert names[-4:] == ["pag_combine", "cfg_sched_step", "latent_blend", "step_advance"]
    m = torch.nn.functional.interpolate(mask, size=(16, 16))
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        il = vae.encode(img).latent_dist.sample(g) * vae.config.scaling_factor
        noise = torch.randn(1, 4, 16, 16, generator=g)
    ref = PC.loop_v1_pag(unet, OS.DDIMScheduler(), sel, noise, m, None, pe, 3, 7.5, 3.0, image_latents=il, noise=noise)
    assert bool(torch.isfinite(out).all())
    close(out, ref, "pag v1 pipeline, 4-channel blend")
    # a duck-typed scheduler (the oracle's DDIM driven through its own .step): the same combine as tensor code
    pipe2 = PP.StableDiffusionInpaintPipeline(vae=hv, unet=hu, scheduler=OS.DDIMScheduler(), pag_applied_layers=["mid", "up"])
    out2 = pipe2(prompt_embeds=pe[1:].to(DEV), negative_prompt_embeds=pe[:1].to(DEV), image=img, mask=mask, height=128, width=128,
                 num_inference_steps=3, guidance_scale=7.5, generator=torch.Generator().manual_seed(5), output_type="latent",
                 return_dict=False, pag_scale=3.0)[0]
    assert pipe2._loop.foreign and "pag_combine" not in _names(pipe2._loop.program.calls) and pipe2._loop.rt.B == 3
    close(out2, ref, "pag v1 pipeline, 4-channel blend, duck-typed scheduler")


# ------------------------------------------------------------------------------------------------ IP-Adapter
def test_unet_with_a_base_adapter_and_pag():
    import ip_adapter_cases as IC
    o, hnet = boosted("unet", seed=7, in_channels=4)
    sds = [IC.adapter_state_dict(o, 50, std=1.0)]
    ipu = IC.IPUNet(o, sds, [1.0]).eval()
    hnet._load_ip_adapter_weights(sds)
    hnet.set_pag_applied_layers(["down", "mid"])
    sel = PAGM.attn1_names(hnet.pag_layers())
    B = 1
    x = torch.cat([gen(B, 4, 8, 8, seed=1)] * 3)
    e = PC.layout(gen(2 * B, 77, 768, seed=2), B, True)
    emb = PC.layout(gen(2 * B, 1, IC.EMBED_DIM, seed=4), B, True)             # [neg, pos] -> [neg, pos, pos]
    with torch.no_grad():
        plain = ipu(x, torch.tensor(500), e, added_cond_kwargs={"image_embeds": [emb]})[0]
        with PC.OraclePAG(o, sel, B):
            ref = ipu(x, torch.tensor(500), e, added_cond_kwargs={"image_embeds": [emb]})[0]
    assert float((ref[2:] - plain[2:]).abs().max()) >= 10 * 3e-2 * max(1.0, float(ref.abs().max()))
    rt = hnet.prepare((3 * B, 4, 8, 8), e.to(DEV), added_cond_kwargs={"image_embeds": [emb.to(DEV)]}, pag_batch=B)
    rt.load_input([(x.to(DEV), 0)])
    rt.set_timestep(500)
    rt.run_step()
    out = rt.eps_tensor().float().cpu()
    names = _names(rt.step_plan.calls)
    assert names.count("attn_identity_v") == 2 and names.count("ip_attn_add") == 4
    for k, seg in enumerate(("uncond", "cond", "perturbed")):
        close(out[k:k + 1], ref[k:k + 1], f"pag + IP-Adapter unet tiny ({seg})")
