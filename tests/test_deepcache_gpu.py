"""-m gpu: DeepCache through the engine -- small networks against the CPU oracle wrapped by the restatement of
tests/deepcache_cases.py (a sequence of full and shallow evaluations on independent inputs), side networks, bitwise identities,
and the three pipelines through the fused loop (graph replay against eager replay, the oracle loops driven with the wrappers).

The networks are test_models_gpu.make_tiny's as they are: tests/test_deepcache.py establishes in float64 that on fresh inputs a
shallow evaluation of them leaves the small networks' gate against the PLAIN oracle at every cache_branch_id (cosine 0.80 ..
0.91), so "evaluations 1 and 2 must FAIL `close` against the plain oracle" can tell a network that ignores the patch from one
that honours it; the second shallow evaluation is the one that catches a cache clobbered by the first.
Gates: test_models_gpu.close (cosine >= 0.999, max-abs <= 3e-2 max(1, max|ref|)) for single evaluations; for the pipelines the
gate their neighbours in test_models_gpu.py use (cosine >= 0.9997, max-abs <= 4.5e-2 max|ref| on the final latents).
"""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import deepcache_cases as DC  # noqa: E402
from oracle import loops as OL  # noqa: E402
from oracle import schedulers as OS  # noqa: E402
from powerpaint_amd import hypertile  # noqa: E402
from powerpaint_amd import models as PM  # noqa: E402
from powerpaint_amd import pipelines as PP  # noqa: E402
from powerpaint_amd import schedulers as PS  # noqa: E402
from powerpaint_amd.deepcache import DeepCacheSDHelper  # noqa: E402
from powerpaint_amd.lora import unet_targets  # noqa: E402
from test_models_gpu import DEV, TINY, _v1_inputs, close, gen, make_tiny  # noqa: E402

SEQ = "FSSFS"                     # five evaluations at cache_interval 3
TS = [901, 640, 333, 500, 99]


def _seq_inputs(cin, h, w, B=2):
    return [(gen(B, cin, h, w, seed=10 + ev), TS[ev], gen(B, 77, 768, seed=20 + ev)) for ev in range(len(SEQ))]


@functools.lru_cache(maxsize=None)
def _unet(cin):
    return make_tiny("unet", in_channels=cin)


@functools.lru_cache(maxsize=None)
def _references(cin, bid, h=16, w=16):
    """-> per evaluation (the plain oracle's output, the restatement's): computed once, never modified."""
    o, _ = _unet(cin)
    wr = DC.DeepCacheUNet(o, 3, bid)
    out = []
    for x, t, e in _seq_inputs(cin, h, w):
        with torch.no_grad():
            out.append((o(x, t, e)[0], wr(x, t, e)[0]))
    assert "".join(wr.trace) == SEQ
    return out


def _run_sequence(hnet, cin, bid, h=16, w=16, what=""):
    refs = _references(cin, bid, h, w)
    helper = DeepCacheSDHelper(hnet).set_params(cache_interval=3, cache_branch_id=bid).enable()
    try:
        for ev, ((x, t, e), (plain, want)) in enumerate(zip(_seq_inputs(cin, h, w), refs)):
            out = hnet(x.to(DEV), t, e.to(DEV), return_dict=False)[0].clone()
            close(out, want, f"deepcache {what} id {bid} evaluation {ev} ({SEQ[ev]}) against the restatement")
            if ev in (1, 2):                 # the patch has an observable effect at this gate
                with pytest.raises(AssertionError):
                    close(out, plain, f"deepcache {what} id {bid} evaluation {ev} against the PLAIN oracle (must fail)")
            elif SEQ[ev] == "F":
                close(out, plain, f"deepcache {what} id {bid} evaluation {ev} (full) against the plain oracle")
        assert hnet.rt.dc_eval == len(SEQ) and hnet.rt.shallow_plan is not None
    finally:
        helper.disable()


@pytest.mark.parametrize("bid", [0, 1, 2])
@pytest.mark.parametrize("cin", [4, 9])
def test_unet_sequence(cin, bid):
    _, hnet = _unet(cin)
    _run_sequence(hnet, cin, bid, what=f"unet tiny cin {cin}")


def test_unet_sequence_fp16():
    o, _ = _unet(4)
    hnet = PM.UNet2DConditionModel(in_channels=4, device=DEV, dtype=torch.float16, **TINY).load_state_dict(o.state_dict())
    _run_sequence(hnet, 4, 0, what="unet tiny fp16")


def test_off_grid_latent():
    """10 x 14: the level below is 5 x 7, and c is the upsampler's output (cache_branch_id 0 of TINY)."""
    _, hnet = _unet(4)
    _run_sequence(hnet, 4, 0, h=10, w=14, what="unet tiny 10x14")
    assert (hnet.rt.H, hnet.rt.W) == (10, 14)


def test_brushnet_into_unet_sequence():
    ob, hb = make_tiny("brushnet")
    ou, hu = make_tiny("unet", seed=1, in_channels=4)
    wb, wu = DC.DeepCacheBrushNet(ob, 3, 0), DC.DeepCacheUNet(ou, 3, 0)
    helpers = [DeepCacheSDHelper(m).set_params(3, 0).enable() for m in (hb, hu)]
    try:
        for ev in range(len(SEQ)):
            x, t, e, eu, cond = (gen(2, 4, 16, 16, seed=30 + ev), TS[ev], gen(2, 77, 768, seed=40 + ev),
                                 gen(2, 77, 768, seed=50 + ev), gen(2, 5, 16, 16, seed=60 + ev))
            dn, md, up = wb(x, t, e, cond, conditioning_scale=0.8)
            want = wu(x, t, eu, down_block_add_samples=list(dn), mid_block_add_sample=md, up_block_add_samples=list(up))[0]
            with torch.no_grad():
                pdn, pmd, pup = ob(x, t, e, cond, conditioning_scale=0.8)
                plain = ou(x, t, eu, down_block_add_samples=list(pdn), mid_block_add_sample=pmd, up_block_add_samples=list(pup))[0]
            hdn, hmd, hup = hb(x.to(DEV), t, e.to(DEV), cond.to(DEV), conditioning_scale=0.8, return_dict=False)
            res, ref = hdn + [hmd] + hup, list(dn) + [md] + list(up)
            for p in wb.live:                # every live residual, against the restatement's
                close(res[p], ref[p], f"deepcache brushnet evaluation {ev} ({SEQ[ev]}) residual {p}", cos_min=0.998)
            out = hu(x.to(DEV), t, eu.to(DEV), down_block_add_samples=list(hdn), mid_block_add_sample=hmd,
                     up_block_add_samples=list(hup), return_dict=False)[0]
            close(out, want, f"deepcache unet(+brushnet) evaluation {ev} ({SEQ[ev]}) against the restatement")
            if ev in (1, 2):
                with pytest.raises(AssertionError):
                    close(out, plain, f"deepcache unet(+brushnet) evaluation {ev} against the PLAIN oracles (must fail)")
        # only live residuals are produced: the shallow plan's zero convs are positions 0, 1 and the last two up layers
        sh = hb.rt.shallow_plan
        assert [c[2] for c in sh.calls].count("zero_conv") == 4 and sh.zero_conv_pos == wb.live == [0, 1, 8, 9]
        assert [c[2] for c in hb.rt.step_plan.calls].count("zero_conv") == 4 + 1 + 5
        full = hb.rt.zero_conv_records()
        assert [a.out for a in hb.rt.zero_conv_records(sh)] == [full[p].out for p in sh.zero_conv_pos]
    finally:
        for hlp in helpers:
            hlp.disable()


@pytest.mark.parametrize("guess_mode", [False, True], ids=["plain", "guess_mode"])
def test_controlnet_into_unet_sequence(guess_mode):
    oc, hc = make_tiny("controlnet")
    ou, hu = make_tiny("unet", seed=1, in_channels=9)
    wc, wu = DC.DeepCacheControlNet(oc, 3, 0), DC.DeepCacheUNet(ou, 3, 0)
    helpers = [DeepCacheSDHelper(m).set_params(3, 0).enable() for m in (hc, hu)]
    try:
        for ev in range(len(SEQ)):
            x4, x9, t, e = gen(2, 4, 16, 16, seed=30 + ev), gen(2, 9, 16, 16, seed=70 + ev), TS[ev], gen(2, 77, 768, seed=40 + ev)
            img = torch.rand(2, 3, 128, 128, generator=torch.Generator("cpu").manual_seed(80 + ev))
            dn, md = wc(x4, t, e, img, conditioning_scale=0.5, guess_mode=guess_mode)
            want = wu(x9, t, e, down_block_additional_residuals=dn, mid_block_additional_residual=md)[0]
            with torch.no_grad():
                pdn, pmd = oc(x4, t, e, img, conditioning_scale=0.5, guess_mode=guess_mode)
                plain = ou(x9, t, e, down_block_additional_residuals=pdn, mid_block_additional_residual=pmd)[0]
            hdn, hmd = hc(x4.to(DEV), t, e.to(DEV), img.to(DEV), conditioning_scale=0.5, guess_mode=guess_mode, return_dict=False)
            for p in wc.live:
                close((hdn + [hmd])[p], (list(dn) + [md])[p], f"deepcache controlnet evaluation {ev} ({SEQ[ev]}) residual {p}",
                      cos_min=0.998)
            out = hu(x9.to(DEV), t, e.to(DEV), down_block_additional_residuals=hdn, mid_block_additional_residual=hmd,
                     return_dict=False)[0]
            close(out, want, f"deepcache unet(+controlnet, guess_mode={guess_mode}) evaluation {ev} ({SEQ[ev]})")
            if ev in (1, 2):
                with pytest.raises(AssertionError):
                    close(out, plain, f"deepcache unet(+controlnet) evaluation {ev} against the PLAIN oracles (must fail)")
        sh = hc.rt.shallow_plan
        assert [c[2] for c in sh.calls].count("zero_conv") == 2 and sh.zero_conv_pos == wc.live == [0, 1]
        if guess_mode:                       # the logspace scales keep their full-network values at the live positions
            want_sc = [float(s) * 0.5 for s in torch.logspace(-1, 0, 5)][:2]
            assert [a.scale for a in hc.rt.zero_conv_records(sh)] == pytest.approx(want_sc)
    finally:
        for hlp in helpers:
            hlp.disable()


def test_interval_one_and_disable_are_bitwise_the_unpatched_network():
    _, hnet = _unet(4)
    ins = [(x.to(DEV), t, e.to(DEV)) for x, t, e in _seq_inputs(4, 16, 16)[:3]]
    never = [hnet(x, t, e, return_dict=False)[0].clone() for x, t, e in ins]
    helper = DeepCacheSDHelper(hnet).set_params(cache_interval=1, cache_branch_id=1).enable()
    try:
        for (x, t, e), want in zip(ins, never):
            assert torch.equal(hnet(x, t, e, return_dict=False)[0], want)       # every evaluation full: the same launches
        assert hnet.rt.shallow_plan is not None
        helper.set_params(cache_interval=2, cache_branch_id=1)
        got = [hnet(x, t, e, return_dict=False)[0].clone() for x, t, e in ins]
        assert torch.equal(got[0], never[0]) and not torch.equal(got[1], never[1]) and torch.equal(got[2], never[2])
    finally:
        helper.disable()
    for (x, t, e), want in zip(ins, never):
        assert torch.equal(hnet(x, t, e, return_dict=False)[0], want)
    assert hnet.rt.shallow_plan is None


def test_freeu_at_the_cache_point_leaves_the_cache_alone():
    """TINY at cache_branch_id 0: c is handed to up_blocks.1.resnets.0, which FreeU (resolution_idx 1: b2, s2) runs in front of,
    and pp_freeu rewrites the hidden tensor in place everywhere else.  Evaluations F S S on ONE input: the shallow form does the
    full form's arithmetic on c (the norm's statistics come from FreeU's launch in both), so both shallow outputs sit at the
    full one within the small networks' gate -- and a c that an in-place FreeU had scaled (b2 = 1.4 on half its channels, once
    per evaluation) would leave it at the first shallow evaluation and further at the second."""
    _, hnet = _unet(4)
    x, t, e = (v.to(DEV) if torch.is_tensor(v) else v for v in _seq_inputs(4, 16, 16)[0])
    hnet.enable_freeu(s1=0.9, s2=0.2, b1=1.2, b2=1.4)
    helper = DeepCacheSDHelper(hnet).set_params(cache_interval=3, cache_branch_id=0).enable()
    try:
        full = hnet(x, t, e, return_dict=False)[0].clone()
        assert [c[2] for c in hnet.rt.shallow_plan.calls].count("freeu") == 2
        for ev in (1, 2):
            close(hnet(x, t, e, return_dict=False)[0], full, f"deepcache + FreeU: shallow evaluation {ev} on the full one's input")
        helper.disable()
        plain = hnet(x, t, e, return_dict=False)[0].clone()
        assert torch.equal(plain, full)                                      # the full form's copy of c changes no number
    finally:
        helper.disable()
        hnet.disable_freeu()


# ------------------------------------------------------------------------------------------------------------ pipelines
def _graph_and_eager(pipe, kw):
    assert pipe.use_graph
    out = pipe(**kw)[0].clone()
    pipe.use_graph = False
    eager = pipe(**kw)[0].clone()
    pipe.use_graph = True
    assert torch.equal(out, eager), "graph replay and eager replay differ"
    assert torch.equal(pipe(**kw)[0], out)                                   # every call counts its evaluations from 0
    return out


def _v1_kw(pe, lat, mask, mil, hh, ww, N, B):
    return dict(prompt_embeds=pe[B:].to(DEV), negative_prompt_embeds=pe[:B].to(DEV), height=hh * 8, width=ww * 8,
                num_inference_steps=N, guidance_scale=7.5, latents=lat.to(DEV), mask_latents=mask.to(DEV),
                masked_image_latents=mil.to(DEV), output_type="latent", return_dict=False)


def test_pipeline_v1_ddim_heun_and_a_duck_typed_scheduler():
    import ksampler_cases as KC
    from test_sigma_gpu import SD15
    o, h = _unet(9)
    B, hh, N = 2, 16, 5
    lat, mask, mil, pe = _v1_inputs(B, hh, hh)
    kw = _v1_kw(pe, lat, mask, mil, hh, hh, N, B)
    pipe = PP.StableDiffusionInpaintPipeline(unet=h, scheduler=PS.DDIMScheduler())
    never = pipe(**kw)[0].clone()
    helper = DeepCacheSDHelper(pipe).set_params(cache_interval=2, cache_branch_id=0).enable()
    try:
        out = _graph_and_eager(pipe, kw)
        assert pipe._loop.shallow_rows(N) == [False, True, False, True, False] and not torch.equal(out, never)
        wr = DC.DeepCacheUNet(o, 2, 0)
        ref = OL.loop_v1(wr, OS.DDIMScheduler(), lat, torch.cat([mask] * 2), torch.cat([mil] * 2), pe, N, 7.5)
        assert "".join(wr.trace) == "FSFSF"
        close(out, ref, "deepcache v1 DDIM, interval 2, free-running", cos_min=0.9997, rel=4.5e-2)
        # a duck-typed scheduler (the oracle's class) drives the same two programs
        duck = PP.StableDiffusionInpaintPipeline(unet=h, scheduler=OS.DDIMScheduler())
        dout = _graph_and_eager_close(duck, kw)
        close(dout, out, "deepcache v1 duck-typed DDIM against the fused step", cos_min=0.9999, rel=1e-2)
        # Heun: 5 steps are 9 rows, every row an evaluation (F S F S F S F S F)
        hp = PP.StableDiffusionInpaintPipeline(unet=h, scheduler=PS.HeunDiscreteScheduler(**SD15))
        hout = _graph_and_eager(hp, kw)
        assert hp._loop.shallow_rows(9) == [bool(i % 2) for i in range(9)]
        wr.reset()
        href = OL.loop_v1(wr, KC.CLASSES["HeunDiscreteScheduler"](**SD15), lat, torch.cat([mask] * 2), torch.cat([mil] * 2), pe,
                          N, 7.5)
        assert "".join(wr.trace) == "FSFSFSFSF"
        close(hout, href, "deepcache v1 Heun, interval 2, free-running", cos_min=0.9997, rel=4.5e-2)
    finally:
        helper.disable()
    assert torch.equal(pipe(**kw)[0], never)


def _graph_and_eager_close(pipe, kw):
    """A duck-typed scheduler's own tensor code runs between the replays: graph against eager at the neighbouring test's gate."""
    out = pipe(**kw)[0].clone()
    pipe.use_graph = False
    close(pipe(**kw)[0], out, "deepcache duck-typed eager vs graph", cos_min=0.99999, rel=1e-4)
    pipe.use_graph = True
    return out


def test_pipeline_v2_brushnet():
    ob, hb = make_tiny("brushnet")
    ou, hu = make_tiny("unet", seed=1, in_channels=4)
    B, hh, N = 2, 16, 5
    lat = gen(B, 4, hh, hh, seed=0)
    mask = torch.zeros(B, 1, hh, hh)
    mask[:, :, 4:12, 4:12] = 1.0
    cl = torch.cat([gen(B, 4, hh, hh, seed=1, scale=0.5), mask], 1)
    pe, peU = gen(2 * B, 77, 768, seed=2), gen(2 * B, 77, 768, seed=3)
    pipe = PP.StableDiffusionPowerPaintBrushNetPipeline(unet=hu, brushnet=hb, scheduler=PS.DPMSolverMultistepScheduler())
    kw = dict(prompt_embeds=pe[B:].to(DEV), negative_prompt_embeds=pe[:B].to(DEV), prompt_embedsU=peU[B:].to(DEV),
              negative_prompt_embedsU=peU[:B].to(DEV), conditioning_latents=cl.to(DEV), num_inference_steps=N,
              guidance_scale=7.5, latents=lat.to(DEV), output_type="latent", return_dict=False)
    never = pipe(**kw)[0].clone()
    helper = DeepCacheSDHelper(pipe).set_params(cache_interval=2, cache_branch_id=0).enable()
    try:
        assert hb.net.deepcache is not None and hu.net.deepcache is not None
        out = _graph_and_eager(pipe, kw)
        assert not torch.equal(out, never)
        wb, wu = DC.DeepCacheBrushNet(ob, 2, 0), DC.DeepCacheUNet(ou, 2, 0)
        ref = OL.loop_v2(wu, wb, OS.DPMSolverMultistepScheduler(), lat, torch.cat([cl] * 2), pe, peU, N, 7.5, 1.0)
        assert "".join(wb.trace) == "".join(wu.trace) == "FSFSF"
        close(out, ref, "deepcache v2 DPM-Solver++, interval 2, free-running", cos_min=0.9997, rel=4.5e-2)
        gref = OL.loop_v2(_reset(wu), _reset(wb), OS.DPMSolverMultistepScheduler(), lat, cl, pe, peU, N, 7.5, 1.0, guess_mode=True)
        gout = pipe(guess_mode=True, **dict(kw, conditioning_latents=cl.to(DEV)))[0]
        close(gout, gref, "deepcache v2 guess_mode, interval 2, free-running", cos_min=0.9997, rel=4.5e-2)
    finally:
        helper.disable()
    assert torch.equal(pipe(**kw)[0], never)


def _reset(w):
    w.reset()
    return w


def test_pipeline_controlnet_with_hypertile_lora_and_strength():
    """UNet + ControlNet at 16 x 64 (HyperTile's 1 x 2 tiles), first plain, then with HyperTile, a LoRA and strength 0.6 of 5
    steps (3 evaluations, F S F, entered at row 2 of the schedule), against the oracle loop with the merged weights, the tiled
    top level (test_hypertile_gpu.OracleHyperTile) and the wrappers."""
    from lora_cases import make_factors
    from test_hypertile_gpu import H16, W64, OracleHyperTile, sharpened
    from test_lora_gpu import oracle_with
    oc, hc = make_tiny("controlnet")
    ou, hu, sd = sharpened("unet", seed=1, in_channels=9)
    B, N = 1, 5
    lat, mask, mil, pe = _v1_inputs(B, H16, W64)
    img = torch.rand(B, 3, 8 * H16, 8 * W64, generator=torch.Generator().manual_seed(3))
    pipe = PP.StableDiffusionControlNetInpaintPipeline(unet=hu, controlnet=hc, scheduler=PS.DDIMScheduler())
    kw = dict(_v1_kw(pe, lat, mask, mil, H16, W64, N, B), control_image=img.to(DEV))
    never = pipe(**kw)[0].clone()
    helper = DeepCacheSDHelper(pipe).set_params(cache_interval=2, cache_branch_id=0).enable()
    try:
        out = _graph_and_eager(pipe, kw)
        wc, wu = DC.DeepCacheControlNet(oc, 2, 0), DC.DeepCacheUNet(ou, 2, 0)
        ref = OL.loop_v1(wu, OS.DDIMScheduler(), lat, torch.cat([mask] * 2), torch.cat([mil] * 2), pe, N, 7.5,
                         controlnet=wc, control_image=torch.cat([img] * 2), controlnet_conditioning_scale=0.5)
        close(out, ref, "deepcache controlnet DDIM, interval 2, free-running", cos_min=0.9997, rel=4.5e-2)
        assert not torch.equal(out, never) and [c[2] for c in hc.rt.shallow_plan.calls].count("zero_conv") == 2
        fac = make_factors(unet_targets(hu.net), sd, 4, seed=51)
        hypertile.apply_patch(pipe)
        hu.load_lora_adapter(fac, "dc")
        try:
            more = dict(kw, strength=0.6)
            got = _graph_and_eager(pipe, more)
            assert pipe._loop.shallow_rows(3) == [False, True, False]
            assert any(c[0].__name__ == "pp_attention_fwd_tiled" for c in hu.rt.shallow_plan.calls)
            wl = DC.DeepCacheUNet(oracle_with(ou, sd, [(fac, 1.0)], 1.0), 2, 0)
            with OracleHyperTile(H16, W64):
                ref2 = OL.loop_v1(wl, OS.DDIMScheduler(), lat, torch.cat([mask] * 2), torch.cat([mil] * 2), pe, N, 7.5,
                                  controlnet=_reset(wc), control_image=torch.cat([img] * 2), controlnet_conditioning_scale=0.5,
                                  t_start=2)
            assert "".join(wl.trace) == "FSF"
            close(got, ref2, "deepcache controlnet + HyperTile + LoRA + strength 0.6", cos_min=0.9997, rel=4.5e-2)
        finally:
            hu.delete_adapters(hu.list_adapters())
            hypertile.remove_patch(pipe)
    finally:
        helper.disable()
    assert torch.equal(pipe(**kw)[0], never)


class _SumOfControlNets:
    """Several wrapped oracle ControlNets in the place of one: each on its own control image and scale, the residuals of the
    live positions summed (what MultiControlNetModel hands the UNet)."""

    def __init__(self, wrappers, images, scales):
        self.ws, self.images, self.scales = wrappers, images, scales

    def __call__(self, x, t, encoder_hidden_states, controlnet_cond=None, conditioning_scale=None, guess_mode=False):
        outs = [w(x, t, encoder_hidden_states, img, conditioning_scale=sc, guess_mode=guess_mode)
                for w, img, sc in zip(self.ws, self.images, self.scales)]
        live, n = self.ws[0].live, self.ws[0].n
        down = [sum(o[0][p] for o in outs) if p in live else DC.DEAD for p in range(n)]
        return down, (sum(o[1] for o in outs) if n in live else DC.DEAD)


def test_pipeline_with_two_controlnets_and_the_refusal_of_changing_sets():
    from powerpaint_amd import _lib as L
    oc1, hc1 = make_tiny("controlnet")
    oc2, hc2 = make_tiny("controlnet", seed=2)
    ou, hu = make_tiny("unet", seed=1, in_channels=9)
    B, hh, N = 1, 16, 5
    lat, mask, mil, pe = _v1_inputs(B, hh, hh)
    imgs = [torch.rand(B, 3, hh * 8, hh * 8, generator=torch.Generator("cpu").manual_seed(s)) for s in (9, 10)]
    pipe = PP.StableDiffusionControlNetInpaintPipeline(unet=hu, controlnet=PM.MultiControlNetModel([hc1, hc2]),
                                                       scheduler=PS.DDIMScheduler())
    kw = dict(_v1_kw(pe, lat, mask, mil, hh, hh, N, B), control_image=[i.to(DEV) for i in imgs],
              controlnet_conditioning_scale=[0.5, 0.8])
    never = pipe(**kw)[0].clone()
    helper = DeepCacheSDHelper(pipe).set_params(cache_interval=2, cache_branch_id=0).enable()
    try:
        assert hc1.net.deepcache is not None and hc2.net.deepcache is not None
        out = _graph_and_eager(pipe, kw)
        ws = [DC.DeepCacheControlNet(oc1, 2, 0), DC.DeepCacheControlNet(oc2, 2, 0)]
        side = _SumOfControlNets(ws, [torch.cat([i] * 2) for i in imgs], [0.5, 0.8])
        ref = OL.loop_v1(DC.DeepCacheUNet(ou, 2, 0), OS.DDIMScheduler(), lat, torch.cat([mask] * 2), torch.cat([mil] * 2), pe, N,
                         7.5, controlnet=side, control_image=None)
        close(out, ref, "deepcache two ControlNets, interval 2, free-running", cos_min=0.9997, rel=4.5e-2)
        assert not torch.equal(out, never)
        with pytest.raises(L.PPError, match="DeepCache with several ControlNets whose set of active nets changes"):
            pipe(control_guidance_start=[0.0, 0.5], control_guidance_end=[1.0, 1.0], **kw)
    finally:
        helper.disable()
    assert torch.equal(pipe(**kw)[0], never)


def test_v1_pipeline_with_the_4_channel_blend_and_eta():
    """A 4-channel UNet: latent_blend and (eta > 0) ddim_variance_noise stand behind the step launch, and the counter moves in
    pp_step_advance -- the one tail both programs share.  Pixels in (the VAE on the HIP path), 5 steps at interval 2."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_ref_pipeline_call as M
    _, _, unet, vae = M.components_4ch()
    img, mask, _ = M.inputs()
    hu = PM.UNet2DConditionModel(in_channels=4, device=DEV, **M.TINY).load_state_dict(unet.state_dict())
    hv = PM.AutoencoderKL(device=DEV, **M.VAE_CFG).load_state_dict(vae.state_dict())
    pe = gen(2, 77, 768, seed=2)
    pipe = PP.StableDiffusionInpaintPipeline(vae=hv, unet=hu, scheduler=PS.DDIMScheduler())
    kw = dict(prompt_embeds=pe[1:].to(DEV), negative_prompt_embeds=pe[:1].to(DEV), image=img, mask=mask, height=128, width=128,
              num_inference_steps=5, guidance_scale=7.5, output_type="latent", return_dict=False)
    helper = DeepCacheSDHelper(pipe).set_params(cache_interval=2, cache_branch_id=0).enable()
    try:
        out = pipe(generator=torch.Generator().manual_seed(5), **kw)[0].clone()
        for prog in (pipe._loop.program, pipe._loop.program_shallow):
            assert [c[2] for c in prog.calls][-3:] == ["cfg_sched_step", "latent_blend", "step_advance"]
        m = torch.nn.functional.interpolate(mask, size=(16, 16))
        with torch.no_grad():
            g = torch.Generator().manual_seed(5)
            il = vae.encode(img).latent_dist.sample(g) * vae.config.scaling_factor
            noise = torch.randn(1, 4, 16, 16, generator=g)
        wr = DC.DeepCacheUNet(unet, 2, 0)
        ref = OL.loop_v1(wr, OS.DDIMScheduler(), noise, torch.cat([m] * 2), None, pe, 5, 7.5, image_latents=il, noise=noise)
        assert "".join(wr.trace) == "FSFSF"
        close(out, ref, "deepcache v1 4-channel blend, interval 2, free-running", cos_min=0.9997, rel=4.5e-2)
        pipe.use_graph = False
        assert torch.equal(pipe(generator=torch.Generator().manual_seed(5), **kw)[0], out)
        eager = pipe(generator=torch.Generator().manual_seed(5), eta=0.4, **kw)[0].clone()
        pipe.use_graph = True
        graph = pipe(generator=torch.Generator().manual_seed(5), eta=0.4, **kw)[0]
        assert torch.equal(graph, eager) and bool(torch.isfinite(graph).all()) and not torch.equal(graph, out)
        assert "ddim_variance_noise" in [c[2] for c in pipe._loop.program_shallow.calls]
    finally:
        helper.disable()
