"""Several ControlNets in one inpainting call -- on the GPU.

1. the HIP pipeline with two ControlNets reproduces the reference's own `__call__` (tests/golden/ref_pipeline_call_multicn.pt);
2. `MultiControlNetModel.forward` at the config-4 shape against the fp32 sum of two oracle ControlNets;
3. a wrapper around ONE net is that net: same bits, same launches;
4. the sum formed in the zero convs' epilogues, element by element, on every path such a launch can take;
5. nets whose guidance window is closed are left out of the step, and that changes no bit;
6. scales and windows change between calls on one pipeline object without stale state.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from oracle import sd_modules as OM  # noqa: E402
from powerpaint_amd import models as PM, ops, pipelines as PP, schedulers as PS  # noqa: E402
from powerpaint_amd.engine import Plan  # noqa: E402
from powerpaint_amd.pipelines._loop import DenoiseLoop  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _hip_components(dtype=torch.bfloat16, n_nets=2):
    """The fixture's components on the HIP path: (pipeline keyword arguments, [HIP ControlNets], tokenizer-side inputs)."""
    import make_ref_multi_controlnet as G
    import make_ref_pipeline_call as M
    tok, enc, unet, cn, vae = M.components_cn()
    no_up = {k: v for k, v in M.TINY.items() if k != "up_block_types"}
    hu = PM.UNet2DConditionModel(in_channels=9, device=DEV, dtype=dtype, **M.TINY).load_state_dict(unet.state_dict())
    nets = [PM.ControlNetModel(in_channels=4, device=DEV, dtype=dtype, **no_up).load_state_dict(o.state_dict())
            for o in [cn, G.second_controlnet()][:n_nets]]
    hv = PM.AutoencoderKL(device=DEV, **M.VAE_CFG).load_state_dict(vae.state_dict())
    he = PM.CLIPTextModel(device=DEV, vocab_size=enc.config.vocab_size, num_hidden_layers=1,
                          eos_token_id=enc.config.eos_token_id)
    he.load_state_dict(enc.state_dict())
    return dict(vae=hv, text_encoder=he, tokenizer=tok, unet=hu), nets


def _call(pipe, images, **kw):
    import make_ref_multi_controlnet as G
    import make_ref_pipeline_call as M
    img, mask, lat = M.inputs()
    args = dict(G.CALL_MCN)
    args.update(kw)
    return pipe(image=img, mask=mask, control_image=images, latents=lat.to(DEV), generator=torch.Generator().manual_seed(5),
                output_type="latent", return_dict=False, **args)[0].clone()


def _images():
    import make_ref_multi_controlnet as G
    import make_ref_pipeline_call as M
    return [M.control_image(), G.control_image2()]


# ------------------------------------------------------------------------------------------------ 1
def test_hip_pipeline_with_two_controlnets_reproduces_the_reference_call():
    """Gate: the one tests/test_golden.py applies to the single-net fixture (cosine >= 0.9997, max-abs <= 4.5e-2 *
    max(1, max|ref|)).  Graph replay and eager launches must both pass and give the same bits.
    Achieved values: profiles/multi_controlnet_parity_achieved.txt."""
    import make_ref_multi_controlnet as G
    from test_golden import _close_latents
    gold = torch.load(os.path.join(HERE, "golden", "ref_pipeline_call_multicn.pt"), weights_only=False)
    comp, nets = _hip_components()
    pipe = PP.StableDiffusionControlNetInpaintPipeline(controlnet=nets, scheduler=PS.DDIMScheduler(), **comp)
    assert isinstance(pipe.controlnet, PM.MultiControlNetModel)
    for name, extra in G.CASES.items():
        outs = {}
        for use_graph in (True, False):
            pipe.use_graph = use_graph
            outs[use_graph] = _call(pipe, _images(), **extra)
            cos = torch.nn.functional.cosine_similarity(outs[use_graph].float().cpu().flatten(), gold[name].flatten(), dim=0)
            err = (outs[use_graph].float().cpu() - gold[name]).abs().max()
            print(f"two ControlNets, {name}, {'graph' if use_graph else 'eager'}: cosine {cos.item():.7f} max-abs "
                  f"{err.item():.4g} max|ref| {gold[name].abs().max().item():.4g}")
        for use_graph in (True, False):
            _close_latents(outs[use_graph], gold[name], f"two ControlNets ({name}, {'graph' if use_graph else 'eager'}) vs "
                                                        f"the reference's own __call__")
        assert torch.equal(outs[True], outs[False]), f"{name}: graph replay and eager launches differ"
    pipe.use_graph = True


# ------------------------------------------------------------------------------------------------ 2
def test_multi_controlnet_forward_64x64_against_the_sum_of_two_oracle_nets():
    from test_models_gpu import close
    ocs = []
    for seed in (6, 16):
        torch.manual_seed(seed)
        o = OM.randomize_zero_convs(OM.ControlNetModel(in_channels=4), seed=seed).eval()
        with torch.no_grad():
            for p in o.parameters():
                if p.dim() >= 2:
                    p.copy_(p.to(torch.bfloat16).float())
        ocs.append(o)
    g = torch.Generator("cpu")
    x4 = torch.randn(2, 4, 64, 64, generator=g.manual_seed(61))
    e = torch.randn(2, 77, 768, generator=g.manual_seed(63))
    imgs = [torch.rand(2, 3, 512, 512, generator=g.manual_seed(s)) for s in (64, 65)]
    scales = [0.5, 0.8]
    with torch.no_grad():
        parts = [o(x4, 700, e, im, conditioning_scale=s) for o, im, s in zip(ocs, imgs, scales)]
    ra = [t.float() for t in list(parts[0][0]) + [parts[0][1]]]
    rb = [t.float() for t in list(parts[1][0]) + [parts[1][1]]]
    hcs = [PM.ControlNetModel(in_channels=4, device=DEV).load_state_dict(o.state_dict()) for o in ocs]
    w = PM.MultiControlNetModel(hcs)
    dn, md = w(x4.to(DEV), 700, e.to(DEV), [im.to(DEV) for im in imgs], scales, return_dict=False)
    assert len(dn) == 12
    for i, (h, a, b) in enumerate(zip(list(dn) + [md], ra, rb)):
        ratio = ((a + b).abs().mean() / (a.abs().mean() + b.abs().mean())).item()
        assert ratio > 0.5, f"residual {i}: the two nets cancel (|sum| / (|a| + |b|) = {ratio:.3f}): the cosine would mean little"
        close(h, a + b, f"two ControlNets, 64x64, residual {i} vs fp32 oracle sum", cos_min=0.9998)


# ------------------------------------------------------------------------------------------------ 3
def _names(calls):
    return [c[2] for c in calls]


def test_a_wrapper_around_one_net_is_that_net():
    import make_ref_multi_controlnet as G
    comp, nets = _hip_components(n_nets=1)
    a = nets[0]
    g = torch.Generator("cpu").manual_seed(3)
    x = torch.randn(2, 4, 16, 16, generator=g).to(DEV)
    e = torch.randn(2, 77, 768, generator=g).to(DEV)
    im = torch.rand(2, 3, 128, 128, generator=g).to(DEV)
    dn, md = a(x, 500, e, im, conditioning_scale=0.7, return_dict=False)
    alone = [t.clone() for t in dn + [md]]
    dn, md = PM.MultiControlNetModel([a])(x, 500, e, [im], [0.7], return_dict=False)
    for p, q in zip(alone, dn + [md]):
        assert torch.equal(p, q)
    # the pipeline: same latents, and a step plan with the same launch names in the same order
    extra = dict(G.WINDOWS, control_guidance_start=[0.25], control_guidance_end=[0.75])
    p1 = PP.StableDiffusionControlNetInpaintPipeline(controlnet=a, scheduler=PS.DDIMScheduler(), **comp)
    single = _call(p1, _images()[0], controlnet_conditioning_scale=0.5)
    single_w = _call(p1, _images()[0], controlnet_conditioning_scale=0.5, control_guidance_start=0.25, control_guidance_end=0.75)
    names1 = _names(p1._loop.program.calls)
    pm = PP.StableDiffusionControlNetInpaintPipeline(controlnet=[a], scheduler=PS.DDIMScheduler(), **comp)
    wrapped = _call(pm, _images()[:1], controlnet_conditioning_scale=[0.5])
    wrapped_w = _call(pm, _images()[:1], controlnet_conditioning_scale=[0.5], **extra)
    assert torch.equal(single, wrapped) and torch.equal(single_w, wrapped_w)
    assert not torch.equal(single, single_w)
    assert _names(pm._loop.program.calls) == names1
    assert pm._loop.side_rt is a.rt and not pm._loop._multi


# ------------------------------------------------------------------------------------------------ 4
def _ulp(v, dtype):
    """2^(floor(log2 |v|) - 7) for bf16, - 10 for fp16; 0 at 0."""
    mant = 7 if dtype == torch.bfloat16 else 10
    _, ex = torch.frexp(v.abs().float())                       # |v| = m 2^ex, m in [0.5, 1): floor(log2 |v|) = ex - 1
    u = torch.ldexp(torch.ones_like(v, dtype=torch.float32), ex - 1 - mant)
    return torch.where(v == 0, torch.zeros_like(u), u)


def _assert_one_rounding(multi, ra, rb, dtype, what):
    """|multi - (ra + rb)| <= ulp(rb) / 2 + ulp(max(|multi|, |ra + rb|)), sums in fp32: the epilogue adds the second net's
    UNROUNDED fp32 value (within half an ulp of rb) to ra and rounds once; the reference rounds rb, then the sum."""
    s = ra.float() + rb.float()
    bound = _ulp(rb, dtype) / 2 + _ulp(torch.maximum(multi.float().abs(), s.abs()), dtype)
    diff = (multi.float() - s).abs()
    bad = diff > bound
    assert not bad.any(), (what, int(bad.sum()), float(diff[bad].max()), float(bound[bad].min()))
    assert (multi.float() - ra.float()).abs().max() > 0, what + ": the second net added nothing"


def _tiny_net(seed, dtype):
    import make_ref_pipeline_call as M
    torch.manual_seed(seed)
    o = OM.randomize_zero_convs(M.bf16_(OM.ControlNetModel(
        in_channels=4, **{k: v for k, v in M.TINY.items() if k != "up_block_types"})), seed=seed).eval()
    no_up = {k: v for k, v in M.TINY.items() if k != "up_block_types"}
    return PM.ControlNetModel(in_channels=4, device=DEV, dtype=dtype, **no_up).load_state_dict(o.state_dict())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_epilogue_sum_of_two_nets_element_by_element(dtype):
    """Model level, the routing the plans choose themselves (the staged single-pass epilogue: zero convs are 1x1 GEMMs with
    K <= 1280 and never split on their own), then the `pad_uncond` layout of the pipelines' guess mode."""
    a, b = _tiny_net(71, dtype), _tiny_net(72, dtype)
    g = torch.Generator("cpu").manual_seed(4)
    x = torch.randn(2, 4, 32, 32, generator=g).to(DEV)
    e = torch.randn(2, 77, 768, generator=g).to(DEV)
    ima, imb = (torch.rand(2, 3, 256, 256, generator=g).to(DEV) for _ in range(2))
    for guess in (False, True):
        dn, md = a(x, 300, e, ima, conditioning_scale=0.5, guess_mode=guess, return_dict=False)
        ra = [t.clone() for t in dn + [md]]
        dn, md = b(x, 300, e, imb, conditioning_scale=0.8, guess_mode=guess, return_dict=False)
        rb = [t.clone() for t in dn + [md]]
        dn, md = PM.MultiControlNetModel([a, b])(x, 300, e, [ima, imb], [0.5, 0.8], guess_mode=guess, return_dict=False)
        for i, (m, p, q) in enumerate(zip(dn + [md], ra, rb)):
            _assert_one_rounding(m, p, q, dtype, f"{dtype} guess={guess} residual {i}")
        # the nets' own plans and scales are untouched: each alone gives what it gave
        dn, md = b(x, 300, e, imb, conditioning_scale=0.8, guess_mode=guess, return_dict=False)
        assert all(torch.equal(p, q) for p, q in zip(dn + [md], rb))
    # pad_uncond: residuals in the conditional half of tensors with twice the batch, the unconditional half exactly zero
    outs = []
    for net, im in ((a, ima), (b, imb)):
        rt = net.prepare((2, 4, 32, 32), e, im, 0.6, False, True)
        rt.load_input([(x, 0)])
        rt.set_timestep(300)
        rt.run_step()
        dn, md = net.outputs()
        outs.append([t.clone() for t in dn + [md]])
    rta, rtb = a.rt, b.rt
    plan = Plan()
    ca, keep_a = rta.chained_step_calls(rta, False, 0.6)
    cb, keep_b = rtb.chained_step_calls(rta, True, 0.6)
    assert _names(cb).count("zero_u64") == _names(rtb.step_plan.calls).count("zero_u64") - 1     # (adds in place: no zeroing)
    assert _names(ca) == _names(rta.step_plan.calls)
    plan.calls = ca + cb
    for t in a.outputs()[0] + [a.outputs()[1]]:
        t.fill_(7.0)                                            # (stale values in both halves)
    plan.run(_stream())
    dn, md = a.outputs()
    for i, (m, p, q) in enumerate(zip(dn + [md], outs[0], outs[1])):
        assert m.shape[0] == 4 and not m[:2].any(), f"pad_uncond residual {i}: unconditional half not zero"
        assert not p[:2].any() and not q[:2].any()
        _assert_one_rounding(m[2:], p[2:], q[2:], dtype, f"{dtype} pad_uncond residual {i}")


ZERO_CONV_SHAPES = [(8192, 320), (2048, 640), (512, 1280), (128, 1280)]        # (rows, channels) of SD-1.5 zero convs, batch 2
SPLIT_SHAPES = [(512, 1280), (2048, 640)]       # split-K: whole tiles, >= 5 K-chunks of 64 per split (what the plans also run)
PATHS = [  # (tile, splitk, fuse_combine): every epilogue a plain 16-bit GEMM with res1 can end in
    (0, 0, False),          # what the plans choose for a zero conv: staged single-pass epilogue (K <= 1280 never splits)
    (2, 1, False),          # register-staged (v1) epilogue
    (2, 2, False),          # ... split-K, separate lean combine
    (31, 2, False),         # 128-row tiles x 3 stages, split-K, separate combine
    (54, 2, False),         # 8-wave ping-pong, split-K, separate combine
    (54, 2, True),          # ... the in-kernel share combine where the library advises it
    (54, 4, True),
    (53, 2, True),
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("tile,splitk,fuse", PATHS)
def test_gemm_res1_may_alias_out_on_every_path(dtype, tile, splitk, fuse):
    """include/pp_hip.h "Aliasing": `out = res1 = buffer` gives the bits of the out-of-place launch, and the accumulated
    value obeys the one-rounding bound against the separately rounded product."""
    fused_seen = []
    shapes = ZERO_CONV_SHAPES if splitk <= 1 else [s for s in SPLIT_SHAPES if s[1] // 64 // splitk >= 5]
    assert shapes
    for M, C_ in shapes:
        g = torch.Generator("cpu").manual_seed(M + C_)
        x = torch.randn(M, C_, generator=g).to(DEV, dtype)
        w = (torch.randn(C_, C_, generator=g) * C_ ** -0.5).to(DEV, dtype)
        bias = torch.randn(C_, generator=g).to(DEV)
        ra = torch.randn(M, C_, generator=g).to(DEV, dtype)
        kw = dict(bias=bias, scale=0.8, tile=tile, splitk=splitk, fuse_combine=fuse)
        rb = ops.gemm(x, w, **kw)
        apart = ops.gemm(x, w, res1=ra, **kw)
        buf = ra.clone()
        got = ops.gemm(x, w, res1=buf, out=buf, **kw)
        fused_seen.append(bool(ops.last_combine["fused"]))
        assert got.data_ptr() == buf.data_ptr()
        assert torch.equal(buf, apart), f"in place differs from out of place: {M}x{C_} tile {tile} splitk {splitk}"
        _assert_one_rounding(buf, ra, rb, dtype, f"gemm {M}x{C_} tile {tile} splitk {splitk} fuse {fuse}")
    if fuse:
        print(f"tile {tile} splitk {splitk}: in-kernel combine taken per shape {list(zip(shapes, fused_seen))}")
        assert any(fused_seen), "no shape of this case took the in-kernel combine: the path is not covered"


# ------------------------------------------------------------------------------------------------ 5
def _loop_run(loop, comp_unet, nets, sched_rows, use_graph, steps=4, guess=False, seed=9):
    g = torch.Generator("cpu").manual_seed(seed)
    B, s = 1, 16
    lat = torch.randn(B, 4, s, s, generator=g)
    mask = torch.zeros(B, 1, s, s)
    mask[:, :, 4:12, 4:12] = 1
    mil = torch.randn(B, 4, s, s, generator=g) * 0.5
    pe = torch.randn(2 * B, 77, 768, generator=g).to(DEV)
    imgs = [torch.rand(B, 3, 128, 128, generator=g).to(DEV) for _ in nets]
    loop.scheduler.set_timesteps(steps, device=DEV)
    loop.bind((B, 4, s, s), True, 7.5, pe, prompt_embeds_side=pe, static_inputs=[(mask.to(DEV), 4), (mil.to(DEV), 5)],
              controlnet_cond=imgs, side_scale=[0.5, 0.8][:len(nets)], guess_mode=guess)
    return loop.run(lat.to(DEV), steps, use_graph=use_graph, scale_schedule=sched_rows).clone()


def test_closed_windows_are_skipped_exactly():
    import make_ref_multi_controlnet as G
    comp, nets = _hip_components()
    unet = comp["unet"]
    rows = PP.StableDiffusionControlNetInpaintPipeline.control_schedule(
        4, [0.5, 0.8], G.WINDOWS["control_guidance_start"], G.WINDOWS["control_guidance_end"])
    sets = [tuple(k for k, v in enumerate(r) if v != 0.0) for r in rows]
    assert sets == [(0,), (0, 1), (1,), ()]
    w = PM.MultiControlNetModel(nets)
    for guess in (False, True):
        skip = DenoiseLoop(unet, PS.DDIMScheduler(), side=w, side_kind="controlnet")
        out_skip = _loop_run(skip, unet, nets, rows, use_graph=True, guess=guess)
        assert sorted(skip._sets) == sorted(set(sets) | {(0, 1)})
        unet_names = [c[2] for i, c in enumerate(skip.rt.step_plan.calls) if i not in skip._parts[False]["skips"][id(skip.rt)]]
        tail = _names(skip._parts[False]["tail"])
        heads = skip._parts[False]["heads"]
        for st in set(sets):
            want = []
            for k in st:
                want += _names(heads[id(skip.side_rts[k])])
            want += _names(heads[id(skip.rt)])
            for n, k in enumerate(st):
                rt = skip.side_rts[k]
                body = [c[2] for i, c in enumerate(rt.step_plan.calls) if i not in skip._parts[False]["skips"][id(rt)]]
                if guess and n > 0:
                    body.remove("zero_u64")                     # (the zeroing of the unconditional halves: once per step)
                want += body
            if not st:
                want += ["zero_u64"]
            want += unet_names + tail
            assert _names(skip._sets[st].program[False].calls) == want, st
        # nothing but the networks' own launches (and ONE zeroing launch for the empty set): the sum costs no launch
        assert len(skip._sets[()].program[False].calls) == len(heads[id(skip.rt)]) + 1 + len(unet_names) + len(tail)
        out_skip_eager = _loop_run(skip, unet, nets, rows, use_graph=False, guess=guess)
        keep = DenoiseLoop(unet, PS.DDIMScheduler(), side=w, side_kind="controlnet", keep_closed_nets=True)
        out_keep = _loop_run(keep, unet, nets, rows, use_graph=True, guess=guess)
        for st in keep._sets:
            assert _names(keep._sets[st].program[False].calls) == _names(keep._sets[(0, 1)].program[False].calls)
        assert torch.equal(out_skip, out_keep), f"guess={guess}: skipping closed nets changed the latents"
        assert torch.equal(out_skip, out_skip_eager)
        every = _loop_run(skip, unet, nets, [[0.5, 0.8]] * 4, use_graph=True, guess=guess)
        assert not torch.equal(every, out_skip)


# ------------------------------------------------------------------------------------------------ 6
def test_scales_and_windows_change_between_calls():
    comp, nets = _hip_components()
    pipe = PP.StableDiffusionControlNetInpaintPipeline(controlnet=nets, scheduler=PS.DDIMScheduler(), **comp)
    first = dict(controlnet_conditioning_scale=[0.5, 0.8], control_guidance_start=[0.0, 0.25], control_guidance_end=[0.5, 0.75])
    second = dict(controlnet_conditioning_scale=[0.9, 0.3], control_guidance_start=[0.25, 0.0], control_guidance_end=[1.0, 0.5])
    for use_graph in (True, False):
        pipe.use_graph = use_graph
        o1 = _call(pipe, _images(), **first)
        o2 = _call(pipe, _images(), **second)
        o3 = _call(pipe, _images(), **first)
        assert not torch.equal(o1, o2)
        assert torch.equal(o1, o3), f"use_graph={use_graph}: stale scale, graph or residual after a call with other scales"
    seen = []
    o4 = _call(pipe, _images(), callback=lambda i, t, l: seen.append(i), eta=0.3, **first)      # callback and eta > 0 keep working
    assert seen == [0, 1, 2, 3] and torch.isfinite(o4).all() and not torch.equal(o4, o1)


# ------------------------------------------------------------------------------------------------ 7
def test_two_controlnets_with_a_duck_typed_scheduler():
    """A scheduler that is not one of powerpaint_amd.schedulers (here the oracle's DDIM) drives the same per-set programs:
    the windowed fixture call ({0}, {0, 1}, {1}, {}) within the fixture's gate, graph replay and eager launches alike."""
    import make_ref_multi_controlnet as G
    from oracle import schedulers as OS
    from test_golden import _close_latents
    gold = torch.load(os.path.join(HERE, "golden", "ref_pipeline_call_multicn.pt"), weights_only=False)
    comp, nets = _hip_components()
    pipe = PP.StableDiffusionControlNetInpaintPipeline(controlnet=nets, scheduler=OS.DDIMScheduler(), **comp)
    outs = {}
    for use_graph in (True, False):
        pipe.use_graph = use_graph
        outs[use_graph] = _call(pipe, _images(), **G.WINDOWS)
        assert pipe._loop.foreign and pipe._loop._multi
        _close_latents(outs[use_graph], gold["windows"], f"two ControlNets, windows, duck-typed scheduler "
                                                         f"({'graph' if use_graph else 'eager'})")
    assert torch.equal(outs[True], outs[False])
