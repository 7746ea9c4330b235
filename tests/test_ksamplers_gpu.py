"""-m gpu: Heun, DPM2, DPM2 ancestral and LMS on the HIP path -- pp_cfg_ksampler_step alone against the float64 row formula,
`scheduler.step` of the four classes against the plain-torch restatement (tests/ksampler_cases.py), an audit of every row of
the fused loop (the step arithmetic against the restatement, the networks' output against the oracle UNet fed the SCALED
latents), and the v1 / BrushNet pipelines against the reference's own `__call__`s (tests/golden/ref_ksamplers.pt).

Achieved numbers are printed and appended to profiles/ksampler_parity_achieved.txt before anything is asserted.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import ksampler_cases as KC  # noqa: E402
from oracle import loops as OL  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import models as PM  # noqa: E402
from powerpaint_amd import pipelines as PP  # noqa: E402
from powerpaint_amd import schedulers as PS  # noqa: E402
from powerpaint_amd.pipelines._loop import DenoiseLoop  # noqa: E402
from test_sigma_gpu import S, SD15, _names, _pe, _tiny  # noqa: E402

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
NAMES = list(KC.CLASSES)


def record(line: str):
    print(line)
    try:
        with open(os.path.join(ROOT, "profiles", "ksampler_parity_achieved.txt"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def _stream():
    return torch.cuda.current_stream().cuda_stream


def step_close(out, ref, what):
    """The bound of tests/test_sigma_gpu.py:60: both sides are the same few fp32 operations (here at most 6 multiply-adds),
    |out - ref| <= 1e-4 max(1, max|ref|) + 1e-4 |ref|."""
    out, ref = out.double().cpu(), ref.double().cpu()
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    err = (out - ref).abs()
    tol = 1e-4 * max(1.0, float(ref.abs().max())) + 1e-4 * ref.abs()
    worst = float((err / tol).max())
    assert worst <= 1.0, f"{what}: max abs err {float(err.max()):.4g} (max|ref| {float(ref.abs().max()):.4g}), {worst:.3g} x the bound"
    return worst


# ------------------------------------------------------------------------------------------------ 1. pp_cfg_ksampler_step alone
#        c_e    c_h1  c_h2   c_h3   s_up  sigma  s1 s2 s3 push use_saved save
ROWS = [[-1.25, 0.0,  0.0,   0.0,   0.0,  3.0,   0, 0, 0, -1,  0,        0],      # plain
        [-0.75, 0.0,  0.0,   0.0,   0.0,  2.0,   0, 0, 0,  1,  0,        1],      # save + push
        [-0.5,  -0.5, 0.0,   0.0,   0.0,  1.5,   1, 0, 0, -1,  1,        0],      # use_saved + one history slot
        [-0.9,  0.55, -0.12, 0.006, 0.0,  1.0,   1, 0, 2,  2,  0,        0],      # three slots, push into a slot it read
        [-1.7,  0.0,  0.0,   0.0,   1.05, 0.8,   0, 0, 0, -1,  1,        0]]      # s_up != 0 (from the saved sample)


@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("n", [61, 512, 1048637], ids=["n61", "n512", "n1048637"])
def test_pp_cfg_ksampler_step_against_the_float64_row_formula(n, cfg):
    """n = 61 (an odd tail below one block), 512 (two whole blocks), 1 048 637 (more work than the 4096-block grid covers in one
    pass, with an odd tail: the grid-stride loop runs twice for some threads).  Every row type, the counter advanced by the
    ticket and not; where s_up = 0 the noise buffer holds NaN, so a finite output proves it was not read.  State slots and the
    saved sample a row must not write, and everything past the row's own update, are compared exactly."""
    lib = L.lib()
    table = torch.zeros(len(ROWS), 16)
    table[:, :12] = torch.tensor(ROWS, dtype=torch.float32)
    tab_d = table.to(DEV)
    g = torch.Generator("cpu").manual_seed(n + cfg)
    gs = 7.5
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst = 0.0
    for r, row in enumerate(table.double().numpy()):
        for with_ticket in (True, False):
            x0 = torch.randn(n, generator=g) * 5
            st0 = torch.randn(4, n, generator=g)
            e = torch.randn((2 if cfg else 1) * n, generator=g)
            z = torch.randn(n, generator=g)
            zk = z if row[4] != 0 else torch.full_like(z, float("nan"))
            x, st, ed, zd = x0.to(DEV), st0.to(DEV), e.to(DEV), zk.to(DEV)
            step.fill_(r)
            L.check(lib.pp_cfg_ksampler_step(ed.data_ptr(), cfg, gs, x.data_ptr(), st.data_ptr(), zd.data_ptr(), n,
                                             tab_d.data_ptr(), step.data_ptr(), ticket.data_ptr() if with_ticket else None,
                                             _stream()), "ksampler step")
            torch.cuda.synchronize()
            assert int(step) == r + (1 if with_ticket else 0) and int(ticket) == 0
            ev = e.double().numpy()
            e64 = ev[:n] + gs * (ev[n:] - ev[:n]) if cfg else ev
            H = [st0[k].double().numpy() for k in range(3)]
            ref, saved, H2 = KC.row_f64(x0.double().numpy(), st0[3].double().numpy(), H, e64, z.double().numpy(), row)
            out = x.cpu()
            assert bool(torch.isfinite(out).all()), (n, cfg, r, "a NaN from the unread noise buffer reached the output")
            worst = max(worst, step_close(out, torch.from_numpy(ref), f"n {n} cfg {cfg} row {r} ticket {with_ticket}"))
            got = st.cpu()
            push = int(row[9])
            for k in range(3):
                if k == push:                      # e itself: the guidance combine is 2 fp32 operations on top of |eu|, g |d|
                    step_close(got[k], torch.from_numpy(e64), f"row {r}: pushed derivative")
                    if not cfg:
                        assert torch.equal(got[k], e)
                else:
                    assert torch.equal(got[k], st0[k]), f"row {r} wrote history slot {k}"
            assert torch.equal(got[3], x0 if row[11] else st0[3]), f"row {r}: saved sample"
            assert torch.equal(ed.cpu(), e) and (row[4] == 0 or torch.equal(zd.cpu(), z))
    record(f"[ksampler] kernel n {n} cfg {cfg}: worst err / bound over {len(ROWS)} rows x ticket on, off: {worst:.3g}")
    for bad in ((ed.data_ptr(), cfg, gs, x.data_ptr(), None, zd.data_ptr(), n), (ed.data_ptr(), cfg, gs, x.data_ptr(), st.data_ptr(), None, n),
                (ed.data_ptr(), cfg, gs, x.data_ptr(), st.data_ptr(), zd.data_ptr(), 0)):
        assert lib.pp_cfg_ksampler_step(*bad, tab_d.data_ptr(), step.data_ptr(), None, _stream()) == -1


# ------------------------------------------------------------------------------------------------ 2. scheduler.step
@pytest.mark.parametrize("karras", [False, True], ids=["plain", "karras"])
@pytest.mark.parametrize("name", NAMES)
def test_scheduler_step_with_twin_generators(name, karras):
    opts = dict(SD15, use_karras_sigmas=karras)
    o, h = KC.CLASSES[name](**opts), getattr(PS, name)(**opts)
    o.set_timesteps(4)
    h.set_timesteps(4, device=DEV)
    assert torch.equal(h.timesteps.cpu(), o.timesteps)
    rows = len(o.timesteps)
    assert rows == (4 if name == "LMSDiscreteScheduler" else 7)
    g = torch.Generator("cpu").manual_seed(0)
    x0 = torch.randn(1, 4, 8, 8, generator=g) * float(o.init_noise_sigma)
    eps = [torch.randn(1, 4, 8, 8, generator=g) for _ in range(rows)]
    go, gh = torch.Generator("cpu").manual_seed(7), torch.Generator("cpu").manual_seed(7)
    xo, xh = x0, x0.to(DEV)
    worst = 0.0
    x = torch.randn(1, 4, 8, 8, generator=g)
    for k, t in enumerate(o.timesteps):
        assert torch.equal(h.scale_model_input(x.to(DEV), h.timesteps[k]).cpu(), o.scale_model_input(x, t)), k
        xo = o.step(eps[k], t, xo, generator=go)[0]
        new = h.step(eps[k].to(DEV), h.timesteps[k], xh, generator=gh, return_dict=False)[0]
        assert new.data_ptr() != xh.data_ptr()                                          # a new tensor
        xh = new
        worst = max(worst, step_close(xh, xo, f"{name}.step row {k}"))
    record(f"[ksampler] {name}{' Karras' if karras else ''}.step over {rows} rows: worst err / bound {worst:.3g}")
    assert o.draws == (rows if name == "KDPM2AncestralDiscreteScheduler" else 0)
    assert torch.equal(torch.randn(3, generator=go), torch.randn(3, generator=gh))      # same number of draws
    h.set_timesteps(4, device=DEV)                                                      # state and call counts restart
    assert h.step(eps[0].to(DEV), h.timesteps[0], x0.to(DEV), generator=gh).prev_sample.shape == x0.shape


# ------------------------------------------------------------------------------------------------ 3. the fused loop, row by row
def _net_gate(out, ref, what):
    """The network gate of tests/test_sigma_gpu.py:210: cosine >= 0.999, max err <= 3e-2 max(1, max|ref|)."""
    out, ref = out.float().cpu(), ref.float().cpu()
    cos = torch.nn.functional.cosine_similarity(out.flatten(), ref.flatten(), dim=0).item()
    err = (out - ref).abs().max().item()
    record(f"[ksampler] {what}: cosine {cos:.6f}  max-abs {err:.4g}  (max|ref| {float(ref.abs().max()):.4g})")
    assert cos >= 0.999 and err <= 3e-2 * max(1.0, ref.abs().max().item()), f"{what}: cos {cos:.6f} err {err:.4g}"


def _audit(loop, bind, name, opts, steps, use_graph, what, t_start=0, blend=None, oracle_eps=None, guidance=7.5, seed=21):
    """Run the bound loop over the rows of `steps` sampler steps entered at step `t_start` and, in the per-row callback, redo
    the row with the restatement on what the loop consumed: the eps the step read (the UNet runtime's output), the latents
    before the row, the noise from a twin generator.  Afterwards `oracle_eps(fresh restatement, [latents before every row])`
    (oracle.loops.loop_v1 with teacher forcing: the oracle networks see `scale_model_input` of exactly the latents the HIP
    networks saw, at the row's own -- possibly fractional -- timestep) is compared with the HIP networks' output."""
    sch = loop.scheduler
    sch.set_timesteps(steps, device=DEV)
    begin = t_start * sch.order
    if begin:
        sch.set_begin_index(begin)
    ref_s = KC.CLASSES[name](**opts)
    ref_s.set_timesteps(steps)
    assert torch.equal(sch.timesteps.cpu(), ref_s.timesteps)
    total = len(ref_s.timesteps)
    g_loop, g_twin = torch.Generator("cpu").manual_seed(seed), torch.Generator("cpu").manual_seed(seed)
    bind(loop, guidance, g_loop)
    lat0 = torch.randn(loop.latents.shape, generator=torch.Generator("cpu").manual_seed(seed + 1)) * float(sch._row_sigma[begin])
    lat0 = lat0.to(DEV)
    prev, worst, seen, before, raw = [lat0.clone()], [0.0], [], [], []

    def cb(i, t, lat):
        row = begin + i
        eps2 = loop.rt.eps_tensor().clone()
        u, c = eps2.chunk(2)
        eps = u + guidance * (c - u)
        ref = ref_s.step(eps, ref_s.timesteps[row], prev[0], generator=g_twin)[0]
        if blend is not None:
            x0, mk, nz = (b.to(DEV) for b in blend)
            proper = x0 if row == total - 1 else ref_s.add_noise(x0, nz, ref_s.timesteps[row + 1:row + 2])
            ref = (1 - mk) * proper + mk * ref
        worst[0] = max(worst[0], step_close(lat, ref, f"{what}: row {row}"))
        before.append(prev[0].cpu())
        raw.append(eps2.cpu())
        prev[0] = lat.clone()
        seen.append(float(t))

    loop.run(lat0, total - begin, use_graph=use_graph, callback=cb, timesteps=sch.timesteps[begin:])
    torch.cuda.synchronize()
    assert seen == ref_s.timesteps[begin:].tolist(), "the rows' timesteps are the interleaved list"
    assert int(sch.step_counter()) == total
    assert torch.equal(torch.randn(3, generator=g_loop), torch.randn(3, generator=g_twin)), "the draws differ from the restatement's"
    record(f"[ksampler] {what}: step arithmetic over {total - begin} rows, worst err / bound {worst[0]:.3g}")
    if oracle_eps is not None:
        fresh = KC.CLASSES[name](**opts)
        for i, (got, ref) in enumerate(zip(raw, oracle_eps(fresh, before, steps, t_start))):
            _net_gate(got, ref, f"{what}: networks' output at row {begin + i}")
    return seen


def _same_launch_count_as_euler(loop, unet, bind):
    eul = DenoiseLoop(unet, PS.EulerDiscreteScheduler(**SD15))
    eul.scheduler.set_timesteps(4, device=DEV)
    bind(eul, 7.5, None)
    assert len(_names(eul.program.calls)) == len(_names(loop.program.calls))
    assert _names(eul.program.calls)[0] == _names(loop.program.calls)[0] == "step_head"


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("name,karras", [("HeunDiscreteScheduler", False), ("KDPM2DiscreteScheduler", False),
                                         ("KDPM2AncestralDiscreteScheduler", False), ("LMSDiscreteScheduler", True)],
                         ids=["heun", "dpm2", "dpm2_a", "lms_karras"])
def test_fused_loop_row_by_row(name, karras, use_graph):
    """8x8 latents, batch 2, 4 sampler steps (7 network evaluations for the two-stage classes); `_tiny` stores bf16."""
    o, unet = _tiny(9)
    B = 2
    shape = (B, 4, S, S)
    g = torch.Generator("cpu").manual_seed(17)
    mask = torch.zeros(B, 1, S, S)
    mask[:, :, 2:6, 1:5] = 1
    mil = torch.randn(B, 4, S, S, generator=g) * 0.5
    pe = _pe(B)
    opts = dict(SD15, use_karras_sigmas=karras)

    def bind(loop, guidance, gen):
        loop.bind(shape, True, guidance, pe.to(DEV), static_inputs=[(mask.to(DEV), 4), (mil.to(DEV), 5)], generator=gen)

    def oracle_eps(ref_s, before, steps, t_start):
        got = []
        OL.loop_v1(o, ref_s, before[0], torch.cat([mask] * 2), torch.cat([mil] * 2), pe, steps, 7.5, t_start=t_start,
                   eps_hook=lambda i, t, lat, e: got.append(e.clone()), teacher_latents=before,
                   generator=torch.Generator().manual_seed(1))
        return got

    sch = getattr(PS, name)(**opts)
    loop = DenoiseLoop(unet, sch)
    tag = f"{name[:-9]}{' Karras' if karras else ''}, {'graph' if use_graph else 'eager'}"
    seen = _audit(loop, bind, name, opts, 4, use_graph, f"loop, 4 steps, {tag}", oracle_eps=oracle_eps)
    assert len(seen) == (4 if sch.order == 1 else 7)
    if name == "KDPM2DiscreteScheduler" or karras:
        assert any(t != round(t) for t in seen), "fractional timesteps were to be covered"
    names = _names(loop.program.calls)
    assert names.count("cfg_ksampler_step") == 1 and names[-1] == "cfg_ksampler_step" and names.count("step_head") == 1
    assert not {"ddim_variance_noise", "step_advance", "cfg_sched_step", "cfg_sigma_step", "nchw_to_nhwc"} & set(names)
    assert loop.program.calls[0][0] is L.lib().pp_step_head_scaled
    assert tuple(loop._keep[2].shape) == (4,) + shape
    _same_launch_count_as_euler(loop, unet, bind)
    if sch.order == 2:          # strength 0.5 of 4 steps: the loop enters at row 4, a first stage, with an empty state
        _audit(loop, bind, name, opts, 4, use_graph, f"loop, rows 4..6 of 7, {tag}", t_start=2, oracle_eps=oracle_eps)


@pytest.mark.parametrize("dtype", [torch.float16], ids=["fp16"])
def test_fused_loop_in_fp16(dtype):
    """The same audit with the networks in fp16 (the parametrised test above runs the cached bf16 net): Heun, graph."""
    from test_sigma_gpu import TINY
    o, _ = _tiny(9)
    unet = PM.UNet2DConditionModel(in_channels=9, device=DEV, dtype=dtype, **TINY).load_state_dict(o.state_dict())
    B = 2
    g = torch.Generator("cpu").manual_seed(17)
    mask = torch.zeros(B, 1, S, S)
    mask[:, :, 2:6, 1:5] = 1
    mil = torch.randn(B, 4, S, S, generator=g) * 0.5
    pe = _pe(B)

    def bind(loop, guidance, gen):
        loop.bind((B, 4, S, S), True, guidance, pe.to(DEV), static_inputs=[(mask.to(DEV), 4), (mil.to(DEV), 5)], generator=gen)

    def oracle_eps(ref_s, before, steps, t_start):
        got = []
        OL.loop_v1(o, ref_s, before[0], torch.cat([mask] * 2), torch.cat([mil] * 2), pe, steps, 7.5, t_start=t_start,
                   eps_hook=lambda i, t, lat, e: got.append(e.clone()), teacher_latents=before)
        return got

    for name in ("HeunDiscreteScheduler", "KDPM2AncestralDiscreteScheduler"):
        loop = DenoiseLoop(unet, getattr(PS, name)(**SD15))
        _audit(loop, bind, name, SD15, 4, True, f"loop, 4 steps, {name[:-9]}, fp16 networks, graph",
               oracle_eps=oracle_eps if name == "HeunDiscreteScheduler" else None)


def test_fused_loop_with_the_4_channel_blend_heun_and_the_kdpm2_refusal():
    o, unet = _tiny(4)
    B = 2
    g = torch.Generator("cpu").manual_seed(31)
    x0 = torch.randn(1, 4, S, S, generator=g)
    mk = torch.zeros(1, 1, S, S)
    mk[:, :, 2:6, 1:5] = 1
    nz = torch.randn(B, 4, S, S, generator=g)
    pe = _pe(B)

    def bind(loop, guidance, gen):
        loop.bind((B, 4, S, S), True, guidance, pe.to(DEV), generator=gen, blend=(x0, mk, nz))

    def oracle_eps(ref_s, before, steps, t_start):
        got = []
        OL.loop_v1(o, ref_s, before[0], torch.cat([mk] * 2), None, pe, steps, 7.5, image_latents=x0, noise=nz,
                   eps_hook=lambda i, t, lat, e: got.append(e.clone()), teacher_latents=before)
        return got

    for name in ("HeunDiscreteScheduler", "LMSDiscreteScheduler"):
        loop = DenoiseLoop(unet, getattr(PS, name)(**SD15))
        for use_graph in (True, False):
            _audit(loop, bind, name, SD15, 4, use_graph,
                   f"loop with the 4-channel blend, {name[:-9]}, {'graph' if use_graph else 'eager'}", blend=(x0, mk, nz),
                   oracle_eps=oracle_eps if (use_graph and name == "HeunDiscreteScheduler") else None)
        names = _names(loop.program.calls)
        assert names[-3:] == ["cfg_ksampler_step", "latent_blend", "step_advance"]
        tab = loop.scheduler.renoise_table().cpu()
        sg = loop.scheduler._row_sigma
        assert torch.equal(tab[:-1, 1], sg[1:]) and tab[-1, 1] == 0 and bool((tab[:, 0] == 1).all())      # sigma of the NEXT row
    for name in ("KDPM2DiscreteScheduler", "KDPM2AncestralDiscreteScheduler"):
        sch = getattr(PS, name)(**SD15)
        sch.set_timesteps(4, device=DEV)
        with pytest.raises(L.PPError, match=name + ".*add_noise at a midpoint timestep is not pinned"):
            bind(DenoiseLoop(unet, sch), 7.5, None)


# ------------------------------------------------------------------------------------------------ 4. the pipelines
# Gate: the defaults of tests/test_golden._close_latents (cosine 0.9997, 4.5e-2 of max(1, max|ref|)), which tests/test_sigma_gpu.py
# applies to the same nets.


def _fixture():
    return torch.load(os.path.join(HERE, "golden", "ref_ksamplers.pt"), weights_only=False)


def _against_fixture(out, gen, gold, what):
    from test_golden import _close_latents
    want = gold["latents"]
    cos = torch.nn.functional.cosine_similarity(out.float().cpu().flatten(), want.flatten(), dim=0).item()
    err = (out.float().cpu() - want).abs().max().item()
    record(f"[ksampler] {what}: cosine {cos:.6f}  max-abs {err:.4g}  (max|ref| {float(want.abs().max()):.4g}, "
           f"{err / max(1.0, float(want.abs().max())):.3g} of it)")
    assert torch.equal(torch.randn(4, generator=gen), gold["next_draw"]), f"{what}: the generator is not where the reference leaves it"
    _close_latents(out, want, what)


def _product_scheduler(case):
    import make_ref_ksamplers as M
    donor = PS.PNDMScheduler().config                       # the SD-1.5 checkpoint's scheduler config: leading, offset 1
    cls = getattr(PS, M.CASES[case][1].__name__)
    return cls.from_config(donor, use_karras_sigmas=bool(M.CASES[case][2].get("use_karras_sigmas", False)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", ["heun", "heun_karras_strength", "dpm2_a"])
def test_v1_pipeline_against_the_reference_call(case, dtype):
    import make_ref_ksamplers as M
    import make_ref_lcm as ML
    import make_ref_pipeline_call as MP
    from test_lcm_gpu import _hip_text_vae
    tok, enc, u9, vae = ML.components("v1")
    he, hv = _hip_text_vae(enc, vae, MP)
    hu = PM.UNet2DConditionModel(in_channels=9, device=DEV, dtype=dtype, **ML.CFG).load_state_dict(u9.state_dict())
    pipe = PP.StableDiffusionInpaintPipeline(vae=hv, text_encoder=he, tokenizer=tok, unet=hu, scheduler=_product_scheduler(case))
    img, mask, _ = MP.inputs()
    g = torch.Generator().manual_seed(M.SEED)
    call = M.CASES[case][3]
    kw = dict(latents=ML.start_latents().to(DEV)) if "strength" not in call else {}
    seen = []
    out = pipe(image=img, mask=mask, generator=g, output_type="latent", return_dict=False,
               callback=lambda i, t, l: seen.append((i, float(t))), **kw, **call)[0]
    ref_s = M.CASES[case][1](**M.CASES[case][2])
    ref_s.set_timesteps(call["num_inference_steps"])
    rows = ref_s.timesteps.tolist()
    begin = 0 if "strength" not in call else 2 * (call["num_inference_steps"] - int(call["num_inference_steps"] * call["strength"]))
    run = rows[begin:]
    # the legacy callback fires after a step's second evaluation and after the last row (pipeline_PowerPaint.py:1038)
    assert seen == [(i, t) for i, t in enumerate(run) if i == len(run) - 1 or (i + 1) % 2 == 0]
    assert int(pipe.scheduler.step_counter()) == len(rows)
    names = _names(pipe._loop.program.calls)
    assert not pipe._loop.foreign and names[-1] == "cfg_ksampler_step"
    _against_fixture(out, g, _fixture()[case], f"v1 pipeline, {case}, {str(dtype)[6:]}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", ["dpm2", "lms_karras"])
def test_brushnet_pipeline_against_the_reference_call(case, dtype):
    import make_ref_ksamplers as M
    import make_ref_lcm as ML
    import make_ref_pipeline_call as MP
    from test_lcm_gpu import _hip_text_vae
    tok, enc, u4, bn, vae = ML.components("v2")
    he, hv = _hip_text_vae(enc, vae, MP)
    hu = PM.UNet2DConditionModel(in_channels=4, device=DEV, dtype=dtype, **ML.CFG).load_state_dict(u4.state_dict())
    hb = PM.BrushNetModel(in_channels=4, conditioning_channels=5, device=DEV, dtype=dtype, **ML.CFG).load_state_dict(bn.state_dict())
    pipe = PP.StableDiffusionPowerPaintBrushNetPipeline(vae=hv, text_encoder=he, text_encoder_brushnet=he, tokenizer=tok,
                                                        unet=hu, brushnet=hb, scheduler=_product_scheduler(case))
    img, mask3, _ = MP.inputs_v2()
    rep = torch.cat([img.repeat(M.NB, 1, 1, 1)] * 2)
    dist = hv.encode(rep.to(DEV)).latent_dist
    torch.manual_seed(9)
    noise = torch.randn(dist.mean.shape)                          # CPU global RNG, as in the reference run
    cl = (dist.mean + dist.std * noise.to(DEV)) * hv.config.scaling_factor
    keep = (torch.cat([mask3.repeat(M.NB, 1, 1, 1)] * 2).sum(1)[:, None] < 0).float()
    cond = torch.cat([cl, torch.nn.functional.interpolate(keep, size=cl.shape[-2:]).to(DEV)], 1)
    g = torch.Generator().manual_seed(M.SEED)
    per_row = []
    out = pipe(conditioning_latents=cond, latents=ML.start_latents().to(DEV), generator=g, output_type="latent",
               return_dict=False, callback_on_step_end=lambda p, i, t, kw: per_row.append(float(t)), **M.CASES[case][3])[0]
    ref_s = M.CASES[case][1](**M.CASES[case][2])
    ref_s.set_timesteps(M.CASES[case][3]["num_inference_steps"])
    assert per_row == ref_s.timesteps.tolist()                    # callback_on_step_end: after every row
    assert any(t != round(t) for t in per_row)
    names = _names(pipe._loop.program.calls)
    assert not pipe._loop.foreign and names[-1] == "cfg_ksampler_step" and names.count("step_head") == 2
    assert all(c[0] is L.lib().pp_step_head_scaled for c in pipe._loop.program.calls if c[2] == "step_head")
    _against_fixture(out, g, _fixture()[case], f"BrushNet pipeline, {case}, {str(dtype)[6:]}")
