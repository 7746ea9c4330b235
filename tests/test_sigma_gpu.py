"""-m gpu: sigma-space sampling on the HIP path -- pp_cfg_sigma_step and pp_step_head_scaled alone, `scheduler.step` of the two
Euler classes against the plain-torch restatement (tests/sigma_cases.py), an audit of every step of the fused loop (the step
arithmetic against the restatement, the networks' output against the oracle UNet fed the SCALED latents), and the v1 / BrushNet
pipelines against the reference's own `__call__`s (tests/golden/ref_sigma.pt).

Achieved numbers are printed and appended to profiles/sigma_parity_achieved.txt before anything is asserted.
"""
import functools
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
import sigma_cases as SC  # noqa: E402
from oracle import loops as OL  # noqa: E402
from oracle import sd_modules as OM  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import models as PM  # noqa: E402
from powerpaint_amd import pipelines as PP  # noqa: E402
from powerpaint_amd import schedulers as PS  # noqa: E402
from powerpaint_amd.pipelines._loop import DenoiseLoop  # noqa: E402
from powerpaint_amd.schedulers import variance_noise  # noqa: E402

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
TINY = dict(block_out_channels=(320, 640), layers_per_block=1,
            down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"))
SD15 = dict(timestep_spacing="leading", steps_offset=1)
U = 2.0 ** -24


def record(line: str):
    print(line)
    try:
        with open(os.path.join(ROOT, "profiles", "sigma_parity_achieved.txt"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def _stream():
    return torch.cuda.current_stream().cuda_stream


def step_close(out, ref, what):
    """The bound of tests/test_lcm_gpu.py's step checks: both sides are the same few fp32 operations,
    |out - ref| <= 1e-4 max(1, max|ref|) + 1e-4 |ref|."""
    out, ref = out.float().cpu(), ref.float().cpu()
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    err = (out - ref).abs()
    tol = 1e-4 * max(1.0, float(ref.abs().max())) + 1e-4 * ref.abs()
    worst = float((err / tol).max())
    assert worst <= 1.0, f"{what}: max abs err {float(err.max()):.4g} (max|ref| {float(ref.abs().max()):.4g}), {worst:.3g} x the bound"
    return worst


# ------------------------------------------------------------------------------------------------ 1. pp_cfg_sigma_step alone
@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("n", [60, 512, 1048636], ids=["n60", "n512", "n1048636"])
def test_pp_cfg_sigma_step_against_the_float64_step(n, cfg):
    """n = 60 (one partial block, not a multiple of 4), 512 (two blocks), 1 048 636 (4097 blocks of work on the 4096-block grid
    cap: the grid-stride loop runs twice for some threads).  Rows 0 (s_up > 0) and 3 (s_up = 0) of a 4-step Euler-ancestral
    table and row 1 of a plain Euler table (s_up = 0, sigma_next > 0), the counter advanced by the ticket and not; where
    s_up = 0 the noise buffer holds NaN.

    Bound, elementwise, with U = 2^-24 per rounded fp32 operation and the table's fp32 (dt, s_up) taken as exact on both sides:
      d = ec - eu: U |d|;  g d: U g |d| more;  e = eu + g d: U |e| <= U (|eu| + g |d|) more  ->  |de| <= U (|eu| + 3 g |d|)
      dt e: |dt| |de| + U |dt e| <= U |dt| (2 |eu| + 4 g |d|);  x + dt e: U (|x| + |dt e|) more;
      s_up z: U |s_up z|, and the last sum U |x'| <= U (|x| + |dt e| + |s_up z|) more.
    Sum <= U (2 |x| + |dt| (4 |eu| + 6 g |d|) + 2 |s_up z|) <= 8 U (|x| + |dt| (|eu| + 2 g |ec - eu|) + |s_up z|), which also
    covers a fused multiply-add contracting any of the products (fewer roundings)."""
    lib = L.lib()
    anc, eul = PS.EulerAncestralDiscreteScheduler(**SD15), PS.EulerDiscreteScheduler(**SD15)
    anc.set_timesteps(4, device=DEV)
    eul.set_timesteps(4, device=DEV)
    g = torch.Generator("cpu").manual_seed(n + cfg)
    gs = 7.5
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst = 0.0
    for sch, row in ((anc, 0), (anc, 3), (eul, 1)):
        dt, s_up = float(sch._coef[row, 1]), float(sch._coef[row, 2])
        assert (s_up > 0) == (sch is anc and row == 0)
        step = sch.step_counter()
        for with_ticket in (True, False):
            x0 = torch.randn(n, generator=g) * 5
            e = torch.randn((2 if cfg else 1) * n, generator=g)
            z = torch.randn(n, generator=g)
            zk = z if s_up > 0 else torch.full_like(z, float("nan"))
            x, ed, zd = x0.to(DEV), e.to(DEV), zk.to(DEV)
            step.fill_(row)
            L.check(lib.pp_cfg_sigma_step(ed.data_ptr(), cfg, gs, x.data_ptr(), zd.data_ptr(), n,
                                          sch.coef_table().data_ptr(), step.data_ptr(),
                                          ticket.data_ptr() if with_ticket else None, _stream()), "sigma step")
            torch.cuda.synchronize()
            assert int(step) == row + (1 if with_ticket else 0) and int(ticket) == 0
            eu = e[:n].double().numpy()
            ec = e[n:].double().numpy() if cfg else None
            ref = SC.step_f64(x0.double().numpy(), eu, ec, z.double().numpy(), gs, dt, s_up)
            d = np.abs(ec - eu) if cfg else 0.0
            bound = 8 * U * (np.abs(x0.double().numpy()) + abs(dt) * (np.abs(eu) + 2 * gs * d) + np.abs(s_up * z.double().numpy()))
            out = x.cpu().double().numpy()
            assert np.isfinite(out).all(), (n, cfg, row, "a NaN from the unread noise buffer reached the output")
            ratio = float((np.abs(out - ref) / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"n {n} cfg {cfg} row {row} ticket {with_ticket}: {ratio:.3g} x the bound"
    record(f"[sigma] kernel n {n} cfg {cfg}: worst err / bound over 3 rows x ticket on, off: {worst:.3g}")
    assert lib.pp_cfg_sigma_step(ed.data_ptr(), cfg, gs, x.data_ptr(), None, n, anc.coef_table().data_ptr(),
                                 anc.step_counter().data_ptr(), None, _stream()) == -1


# ------------------------------------------------------------------------------------------------ 2. pp_step_head_scaled alone
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("hw", [(8, 8), (24, 40)], ids=["8x8", "24x40"])
@pytest.mark.parametrize("c0", [0, 5])
def test_pp_step_head_scaled_is_step_head_on_divided_latents(c0, hw, dtype):
    """x_in = to16(latents / in_div[step]): the library is built without fast-math, so hipcc's fp32 division is the correctly
    rounded one (v_div_scale / v_div_fmas / v_div_fixup), and torch's fp32 division and round-to-nearest-even conversion give
    the same bits: the comparison is exact.  Batch 4 reading 2 latents (wrap), 4 channels into a 9-wide row at offset c0;
    8x8 is one partial block of pixels, 24x40 = 960 pixels x 4 = 15 blocks.  The time-embedding row and the zeroed words are
    those of pp_step_head on the same inputs."""
    B, wrap, C, ldc, rows, steps = 4, 2, 4, 9, 1000, 5
    h, w = hw
    g = torch.Generator("cpu").manual_seed(h + c0)
    table = torch.randn(steps, rows, generator=g).to(DEV)
    lat = (torch.randn(wrap, C, h, w, generator=g) * 6).to(DEV)
    div = (torch.rand(steps, generator=g) * 14 + 1).to(DEV)
    lib = L.lib()
    outs = {}
    for name in ("plain", "scaled"):
        step = torch.tensor([3], dtype=torch.int32, device=DEV)
        temb = torch.full((rows,), -1.0, device=DEV)
        x = torch.full((B, h * w, ldc), 3.0, device=DEV).to(dtype)
        acc = torch.full((777,), 7, dtype=torch.int64, device=DEV)
        args = (table.data_ptr(), step.data_ptr(), temb.data_ptr(), rows, lat.data_ptr(), B, C, h * w, wrap, x.data_ptr(), ldc,
                c0, L.dtype_code(dtype), acc.data_ptr(), acc.numel())
        if name == "plain":
            L.check(lib.pp_step_head(*args, _stream()), "pp_step_head")
        else:
            L.check(lib.pp_step_head_scaled(*args, div.data_ptr(), _stream()), "pp_step_head_scaled")
        torch.cuda.synchronize()
        assert int(step) == 3
        outs[name] = (temb, acc, x)
    assert torch.equal(outs["scaled"][0], outs["plain"][0]) and torch.equal(outs["scaled"][0], table[3])
    assert torch.equal(outs["scaled"][1], outs["plain"][1]) and int(outs["scaled"][1].abs().sum()) == 0
    x = outs["scaled"][2]
    ref = (torch.cat([lat, lat]).cpu() / div[3].cpu()).permute(0, 2, 3, 1).reshape(B, h * w, C).to(dtype)      # (IEEE on the host)
    assert torch.equal(x[:, :, c0:c0 + C].cpu(), ref)
    keep = [j for j in range(ldc) if not c0 <= j < c0 + C]
    assert bool((x[:, :, keep] == 3.0).all())                                        # (the other channels untouched)
    assert torch.equal(outs["plain"][2][:, :, c0:c0 + C], torch.cat([lat, lat]).permute(0, 2, 3, 1).reshape(B, h * w, C).to(dtype))


# ------------------------------------------------------------------------------------------------ 3. scheduler.step
@pytest.mark.parametrize("name", ["EulerDiscreteScheduler", "EulerAncestralDiscreteScheduler"])
def test_scheduler_step_with_twin_generators(name):
    o, h = getattr(SC, name)(**SD15), getattr(PS, name)(**SD15)
    o.set_timesteps(5)
    h.set_timesteps(5, device=DEV)
    assert torch.equal(h.timesteps.cpu(), o.timesteps)
    g = torch.Generator("cpu").manual_seed(0)
    x0 = torch.randn(2, 4, 8, 8, generator=g) * float(o.init_noise_sigma)
    eps = [torch.randn(2, 4, 8, 8, generator=g) for _ in range(5)]
    go, gh = torch.Generator("cpu").manual_seed(7), torch.Generator("cpu").manual_seed(7)
    xo, xh = x0, x0.to(DEV)
    worst = 0.0
    for k, t in enumerate(o.timesteps):
        xo = o.step(eps[k], t, xo, generator=go)[0]
        xh = h.step(eps[k].to(DEV), h.timesteps[k], xh, generator=gh, return_dict=False)[0]
        worst = max(worst, step_close(xh, xo, f"{name}.step {k}"))
    record(f"[sigma] {name}.step over 5 steps: worst err / bound {worst:.3g}")
    assert o.draws == 5
    assert torch.equal(torch.randn(3, generator=go), torch.randn(3, generator=gh))      # same number of draws
    assert h.step(eps[0].to(DEV), h.timesteps[0], x0.to(DEV), generator=gh).prev_sample.shape == x0.shape
    x = torch.randn(2, 4, 8, 8, generator=g)
    assert torch.equal(h.scale_model_input(x.to(DEV), h.timesteps[2]).cpu(), o.scale_model_input(x, o.timesteps[2]))


# ------------------------------------------------------------------------------------------------ 4. the fused loop, step by step
S = 8                                   # 8x8 latents


@functools.lru_cache(maxsize=None)
def _tiny(cin):
    """(oracle UNet with bf16-rounded matrices, the HIP UNet on the same weights)"""
    import make_ref_pipeline_call as MP
    torch.manual_seed(3 + cin)
    o = MP.bf16_(OM.UNet2DConditionModel(in_channels=cin, **TINY)).eval()
    h = PM.UNet2DConditionModel(in_channels=cin, device=DEV, **TINY).load_state_dict(o.state_dict())
    return o, h


def _names(calls):
    return [c[2] for c in calls]


def _pe(B, seed=5):
    return torch.randn(2 * B, 77, 768, generator=torch.Generator("cpu").manual_seed(seed))


def _net_gate(out, ref, what):
    """The network gate of tests/test_golden.py:60 / tests/test_lcm_gpu.py: cosine >= 0.999, max err <= 3e-2 max(1, max|ref|)."""
    out, ref = out.float().cpu(), ref.float().cpu()
    cos = torch.nn.functional.cosine_similarity(out.flatten(), ref.flatten(), dim=0).item()
    err = (out - ref).abs().max().item()
    record(f"[sigma] {what}: cosine {cos:.6f}  max-abs {err:.4g}  (max|ref| {float(ref.abs().max()):.4g})")
    assert cos >= 0.999 and err <= 3e-2 * max(1.0, ref.abs().max().item()), f"{what}: cos {cos:.6f} err {err:.4g}"


def _audit(loop, bind, name, opts, steps, use_graph, what, begin=0, blend=None, run_kw=None, oracle_eps=None, guidance=7.5,
           seed=21):
    """Run the bound loop and, in the per-step callback, redo the step with the restatement on what the loop consumed: the
    eps the step read (the UNet runtime's output), the latents before the step, the noise from a twin generator.  Afterwards
    `oracle_eps(ref scheduler, [latents before every step]) -> [eps of the CFG pair per step]` (oracle.loops.loop_v1 with
    teacher forcing: the oracle networks see `scale_model_input` of exactly the latents the HIP networks saw) is compared with
    the HIP networks' output at the network gate -- unscaled inputs are sigma times too large and miss it by far."""
    sch = loop.scheduler
    total = steps + begin
    sch.set_timesteps(total, device=DEV)
    if begin:
        sch.set_begin_index(begin)
    ref_s = getattr(SC, name)(**opts)
    ref_s.set_timesteps(total)
    assert torch.equal(sch.timesteps.cpu(), ref_s.timesteps)
    g_loop, g_twin = torch.Generator("cpu").manual_seed(seed), torch.Generator("cpu").manual_seed(seed)
    bind(loop, guidance, g_loop)
    lat0 = torch.randn(loop.latents.shape, generator=torch.Generator("cpu").manual_seed(seed + 1)) * float(ref_s.sigmas[begin])
    lat0 = lat0.to(DEV)
    prev, worst, seen, before, raw = [lat0.clone()], [0.0], [], [], []

    def cb(i, t, lat):
        row = begin + i
        eps2 = loop.rt.eps_tensor().clone()
        u, c = eps2.chunk(2)
        eps = u + guidance * (c - u)
        z = variance_noise(lat.shape, g_twin, lat.device, torch.float32)           # one draw per step, both classes
        ref = ref_s.step(eps, ref_s.timesteps[row], prev[0], noise=z)[0]
        if blend is not None:
            x0, mk, nz = (b.to(DEV) for b in blend)
            proper = x0 if row == total - 1 else ref_s.add_noise(x0, nz, ref_s.timesteps[row + 1:row + 2])
            ref = (1 - mk) * proper + mk * ref
        worst[0] = max(worst[0], step_close(lat, ref, f"{what}: step {i} (row {row})"))
        before.append(prev[0].cpu())
        raw.append(eps2.cpu())
        prev[0] = lat.clone()
        seen.append(float(t))

    loop.run(lat0, steps, use_graph=use_graph, callback=cb, timesteps=sch.timesteps[begin:], **(run_kw or {}))
    torch.cuda.synchronize()
    assert seen == ref_s.timesteps[begin:].tolist()
    assert int(sch.step_counter()) == total
    assert torch.equal(torch.randn(3, generator=g_loop), torch.randn(3, generator=g_twin)), "not one draw per step"
    record(f"[sigma] {what}: step arithmetic, worst err / bound {worst[0]:.3g}")
    if oracle_eps is not None:
        fresh = getattr(SC, name)(**opts)
        for i, (got, ref) in enumerate(zip(raw, oracle_eps(fresh, before, total, begin))):
            _net_gate(got, ref, f"{what}: networks' output at step {i}")
    return worst[0]


def _same_launch_count_as_ddim(loop, unet, bind, side=None):
    ddim = DenoiseLoop(unet, PS.DDIMScheduler(), side=side, side_kind="controlnet" if side is not None else None)
    ddim.scheduler.set_timesteps(4, device=DEV)
    bind(ddim, 7.5, None)
    assert len(_names(ddim.program.calls)) == len(_names(loop.program.calls))
    assert _names(ddim.program.calls)[0] == _names(loop.program.calls)[0] == "step_head"


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("name,opts", [("EulerAncestralDiscreteScheduler", SD15),
                                       ("EulerDiscreteScheduler", dict(SD15, use_karras_sigmas=True))],
                         ids=["euler_a", "euler_karras"])
def test_fused_loop_step_by_step(name, opts, use_graph):
    o, unet = _tiny(9)
    B = 2
    shape = (B, 4, S, S)
    g = torch.Generator("cpu").manual_seed(17)
    mask = torch.zeros(B, 1, S, S)
    mask[:, :, 2:6, 1:5] = 1
    mil = torch.randn(B, 4, S, S, generator=g) * 0.5
    pe = _pe(B)

    def bind(loop, guidance, gen):
        loop.bind(shape, True, guidance, pe.to(DEV), static_inputs=[(mask.to(DEV), 4), (mil.to(DEV), 5)], generator=gen)

    def oracle_eps(ref_s, before, total, begin):
        got = []
        OL.loop_v1(o, ref_s, before[0], torch.cat([mask] * 2), torch.cat([mil] * 2), pe, total, 7.5, t_start=begin,
                   eps_hook=lambda i, t, lat, e: got.append(e.clone()), teacher_latents=before,
                   generator=torch.Generator().manual_seed(1))
        return got

    sch = getattr(PS, name)(**opts)
    loop = DenoiseLoop(unet, sch)
    tag = f"{name[:-17]}{' Karras' if opts.get('use_karras_sigmas') else ''}, {'graph' if use_graph else 'eager'}"
    _audit(loop, bind, name, opts, 4, use_graph, f"loop, 4 steps, {tag}", oracle_eps=oracle_eps)
    if opts.get("use_karras_sigmas"):
        assert any(t != round(t) for t in sch.timesteps.tolist()), "fractional timesteps were to be covered"
    names = _names(loop.program.calls)
    assert names.count("cfg_sigma_step") == 1 and names[-1] == "cfg_sigma_step" and names.count("step_head") == 1
    assert not {"ddim_variance_noise", "step_advance", "cfg_sched_step", "cfg_lcm_step", "nchw_to_nhwc"} & set(names)
    assert loop.program.calls[0][0] is L.lib().pp_step_head_scaled and loop._keep[2] is None
    _same_launch_count_as_ddim(loop, unet, bind)
    # strength 0.5 of 8 steps: the loop enters at row 4
    _audit(loop, bind, name, opts, 4, use_graph, f"loop, rows 4..7 of 8, {tag}", begin=4, oracle_eps=oracle_eps)


def test_fused_loop_with_the_4_channel_blend():
    o, unet = _tiny(4)
    B = 2
    g = torch.Generator("cpu").manual_seed(31)
    x0 = torch.randn(1, 4, S, S, generator=g)
    mk = torch.zeros(1, 1, S, S)
    mk[:, :, 2:6, 1:5] = 1
    nz = torch.randn(B, 4, S, S, generator=g)
    pe = _pe(B)
    name = "EulerAncestralDiscreteScheduler"

    def bind(loop, guidance, gen):
        loop.bind((B, 4, S, S), True, guidance, pe.to(DEV), generator=gen, blend=(x0, mk, nz))

    def oracle_eps(ref_s, before, total, begin):
        got = []
        OL.loop_v1(o, ref_s, before[0], torch.cat([mk] * 2), None, pe, total, 7.5, image_latents=x0, noise=nz,
                   eps_hook=lambda i, t, lat, e: got.append(e.clone()), teacher_latents=before,
                   generator=torch.Generator().manual_seed(1))
        return got

    loop = DenoiseLoop(unet, getattr(PS, name)(**SD15))
    for use_graph in (True, False):
        _audit(loop, bind, name, SD15, 4, use_graph, f"loop with the 4-channel blend, {'graph' if use_graph else 'eager'}",
               blend=(x0, mk, nz), oracle_eps=oracle_eps if use_graph else None)
    names = _names(loop.program.calls)
    assert names[-3:] == ["cfg_sigma_step", "latent_blend", "step_advance"]
    tab = loop.scheduler.renoise_table()
    assert torch.equal(tab[:, 1].cpu(), loop.scheduler.sigmas[1:]) and bool((tab[:, 0] == 1).all())
    _same_launch_count_as_ddim(loop, unet, bind)


class _TwoControlNets:
    """Two oracle ControlNets as the reference's MultiControlNetModel sums them (pipeline_PowerPaint_ControlNet.py:1678-1694),
    with this step's per-net scales from the window schedule (a closed window: scale 0)."""

    def __init__(self, nets, conds, rows):
        self.nets, self.conds, self.rows, self.i = nets, conds, rows, 0

    def __call__(self, x, t, encoder_hidden_states, controlnet_cond, conditioning_scale, guess_mode):
        down = mid = None
        for net, cond, sc in zip(self.nets, self.conds, self.rows[self.i]):
            d, m = net(x, t, encoder_hidden_states=encoder_hidden_states, controlnet_cond=cond, conditioning_scale=sc,
                       guess_mode=guess_mode)
            down = list(d) if down is None else [a + b for a, b in zip(down, d)]
            mid = m if mid is None else mid + m
        self.i += 1
        return down, mid


def test_fused_loop_with_two_controlnets_whose_windows_differ():
    import make_ref_multi_controlnet as G
    import make_ref_pipeline_call as M
    from test_multi_controlnet_gpu import _hip_components
    comp, nets = _hip_components()
    unet = comp["unet"]
    _, _, o_unet, o_cn, _ = M.components_cn()
    o_nets = [o_cn, G.second_controlnet()]
    rows = PP.StableDiffusionControlNetInpaintPipeline.control_schedule(
        4, [0.5, 0.8], G.WINDOWS["control_guidance_start"], G.WINDOWS["control_guidance_end"])
    assert len({tuple(k for k, v in enumerate(r) if v != 0.0) for r in rows}) > 2
    g = torch.Generator("cpu").manual_seed(9)
    B = 1
    mask = torch.zeros(B, 1, S, S)
    mask[:, :, 2:6, 2:6] = 1
    mil = torch.randn(B, 4, S, S, generator=g) * 0.5
    imgs = [torch.rand(B, 3, 8 * S, 8 * S, generator=g) for _ in nets]
    pe = _pe(B)
    name = "EulerAncestralDiscreteScheduler"

    def bind(loop, guidance, gen):
        loop.bind((B, 4, S, S), True, guidance, pe.to(DEV), prompt_embeds_side=pe.to(DEV),
                  static_inputs=[(mask.to(DEV), 4), (mil.to(DEV), 5)], controlnet_cond=[i.to(DEV) for i in imgs],
                  side_scale=[0.5, 0.8], generator=gen)

    def oracle_eps(ref_s, before, total, begin):
        got = []
        two = _TwoControlNets(o_nets, [torch.cat([i] * 2) for i in imgs], rows)
        OL.loop_v1(o_unet, ref_s, before[0], torch.cat([mask] * 2), torch.cat([mil] * 2), pe, total, 7.5, controlnet=two,
                   control_image=None, eps_hook=lambda i, t, lat, e: got.append(e.clone()), teacher_latents=before,
                   generator=torch.Generator().manual_seed(1))
        return got

    side = PM.MultiControlNetModel(nets)
    loop = DenoiseLoop(unet, getattr(PS, name)(**SD15), side=side, side_kind="controlnet")
    for use_graph in (True, False):
        _audit(loop, bind, name, SD15, 4, use_graph, f"loop, two ControlNets with windows, {'graph' if use_graph else 'eager'}",
               run_kw=dict(scale_schedule=rows), oracle_eps=oracle_eps if use_graph else None)
    assert len(loop._sets) > 2
    for ent in loop._sets.values():
        names = _names(ent.program[False].calls)
        assert names[-1] == "cfg_sigma_step" and names.count("cfg_sigma_step") == 1 and "step_advance" not in names
        heads = [c for c in ent.program[False].calls if c[2] == "step_head"]
        assert len(heads) == len(ent.included) + 1 and all(c[0] is L.lib().pp_step_head_scaled for c in heads)
    _same_launch_count_as_ddim(loop, unet, bind, side=side)


def test_lab_form_without_the_time_embedding_table_is_refused(monkeypatch):
    _, unet = _tiny(4)
    monkeypatch.setenv("PP_LAB", "1")
    monkeypatch.setenv("PP_TEMB_TABLE", "0")
    sch = PS.EulerDiscreteScheduler()
    sch.set_timesteps(2, device=DEV)
    with pytest.raises(L.PPError):
        DenoiseLoop(unet, sch).bind((1, 4, S, S), True, 7.5, _pe(1).to(DEV))


# ------------------------------------------------------------------------------------------------ 5. the pipelines
# Gate: the defaults of tests/test_golden._close_latents (cosine 0.9997, 4.5e-2 of max(1, max|ref|)), which tests/test_lcm_gpu.py
# applies to the same nets and step counts.  Achieved on MI355X (profiles/sigma_parity_achieved.txt): bf16 cosine >= 0.999855,
# max-abs <= 2.4e-2 of max|ref|; fp16 cosine >= 0.999996, max-abs <= 3.9e-3.


def _fixture():
    return torch.load(os.path.join(HERE, "golden", "ref_sigma.pt"), weights_only=False)


def _against_fixture(out, gen, gold, what):
    from test_golden import _close_latents
    want = gold["latents"]
    cos = torch.nn.functional.cosine_similarity(out.float().cpu().flatten(), want.flatten(), dim=0).item()
    err = (out.float().cpu() - want).abs().max().item()
    record(f"[sigma] {what}: cosine {cos:.6f}  max-abs {err:.4g}  (max|ref| {float(want.abs().max()):.4g}, "
           f"{err / max(1.0, float(want.abs().max())):.3g} of it)")
    assert torch.equal(torch.randn(4, generator=gen), gold["next_draw"]), f"{what}: the generator is not where the reference leaves it"
    _close_latents(out, want, what)


def _product_scheduler(case):
    donor = PS.PNDMScheduler().config                       # the SD-1.5 checkpoint's scheduler config: leading, offset 1
    if case == "dpm_karras":
        return PS.DPMSolverMultistepScheduler.from_config(donor, use_karras_sigmas=True)
    if case == "euler_karras":
        return PS.EulerDiscreteScheduler.from_config(donor, use_karras_sigmas=True)
    return PS.EulerAncestralDiscreteScheduler.from_config(donor)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", ["euler_a", "euler_a_strength", "dpm_karras"])
def test_v1_pipeline_against_the_reference_call(case, dtype):
    import make_ref_lcm as ML
    import make_ref_pipeline_call as MP
    import make_ref_sigma as M
    from test_lcm_gpu import _hip_text_vae
    tok, enc, u9, vae = ML.components("v1")
    he, hv = _hip_text_vae(enc, vae, MP)
    hu = PM.UNet2DConditionModel(in_channels=9, device=DEV, dtype=dtype, **ML.CFG).load_state_dict(u9.state_dict())
    pipe = PP.StableDiffusionInpaintPipeline(vae=hv, text_encoder=he, tokenizer=tok, unet=hu, scheduler=_product_scheduler(case))
    img, mask, _ = MP.inputs()
    g = torch.Generator().manual_seed(M.SEED)
    call = M.CASES[case][3]
    kw = dict(latents=ML.start_latents().to(DEV)) if "strength" not in call else {}
    seen, first = [], []
    out = pipe(image=img, mask=mask, generator=g, output_type="latent", return_dict=False,
               callback=lambda i, t, l: (seen.append(float(t)), first.append(float(l.abs().max()))), **kw, **call)[0]
    ref_s = M.CASES[case][1](**M.CASES[case][2])
    ref_s.set_timesteps(call["num_inference_steps"])
    assert seen == [float(t) for t in ref_s.timesteps[len(ref_s.timesteps) - len(seen):]]
    names = _names(pipe._loop.program.calls)
    assert not pipe._loop.foreign and ("cfg_sched_step" if case == "dpm_karras" else "cfg_sigma_step") in names
    _against_fixture(out, g, _fixture()[case], f"v1 pipeline, {case}, {str(dtype)[6:]}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_brushnet_pipeline_against_the_reference_call(dtype):
    import make_ref_lcm as ML
    import make_ref_pipeline_call as MP
    import make_ref_sigma as M
    from test_lcm_gpu import _hip_text_vae
    case = "euler_karras"
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
    out = pipe(conditioning_latents=cond, latents=ML.start_latents().to(DEV), generator=g, output_type="latent",
               return_dict=False, **M.CASES[case][3])[0]
    names = _names(pipe._loop.program.calls)
    assert not pipe._loop.foreign and names[-1] == "cfg_sigma_step" and names.count("step_head") == 2
    assert all(c[0] is L.lib().pp_step_head_scaled for c in pipe._loop.program.calls if c[2] == "step_head")
    _against_fixture(out, g, _fixture()[case], f"BrushNet pipeline, {case}, {str(dtype)[6:]}")
