"""-m gpu: the fused loop's step launch and `scheduler.step` are the same launch.  For each of the eleven scheduler classes (DDIM
also at eta = 0.5) the loop runs five table rows on a tiny UNet, once eagerly and once through the graph; in the per-step
callback a second instance of the class redoes the row through its public `.step` on what the loop consumed -- the eps the
step read, the latents before the step, a twin generator.  Without CFG both paths hand the kernel the same eps and the same
row, so latents and state must be equal to the bit, and both generators must end at the same place.

Batch 1, latents 8 x 10: n = 320 is two blocks of the step kernel, the second partial, so the ticket hand-off counts more than
one block.  The sigma-space classes cannot be bound at that size: they need the fused head launch to scale the networks' input,
which this tiny UNet's step plan has only where h w is a multiple of 64 (no GroupNorm accumulators to zero otherwise), and then
n = 4 h w is a multiple of the block.  They run at 8 x 16, n = 512: two blocks still, both whole; the partial blocks of their
kernels are in tests/test_sigma_gpu.py and tests/test_ksamplers_gpu.py (n = 60, 61).  Five rows reach both stages of the
two-stage samplers and LMS's full order."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from powerpaint_amd import models as PM  # noqa: E402
from powerpaint_amd import schedulers as PS  # noqa: E402
from powerpaint_amd.pipelines._loop import DenoiseLoop  # noqa: E402

DEV = "cuda"
TINY = dict(block_out_channels=(320, 640), layers_per_block=1,
            down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"))
SD15 = dict(timestep_spacing="leading", steps_offset=1)
H, ROWS = 8, 5
#        class                               options  eta  W   `set_timesteps(N)` with five table rows   step launch   state
CASES = [("DDIMScheduler",                   {},      0.0, 10, 5, "cfg_sched_step",     False),
         ("DDIMScheduler",                   {},      0.5, 10, 5, "cfg_sched_step",     False),
         ("DPMSolverMultistepScheduler",     {},      0.0, 10, 5, "cfg_sched_step",     True),
         ("PNDMScheduler",                   {},      0.0, 10, 4, "cfg_sched_step",     True),      # (its second entry repeats)
         ("UniPCMultistepScheduler",         {},      0.0, 10, 5, "cfg_sched_step",     True),
         ("LCMScheduler",                    {},      0.0, 10, 5, "cfg_lcm_step",       False),
         ("EulerDiscreteScheduler",          SD15,    0.0, 16, 5, "cfg_sigma_step",     False),
         ("EulerAncestralDiscreteScheduler", SD15,    0.0, 16, 5, "cfg_sigma_step",     False),
         ("HeunDiscreteScheduler",           SD15,    0.0, 16, 3, "cfg_ksampler_step",  True),      # (two rows per step)
         ("KDPM2DiscreteScheduler",          SD15,    0.0, 16, 3, "cfg_ksampler_step",  True),
         ("KDPM2AncestralDiscreteScheduler", SD15,    0.0, 16, 3, "cfg_ksampler_step",  True),
         ("LMSDiscreteScheduler",            SD15,    0.0, 16, 5, "cfg_ksampler_step",  True)]
IDS = [f"{c[0][:-9]}{'-eta' if c[2] else ''}" for c in CASES]


@functools.lru_cache(maxsize=None)
def _unet():
    h = PM.UNet2DConditionModel(in_channels=9, device=DEV, **TINY)
    return h.load_state_dict(h.net.synthetic_state_dict(seed=12))


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name,opts,eta,W,steps,launch,stateful", CASES, ids=IDS)
def test_loop_step_equals_scheduler_step_to_the_bit(name, opts, eta, W, steps, launch, stateful, use_graph):
    cls = getattr(PS, name)
    sch, twin = cls(**opts), cls(**opts)
    sch.set_timesteps(steps, device=DEV)
    twin.set_timesteps(steps, device=DEV)
    assert len(sch.timesteps) == ROWS
    g = torch.Generator("cpu").manual_seed(40)
    mask = torch.zeros(1, 1, H, W)
    mask[:, :, 2:6, 3:8] = 1
    mil = torch.randn(1, 4, H, W, generator=g) * 0.5
    pe = torch.randn(1, 77, 768, generator=g)
    lat0 = (torch.randn(1, 4, H, W, generator=g) * float(sch.init_noise_sigma)).to(DEV)
    g_loop, g_twin = torch.Generator("cpu").manual_seed(41), torch.Generator("cpu").manual_seed(41)
    loop = DenoiseLoop(_unet(), sch)
    loop.bind((1, 4, H, W), False, 1.0, pe.to(DEV), static_inputs=[(mask.to(DEV), 4), (mil.to(DEV), 5)], eta=eta,
              generator=g_loop)
    names = [c[2] for c in loop.program.calls]
    assert names.count(launch) == 1 and ("ddim_variance_noise" in names) == (eta > 0)
    assert (loop._keep[2] is not None) == stateful
    assert loop.latents.numel() == 4 * H * W > 256, "more than one block of the step kernel"
    kw = dict(eta=eta) if eta else {}
    prev, rows = [lat0.clone()], []

    def cb(i, t, lat):
        out = twin.step(loop.rt.eps_tensor(), t, prev[0], generator=g_twin, return_dict=False, **kw)[0]
        assert torch.isfinite(lat).all(), f"{name}: non-finite latents after row {i}"
        assert torch.equal(out, lat), f"{name} row {i}: max |loop - step| {float((out - lat).abs().max()):.3g}"
        if stateful:
            assert torch.equal(twin.m_prev(lat), loop._keep[2]), f"{name} row {i}: the state differs"
        prev[0] = lat.clone()
        rows.append(i)

    loop.run(lat0, ROWS, use_graph=use_graph, callback=cb, timesteps=sch.timesteps)
    torch.cuda.synchronize()
    assert rows == list(range(ROWS)) and int(sch.step_counter()) == ROWS
    assert torch.equal(torch.randn(3, generator=g_loop), torch.randn(3, generator=g_twin)), f"{name}: the generators differ"
