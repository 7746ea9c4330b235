"""CPU: LCMScheduler (kind 4) -- schedules, coefficient rows, the step kernel's arithmetic emulated on the host, config
handling and loading, the ABI entry, the guidance-embedded UNet's config and the guidance-scale embedding."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lcm_cases as LC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import schedulers as PS  # noqa: E402

LISTS = {1: [999], 2: [999, 499], 4: [999, 759, 499, 259], 6: [999, 839, 679, 499, 339, 179],
         8: [999, 879, 759, 639, 499, 379, 259, 139]}


# ------------------------------------------------------------------------------------------------ schedules and rows
@pytest.mark.parametrize("N", sorted(LISTS))
def test_timestep_lists(N):
    s, r = PS.LCMScheduler(), LC.LCMScheduler()
    s.set_timesteps(N)
    r.set_timesteps(N)
    assert s.timesteps.tolist() == LISTS[N] == r.timesteps.tolist()
    assert s.num_inference_steps == N and s.order == 1 and s.init_noise_sigma == 1.0 and s.kind == 4
    x = torch.randn(1, 4, 2, 2)
    assert s.scale_model_input(x, s.timesteps[0]) is x


def test_other_schedules_and_every_value_error():
    s, r = PS.LCMScheduler(), LC.LCMScheduler()
    s.set_timesteps(4, original_inference_steps=100)
    r.set_timesteps(4, original_inference_steps=100)
    assert s.timesteps.tolist() == r.timesteps.tolist() == [999, 749, 499, 249]
    s.set_timesteps(4, strength=0.5)                       # origin = 19, 39 .. 499 reversed; indices 0, 6, 12, 18
    r.set_timesteps(4, strength=0.5)
    assert s.timesteps.tolist() == r.timesteps.tolist() == [499, 379, 259, 139]
    s.set_timesteps(timesteps=[999, 600, 301, 7])          # a custom list is taken as given
    assert s.timesteps.tolist() == [999, 600, 301, 7] and s.custom_timesteps and s.num_inference_steps == 4
    s.set_timesteps(timesteps=[999, 600, 301, 7], strength=0.5)      # ... and then truncated: timesteps[4 - int(4 * 0.5):]
    r.set_timesteps(timesteps=[999, 600, 301, 7], strength=0.5)
    assert s.timesteps.tolist() == r.timesteps.tolist() == [301, 7]
    s.set_timesteps(2)
    assert not s.custom_timesteps and s.timesteps.tolist() == LISTS[2]
    for kw in (dict(num_inference_steps=4, original_inference_steps=1001),        # original_steps > T
               dict(num_inference_steps=1001, original_inference_steps=1000),     # num_inference_steps > T
               dict(num_inference_steps=51),                                      # num_inference_steps > original_steps
               dict(num_inference_steps=8, strength=0.1),                         # len(origin) // N < 1  (5 // 8)
               dict(),                                                            # neither a count nor a list
               dict(num_inference_steps=4, timesteps=[999, 499]),                 # both
               dict(timesteps=[499, 999]), dict(timesteps=[999, 999]),            # not descending
               dict(timesteps=[1000, 499]),                                       # first >= T
               dict(timesteps=[999.5, 499])):                                     # not integers
        with pytest.raises(ValueError):
            s.set_timesteps(**kw)


@pytest.mark.parametrize("scaling", [10.0, 0.001])
def test_table_rows_against_the_float64_formulas(scaling):
    s = PS.LCMScheduler(timestep_scaling=scaling)
    for N in (1, 4, 8):
        s.set_timesteps(N)
        ts = s.timesteps.tolist()
        assert tuple(s._coef.shape) == (N, 8) and s._coef.dtype == torch.float32
        for i, t in enumerate(ts):
            last = i == N - 1
            want = LC.row_f64(t, t if last else ts[i + 1], last, scaling)
            got = s._coef[i].double().numpy()
            # fp32 sqrt / divide of fp32 inputs: a few ulp of the value; c_skip ~ 1e-8 at the default scaling, hence relative
            assert np.allclose(got, want, rtol=2e-6, atol=0), (N, i, got, want)
        assert s._coef[-1, 4] == 1.0 and s._coef[-1, 5] == 0.0
    s.set_timesteps(8)
    full = s._coef.clone()
    s.set_begin_index(4)                                    # strength 0.5 through get_timesteps: only the counter moves
    assert torch.equal(s._coef, full) and s.begin_index == 4 and s.timesteps.tolist() == LISTS[8]
    assert [s.draws_noise_at(i) for i in range(8)] == [True] * 7 + [False] and s.step_noise
    assert not PS.DDIMScheduler().step_noise and PS.DDIMScheduler().set_eta(0.5).step_noise
    assert not PS.UniPCMultistepScheduler().step_noise


# ------------------------------------------------------------------------------------------------ kernel arithmetic on the host
def emulate(c, x, e, z):
    """cfg_lcm_step_kernel (csrc/small.hip) on one table row, fp32, in its operation order."""
    x0 = (x - c[0] * e) / c[1]
    den = c[2] * x0 + c[3] * x
    return c[4] * den + c[5] * z if c[5] != 0 else den


@pytest.mark.parametrize("scaling", [10.0, 0.001])
@pytest.mark.parametrize("N", [4, 8])
def test_whole_schedule_on_the_product_table_reproduces_the_restatement(N, scaling):
    """At the default timestep_scaling c_skip ~ 1e-8 and c_out rounds to 1: a kernel without the boundary terms would pass
    there.  At 0.001 (s = 0.999 .. 0.139: c_skip 0.2 .. 0.93, c_out 0.89 .. 0.27) it cannot."""
    g = torch.Generator().manual_seed(0)
    x0 = torch.randn(2, 4, 8, 8, generator=g)
    eps = [torch.randn(2, 4, 8, 8, generator=g) for _ in range(N)]
    zs = [torch.randn(2, 4, 8, 8, generator=g) for _ in range(N)]
    p, r = PS.LCMScheduler(timestep_scaling=scaling), LC.LCMScheduler(timestep_scaling=scaling)
    p.set_timesteps(N)
    r.set_timesteps(N)
    assert torch.equal(p.timesteps, r.timesteps)
    x, ref = x0.clone(), x0.clone()
    plain = x0.clone()
    for i, t in enumerate(r.timesteps):
        c = p._coef[i]
        z = zs[i] if i < N - 1 else torch.full_like(x0, float("nan"))      # the last row must not read it
        x = emulate(c, x, eps[i], z)
        ref = r.step(eps[i], t, ref, noise=zs[i])[0]
        pc = c.clone()
        pc[2], pc[3] = 1.0, 0.0                                            # a step without the boundary terms
        plain = emulate(pc, plain, eps[i], z)
    assert torch.isfinite(x).all()
    assert torch.allclose(x, ref, rtol=1e-5, atol=1e-5), (N, scaling, float((x - ref).abs().max()))
    if scaling == 0.001:
        assert not torch.allclose(plain, ref, rtol=1e-5, atol=1e-5)
    # ... and the float64 form of the step agrees with the fp32 restatement on one step
    ts = r.timesteps.tolist()
    f64 = LC.step_f64(x0.double().numpy(), eps[0].double().numpy(), zs[0].double().numpy(), ts[0], ts[1], False, scaling)
    one = r.step(eps[0], r.timesteps[0], x0, noise=zs[0])[0]
    assert np.allclose(one.double().numpy(), f64, rtol=1e-5, atol=1e-5)


def test_restatement_draws_once_per_step_but_the_last():
    r = LC.LCMScheduler(generator=torch.Generator().manual_seed(3))
    r.set_timesteps(4)
    x = torch.zeros(1, 4, 2, 2)
    for t in r.timesteps:
        x = r.step(torch.ones_like(x), t, x)[0]
    assert r.draws == 3
    twin = torch.Generator().manual_seed(3)
    for _ in range(3):
        torch.randn(1, 4, 2, 2, generator=twin)
    assert torch.equal(torch.randn(3, generator=twin), torch.randn(3, generator=r.generator))


# ------------------------------------------------------------------------------------------------ config and loading
PNDM_JSON = dict(_class_name="PNDMScheduler", _diffusers_version="0.6.0", beta_end=0.012, beta_schedule="scaled_linear",
                 beta_start=0.00085, num_train_timesteps=1000, set_alpha_to_one=False, skip_prk_steps=True, steps_offset=1,
                 trained_betas=None, clip_sample=False)


def test_from_config_of_an_sd15_donor_and_refused_options():
    s = PS.LCMScheduler.from_config(PS.PNDMScheduler.from_config(PNDM_JSON).config)
    assert isinstance(s, PS.LCMScheduler)
    # kept in config, no effect on the arithmetic
    assert s.config.steps_offset == 1 and s.config.set_alpha_to_one is False and s.config.timestep_spacing == "leading"
    assert s.config.original_inference_steps == 50 and s.config.timestep_scaling == 10.0
    s.set_timesteps(4)
    d = PS.LCMScheduler()
    d.set_timesteps(4)
    assert s.timesteps.tolist() == LISTS[4] and torch.equal(s._coef, d._coef)
    s2 = PS.LCMScheduler.from_config(PS.DDIMScheduler().config, timestep_scaling=5.0)
    assert s2.config.timestep_scaling == 5.0
    # a DPM donor's own options never reach this class's constructor
    PS.LCMScheduler.from_config(dict(vars(PS.DPMSolverMultistepScheduler().config), use_karras_sigmas=True))
    for bad in (dict(prediction_type="v_prediction"), dict(clip_sample=True), dict(thresholding=True),
                dict(rescale_betas_zero_snr=True), dict(beta_schedule="linear"), dict(trained_betas=[0.1, 0.2])):
        with pytest.raises(L.PPError):
            PS.LCMScheduler(**bad)
        with pytest.raises(L.PPError):
            PS.LCMScheduler.from_config(dict(PNDM_JSON, **bad))
    # the other classes' checks did not move
    assert PS.DDIMScheduler.from_config(PNDM_JSON).config.steps_offset == 1
    with pytest.raises(L.PPError):
        PS.DDIMScheduler(clip_sample=True)


def test_load_scheduler_reads_an_lcm_json(tmp_path):
    from powerpaint_amd import loaders
    cfg = dict(_class_name="LCMScheduler", _diffusers_version="0.27.0", beta_start=0.00085, beta_end=0.012,
               beta_schedule="scaled_linear", clip_sample=False, clip_sample_range=1.0, dynamic_thresholding_ratio=0.995,
               num_train_timesteps=1000, original_inference_steps=50, prediction_type="epsilon", rescale_betas_zero_snr=False,
               sample_max_value=1.0, set_alpha_to_one=True, steps_offset=1, thresholding=False, timestep_scaling=10.0,
               timestep_spacing="leading", trained_betas=None)
    (tmp_path / "scheduler_config.json").write_text(json.dumps(cfg))
    s = loaders.load_scheduler(str(tmp_path))
    assert isinstance(s, PS.LCMScheduler) and s.config.steps_offset == 1 and "LCMScheduler" in PS.SCHEDULERS
    (tmp_path / "scheduler_config.json").write_text(json.dumps(dict(cfg, clip_sample=True)))
    with pytest.raises(L.PPError):
        loaders.load_scheduler(str(tmp_path))
    import inspect
    assert "timesteps" in inspect.signature(s.set_timesteps).parameters       # retrieve_timesteps hands a custom list over
    assert "generator" in inspect.signature(s.step).parameters and "eta" not in inspect.signature(s.step).parameters
    with pytest.raises(Exception):
        s.set_timesteps(2)
        s.step(torch.zeros(1, 4, 2, 2), 999, torch.zeros(1, 4, 2, 2))         # CPU tensors: no fallback


def test_retrieve_timesteps_hands_a_custom_list_to_lcm_and_refuses_it_for_ddim():
    from powerpaint_amd.pipelines.pipeline_PowerPaint_Brushnet_CA import retrieve_timesteps
    ts, n = retrieve_timesteps(PS.LCMScheduler(), timesteps=[999, 499, 259])
    assert ts.tolist() == [999, 499, 259] and n == 3
    ts, n = retrieve_timesteps(PS.LCMScheduler(), 4)
    assert ts.tolist() == LISTS[4] and n == 4
    with pytest.raises(ValueError):
        retrieve_timesteps(PS.DDIMScheduler(), timesteps=[999, 499])


# ------------------------------------------------------------------------------------------------ ABI
def test_lcm_entry_rejects_bad_arguments_without_a_gpu():
    lib = L.lib()
    assert L.ABI_VERSION >= 25
    assert lib.pp_cfg_lcm_step(None, 0, 0.0, None, None, 16, None, None, None, None) == -1
    assert lib.pp_cfg_lcm_step(0x1000, 0, 0.0, 0x2000, 0x3000, 0, 0x4000, 0x5000, None, None) == -1       # n <= 0
    assert lib.pp_cfg_lcm_step(0x1000, 0, 0.0, 0x2000, None, 16, 0x4000, 0x5000, None, None) == -1         # no noise buffer
    # pp_cfg_sched_step keeps its kinds: 4 is not one of them
    assert lib.pp_cfg_sched_step(0x1000, 0, 0.0, 0x2000, 0x3000, 16, 4, 0x4000, 0x5000, None, None) == -1


# ------------------------------------------------------------------------------------------------ guidance-embedded UNet
TINY = dict(block_out_channels=(320, 640), layers_per_block=1, down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
            up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"), device="cpu")


def test_time_cond_proj_dim_is_a_unet_option_only():
    from powerpaint_amd import models as PM
    u = PM.UNet2DConditionModel(in_channels=4, time_cond_proj_dim=256, **TINY)
    assert u.config.time_cond_proj_dim == 256
    spec = u.net.synthetic_state_dict(meta=True)
    assert tuple(spec["time_embedding.cond_proj.weight"].shape) == (320, 256)
    assert "time_embedding.cond_proj.bias" not in spec
    plain = PM.UNet2DConditionModel(in_channels=4, **TINY)
    assert plain.config.time_cond_proj_dim is None
    assert "time_embedding.cond_proj.weight" not in plain.net.synthetic_state_dict(meta=True)
    with pytest.raises(L.PPError):
        PM.UNet2DConditionModel(in_channels=4, time_cond_proj_dim=100, **TINY)          # d % 8
    with pytest.raises(L.PPError):
        PM.BrushNetModel(time_cond_proj_dim=256, **TINY)
    with pytest.raises(L.PPError):
        PM.ControlNetModel(time_cond_proj_dim=256, **{k: v for k, v in TINY.items() if k != "up_block_types"})
    with pytest.raises(Exception):
        plain(torch.zeros(1, 4, 8, 8), 1, torch.zeros(1, 77, 768), timestep_cond=torch.zeros(1, 256))


def test_guidance_scale_embedding_equals_the_reference_function():
    """tests/golden/ref_lcm.pt holds what the reference pipeline's own `get_guidance_scale_embedding` returned."""
    from powerpaint_amd import pipelines as PP
    G = torch.load(os.path.join(HERE, "golden", "ref_lcm.pt"), weights_only=False)
    pipe = PP.StableDiffusionPowerPaintBrushNetPipeline()
    for w in (0.0, 0.5, 6.5):
        got = pipe.get_guidance_scale_embedding(torch.tensor([w, w]), embedding_dim=256)
        ref = G["w_embedding"][w]
        assert got.shape == ref.shape == (2, 256) and got.dtype == torch.float32
        assert torch.equal(got, ref), (w, float((got - ref).abs().max()))
    odd = pipe.get_guidance_scale_embedding(torch.tensor([1.5]), embedding_dim=7, dtype=torch.float64)
    assert odd.shape == (1, 7) and odd.dtype == torch.float64 and float(odd[0, -1]) == 0.0


# ------------------------------------------------------------------------------------------------ oracle loops vs the fixture
def test_oracle_loops_with_the_restatement_reproduce_the_reference_calls():
    """The reference's own v1 and BrushNet `__call__` ran with the restated scheduler (tests/golden/make_ref_lcm.py); the
    oracle's loop bodies with the same scheduler give the same latents in fp32 and leave the generator in the same state."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_ref_lcm as M
    G = torch.load(os.path.join(HERE, "golden", "ref_lcm.pt"), weights_only=False)
    for name in ("v1", "v1_strength", "v2"):
        out, nxt = M.oracle_run(name)
        ref = G[name]["latents"]
        assert torch.allclose(out, ref, atol=M.ATOL, rtol=M.RTOL), (name, float((out - ref).abs().max()))
        assert torch.equal(nxt, G[name]["next_draw"]), name
