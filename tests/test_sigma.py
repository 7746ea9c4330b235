"""CPU: the sigma-space schedulers (EulerDiscreteScheduler kind 5, EulerAncestralDiscreteScheduler kind 6) and
`use_karras_sigmas` (both, and DPM-Solver++ 2M) -- grids, coefficient rows, the step kernel's arithmetic emulated on the host,
config handling and loading, the ABI entries, and the oracle loops against the reference's own calls."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sigma_cases as SC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import schedulers as PS  # noqa: E402

U = 2.0 ** -24                       # unit roundoff of fp32
CLASSES = [("EulerDiscreteScheduler", False), ("EulerAncestralDiscreteScheduler", True)]
SPACINGS = [dict(timestep_spacing="linspace"), dict(timestep_spacing="leading", steps_offset=1),
            dict(timestep_spacing="trailing")]


# ------------------------------------------------------------------------------------------------ grids
@pytest.mark.parametrize("karras", [False, True], ids=["plain", "karras"])
@pytest.mark.parametrize("opts", SPACINGS, ids=["linspace", "leading", "trailing"])
@pytest.mark.parametrize("name,anc", CLASSES)
def test_timesteps_sigmas_and_init_noise_sigma(name, anc, opts, karras):
    """Both sides evaluate the same numpy expressions on the same fp32 training table: equal to the bit."""
    for N in (1, 6, 25):
        p = getattr(PS, name)(use_karras_sigmas=karras, **opts)
        r = getattr(SC, name)(use_karras_sigmas=karras, **opts)
        # before set_timesteps: the training table's largest sigma
        assert float(p.init_noise_sigma) == pytest.approx(float(r.init_noise_sigma), rel=1e-6)
        p.set_timesteps(N)
        r.set_timesteps(N)
        assert p.timesteps.dtype == torch.float32 and torch.equal(p.timesteps, r.timesteps), (N, p.timesteps, r.timesteps)
        assert p.sigmas.dtype == torch.float32 and torch.equal(p.sigmas, r.sigmas) and float(p.sigmas[-1]) == 0.0
        assert float(p.init_noise_sigma) == pytest.approx(float(r.init_noise_sigma), rel=1e-6)
        assert N == 1 or float(p.init_noise_sigma) > 1.0          # (one `linspace` / `leading` step sits at t = 0 / 1)
        want = float(p.sigmas.max())
        if opts["timestep_spacing"] == "leading":
            want = (want ** 2 + 1) ** 0.5
        assert float(p.init_noise_sigma) == pytest.approx(want, rel=1e-6)
        assert p.num_inference_steps == N and p.order == 1 and p.kind == (6 if anc else 5)
        assert all(a > b for a, b in zip(p.timesteps.tolist(), p.timesteps.tolist()[1:]))
        if karras and N == 6:
            frac = [t for t in p.timesteps.tolist() if t != round(t)]
            assert frac, "the Karras timesteps of the Euler classes stay fractional"
        x = torch.randn(2, 4, 3, 3, generator=torch.Generator().manual_seed(N))
        for i, t in enumerate(p.timesteps):
            assert torch.equal(p.scale_model_input(x, t), r.scale_model_input(x, t))
            assert torch.equal(p.scale_model_input(x, t), x / ((p.sigmas[i] ** 2 + 1) ** 0.5))
        tt = p.timesteps[N // 2:N // 2 + 1].repeat(2)
        assert torch.equal(p.add_noise(x, 2 * x, tt), r.add_noise(x, 2 * x, tt))
        assert torch.equal(p.add_noise(x, 2 * x, tt), x + 2 * x * p.sigmas[N // 2])


def test_sd15_leading_grid_values():
    """Six steps of the SD-1.5 checkpoint config: 1000 // 6 = 166 apart, offset 1; sigma(t) = sqrt((1 - abar) / abar)."""
    p = PS.EulerAncestralDiscreteScheduler(timestep_spacing="leading", steps_offset=1)
    p.set_timesteps(6)
    assert p.timesteps.tolist() == [831.0, 665.0, 499.0, 333.0, 167.0, 1.0]
    ac = p.alphas_cumprod.double()
    want = ((1 - ac) / ac).sqrt()[[831, 665, 499, 333, 167, 1]]
    assert torch.allclose(p.sigmas[:-1].double(), want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("N", [6, 25, 100])
def test_dpm_karras_grid(N):
    p, r = PS.DPMSolverMultistepScheduler(use_karras_sigmas=True), SC.DPMKarras()
    p.set_timesteps(N)
    r.set_timesteps(N)
    assert p.timesteps.dtype == torch.int64 and torch.equal(p.timesteps, r.timesteps)
    assert torch.equal(p.sigmas, r.sigmas)
    train = SC.train_sigmas()
    assert float(p.sigmas[0]) == pytest.approx(float(train[-1]), rel=1e-6)       # the ends of the full table,
    assert float(p.sigmas[-2]) == pytest.approx(float(train[0]), rel=1e-6)       # not of an inference grid
    assert p.timesteps[0] == 999 and p.timesteps[-1] == 0
    # the spacing options have no effect
    q = PS.DPMSolverMultistepScheduler(use_karras_sigmas=True, timestep_spacing="leading", steps_offset=1)
    q.set_timesteps(N)
    assert torch.equal(q.timesteps, p.timesteps) and torch.equal(q._coef, p._coef)
    # and without the option nothing moved
    a, b = PS.DPMSolverMultistepScheduler(), PS.DPMSolverMultistepScheduler(use_karras_sigmas=False)
    a.set_timesteps(N)
    b.set_timesteps(N)
    assert torch.equal(a._coef, b._coef) and not torch.equal(a.sigmas, p.sigmas)


def test_repeated_rounded_karras_timesteps_resolve_by_call_order():
    p = PS.DPMSolverMultistepScheduler(use_karras_sigmas=True)
    p.set_timesteps(100)
    ts = p.timesteps.tolist()
    assert len(set(ts)) < len(ts), "100 rounded Karras timesteps were expected to repeat near 0"
    assert [p._index_of(t) for t in ts] == list(range(100))
    p.reset()
    assert [p._index_of(t) for t in ts] == list(range(100))
    p.set_timesteps(100)
    assert p._index_of(ts[-1]) == ts.index(ts[-1])
    # PLMS keeps its rule: the repeated second entry
    q = PS.PNDMScheduler()
    q.set_timesteps(5)
    assert [q._index_of(t) for t in q.timesteps.tolist()] == list(range(6))
    e = PS.EulerDiscreteScheduler(use_karras_sigmas=True)
    e.set_timesteps(6)
    assert [e._index_of(t) for t in e.timesteps] == list(range(6))            # float compare, fractional values
    with pytest.raises(ValueError):
        e._index_of(500.25)


# ------------------------------------------------------------------------------------------------ rows
def row_tolerance(s_from, s_to, s_up, s_down):
    """Absolute fp32 error bounds of (dt, s_up) as `_fill_table` evaluates them from the fp32 grid, from the row's own
    magnitudes (float64 values in, U = 2^-24 per rounded operation, first order, doubled for the second-order terms).
      q = s_to^2 (s_from^2 - s_to^2) / s_from^2:  the two squares carry U each, their difference
          U (s_from^2 + s_to^2) + U |diff| <= 3 U s_from^2, times s_to^2 / s_from^2 -> 3 U s_to^2, plus one U q each for the
          square, the product and the quotient (q <= s_to^2):  |dq| <= 6 U s_to^2
      s_up = sqrt(q):        |d s_up| <= |dq| / (2 s_up) + U s_up
      r = s_to^2 - s_up^2:   |dr| <= U s_to^2 + (2 s_up |d s_up| + U s_up^2) + U r
      s_down = sqrt(r):      |d s_down| <= |dr| / (2 s_down) + U s_down
      dt = s_down - s_from:  |d dt| <= |d s_down| + U |dt|
    With s_up = 0 (plain Euler, the last row) q and d s_up vanish; with s_to = 0 everything but U |dt| does."""
    d_up = (6 * U * s_to ** 2 / (2 * s_up) + U * s_up) if s_up > 0 else 0.0
    r = s_to ** 2 - s_up ** 2
    d_r = U * s_to ** 2 + 2 * s_up * d_up + U * s_up ** 2 + U * r
    d_down = (d_r / (2 * s_down) + U * s_down) if s_down > 0 else 0.0
    return 2 * (d_down + U * abs(s_down - s_from)), 2 * d_up


@pytest.mark.parametrize("karras", [False, True], ids=["plain", "karras"])
@pytest.mark.parametrize("opts", SPACINGS, ids=["linspace", "leading", "trailing"])
@pytest.mark.parametrize("name,anc", CLASSES)
def test_table_rows_against_the_float64_formulas(name, anc, opts, karras):
    p = getattr(PS, name)(use_karras_sigmas=karras, **opts)
    for N in (1, 6, 25):
        p.set_timesteps(N)
        assert tuple(p._coef.shape) == (N, 8) and p._coef.dtype == torch.float32
        sig = p.sigmas.double().numpy()
        for i in range(N):
            want = SC.row_f64(sig, i, anc)
            got = p._coef[i].double().numpy()
            s_down = want[1] + want[0]
            tol_dt, tol_up = row_tolerance(sig[i], sig[i + 1], want[2], s_down)
            assert got[0] == sig[i]                                              # the grid value itself
            assert abs(got[1] - want[1]) <= tol_dt, (N, i, got[1], want[1], tol_dt)
            assert abs(got[2] - want[2]) <= tol_up, (N, i, got[2], want[2], tol_up)
            assert (got[3:] == 0).all()
            assert (got[2] > 0) == (anc and i < N - 1)
        assert float(p._coef[-1, 1]) == -float(p.sigmas[-2]) and float(p._coef[-1, 2]) == 0.0     # sigma_last = 0
        assert torch.equal(p._in_div, (p.sigmas[:-1] ** 2 + 1) ** 0.5) and p._in_div.dtype == torch.float32
    p.set_timesteps(8)
    full = p._coef.clone()
    p.set_begin_index(4)                                    # strength 0.5 through get_timesteps: only the counter moves
    assert torch.equal(p._coef, full) and p.begin_index == 4 and len(p.timesteps) == 8
    assert p.step_noise == anc and [p.draws_noise_at(i) for i in range(8)] == [True] * 8
    assert p.discards_draw == (not anc)


@pytest.mark.parametrize("name,anc", CLASSES)
def test_renoise_table_is_add_noise_of_the_next_timestep(name, anc):
    """(1, sigma_{i+1}) after step i, (1, 0) after the last: what pp_latent_blend multiplies x0 and the noise by."""
    for karras in (False, True):
        p = getattr(PS, name)(timestep_spacing="leading", steps_offset=1, use_karras_sigmas=karras)
        r = getattr(SC, name)(timestep_spacing="leading", steps_offset=1, use_karras_sigmas=karras)
        p.set_timesteps(7)
        r.set_timesteps(7)
        tab = p.renoise_table()
        assert tab.shape == (7, 2) and tab.dtype == torch.float32
        one, zero = torch.ones(1, 1), torch.zeros(1, 1)
        for i in range(6):
            t = r.timesteps[i + 1:i + 2]
            assert float(tab[i, 0]) == float(r.add_noise(one, zero, t)) == 1.0
            assert float(tab[i, 1]) == float(r.add_noise(zero, one, t))
        assert tab[6].tolist() == [1.0, 0.0]


# ------------------------------------------------------------------------------------------------ kernel arithmetic on the host
def emulate(c, x, e, z):
    """cfg_sigma_step_kernel (csrc/small.hip) on one table row, fp32, in its operation order."""
    xn = x + c[1] * e
    return xn + c[2] * z if c[2] != 0 else xn


@pytest.mark.parametrize("karras", [False, True], ids=["plain", "karras"])
@pytest.mark.parametrize("name,anc", CLASSES)
def test_whole_schedule_on_the_product_table_reproduces_the_restatement(name, anc, karras):
    N = 6
    g = torch.Generator().manual_seed(0)
    x0 = torch.randn(2, 4, 8, 8, generator=g)
    eps = [torch.randn(2, 4, 8, 8, generator=g) for _ in range(N)]
    zs = [torch.randn(2, 4, 8, 8, generator=g) for _ in range(N)]
    opts = dict(timestep_spacing="leading", steps_offset=1, use_karras_sigmas=karras)
    p, r = getattr(PS, name)(**opts), getattr(SC, name)(**opts)
    p.set_timesteps(N)
    r.set_timesteps(N)
    x = ref = x0 * float(p.init_noise_sigma)
    for i, t in enumerate(r.timesteps):
        z = zs[i] if (anc and i < N - 1) else torch.full_like(x0, float("nan"))      # rows with s_up = 0 must not read it
        x = emulate(p._coef[i], x, eps[i], z)
        ref = r.step(eps[i], t, ref, noise=zs[i])[0]
    assert torch.isfinite(x).all()
    # the restatement goes through x0 = x - sigma e and (x - x0) / sigma, the kernel uses e: a few ulp of |x| + sigma |e|
    assert torch.allclose(x, ref, rtol=1e-5, atol=1e-5 * float(p.sigmas[0])), float((x - ref).abs().max())
    f64 = SC.step_f64(x0.double().numpy(), eps[0].double().numpy(), None, zs[0].double().numpy(), 0.0,
                      *SC.row_f64(p.sigmas.double().numpy(), 0, anc)[1:])
    one = r.step(eps[0], r.timesteps[0], x0, noise=zs[0])[0]
    assert np.allclose(one.double().numpy(), f64, rtol=1e-5, atol=1e-5 * float(p.sigmas[0]))


def test_restatement_draws_once_per_step_for_both_classes():
    for name, _ in CLASSES:
        r = getattr(SC, name)(generator=torch.Generator().manual_seed(3))
        r.set_timesteps(4)
        x = torch.zeros(1, 4, 2, 2)
        for t in r.timesteps:
            x = r.step(torch.ones_like(x), t, x)[0]
        assert r.draws == 4
        twin = torch.Generator().manual_seed(3)
        for _ in range(4):
            torch.randn(1, 4, 2, 2, generator=twin)
        assert torch.equal(torch.randn(3, generator=twin), torch.randn(3, generator=r.generator))
    # the product's host-side discard advances a generator by exactly one such draw
    a, b = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    PS.EulerDiscreteScheduler.discard_draw((1, 4, 2, 2), a, torch.float32)
    torch.randn(1, 4, 2, 2, generator=b)
    assert torch.equal(torch.randn(3, generator=a), torch.randn(3, generator=b))
    PS.EulerDiscreteScheduler.discard_draw((1, 4, 2, 2), None, torch.float32)            # no generator: nothing to do


# ------------------------------------------------------------------------------------------------ config and loading
PNDM_JSON = dict(_class_name="PNDMScheduler", _diffusers_version="0.6.0", beta_end=0.012, beta_schedule="scaled_linear",
                 beta_start=0.00085, num_train_timesteps=1000, set_alpha_to_one=False, skip_prk_steps=True, steps_offset=1,
                 trained_betas=None, clip_sample=False)


@pytest.mark.parametrize("name,anc", CLASSES)
def test_from_config_of_an_sd15_donor_and_refused_options(name, anc):
    cls = getattr(PS, name)
    s = cls.from_config(PS.PNDMScheduler.from_config(PNDM_JSON).config)
    assert isinstance(s, cls) and s.config.timestep_spacing == "leading" and s.config.steps_offset == 1
    assert s.config.use_karras_sigmas is False and s.config.prediction_type == "epsilon"
    s.set_timesteps(6)
    assert s.timesteps.tolist() == [831.0, 665.0, 499.0, 333.0, 167.0, 1.0]
    d = cls()                                                 # the class default is `linspace`
    d.set_timesteps(6)
    assert d.config.timestep_spacing == "linspace" and d.timesteps[0] == 999.0 and d.timesteps[-1] == 0.0
    k = cls.from_config(PNDM_JSON, use_karras_sigmas=True)
    assert k.config.use_karras_sigmas is True and k.config.steps_offset == 1
    assert cls.from_config(dict(vars(PS.DPMSolverMultistepScheduler(use_karras_sigmas=True).config))).config.use_karras_sigmas
    # the donor's own options never reach this class's constructor
    cls.from_config(dict(vars(PS.DPMSolverMultistepScheduler().config), clip_sample=True, thresholding=True))
    for bad in (dict(prediction_type="v_prediction"), dict(beta_schedule="linear"), dict(rescale_betas_zero_snr=True),
                dict(trained_betas=[0.1, 0.2]), dict(interpolation_type="log_linear"), dict(timestep_type="continuous"),
                dict(final_sigmas_type="sigma_min"), dict(timestep_spacing="quadratic"), dict(sigma_min=0.1)):
        with pytest.raises(L.PPError):
            cls(**bad)
        with pytest.raises(L.PPError):
            cls.from_config(dict(PNDM_JSON, **bad))
        with pytest.raises(L.PPError):
            cls.from_config(PNDM_JSON, **bad)


def test_karras_option_is_per_class():
    base = dict(vars(PS.DPMSolverMultistepScheduler().config))
    assert PS.DPMSolverMultistepScheduler.from_config(dict(base, use_karras_sigmas=True)).config.use_karras_sigmas is True
    assert PS.DPMSolverMultistepScheduler.from_config(base).config.use_karras_sigmas is False
    for cls in (PS.DDIMScheduler, PS.PNDMScheduler, PS.UniPCMultistepScheduler):
        with pytest.raises(L.PPError):
            cls(use_karras_sigmas=True)
        with pytest.raises(L.PPError):
            cls.from_config(dict(PNDM_JSON, use_karras_sigmas=True))
    PS.LCMScheduler.from_config(dict(base, use_karras_sigmas=True))                  # LCM goes on ignoring it
    with pytest.raises(L.PPError):
        PS.DPMSolverMultistepScheduler.from_config(dict(base, use_lu_lambdas=True))
    with pytest.raises(L.PPError):
        PS.DPMSolverMultistepScheduler(use_karras_sigmas=True, algorithm_type="sde-dpmsolver++")


def test_load_scheduler_reads_an_euler_ancestral_json_and_not_the_plain_euler_name(tmp_path):
    from powerpaint_amd import loaders
    cfg = dict(_class_name="EulerAncestralDiscreteScheduler", _diffusers_version="0.27.0", beta_start=0.00085,
               beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000, prediction_type="epsilon",
               rescale_betas_zero_snr=False, steps_offset=1, timestep_spacing="leading", trained_betas=None)
    (tmp_path / "scheduler_config.json").write_text(json.dumps(cfg))
    s = loaders.load_scheduler(str(tmp_path))
    assert isinstance(s, PS.EulerAncestralDiscreteScheduler) and s.config.steps_offset == 1
    assert s.config.timestep_spacing == "leading"
    (tmp_path / "scheduler_config.json").write_text(json.dumps(dict(cfg, prediction_type="v_prediction")))
    with pytest.raises(L.PPError):
        loaders.load_scheduler(str(tmp_path))
    # the plain Euler class works as an object; its name is not in the loader map (see load_scheduler)
    assert "EulerDiscreteScheduler" not in PS.SCHEDULERS and "EulerAncestralDiscreteScheduler" in PS.SCHEDULERS
    assert "EulerDiscreteScheduler" in loaders.load_scheduler.__doc__
    import inspect
    for cls in (PS.EulerDiscreteScheduler, PS.EulerAncestralDiscreteScheduler):
        names = inspect.signature(cls().step).parameters
        assert "generator" in names and "eta" not in names                    # prepare_extra_step_kwargs
    e = PS.EulerDiscreteScheduler()
    e.set_timesteps(2)
    with pytest.raises(L.PPError):
        e.step(torch.zeros(1, 4, 2, 2), e.timesteps[0], torch.zeros(1, 4, 2, 2), s_churn=0.5)
    with pytest.raises(L.PPError):
        e.step(torch.zeros(1, 4, 2, 2), e.timesteps[0], torch.zeros(1, 4, 2, 2))         # CPU tensors: no fallback


# ------------------------------------------------------------------------------------------------ ABI
def test_sigma_entries_reject_bad_arguments_without_a_gpu():
    lib = L.lib()
    assert L.ABI_VERSION >= 26 and lib.pp_abi_version() == L.ABI_VERSION
    assert lib.pp_cfg_sigma_step(None, 0, 0.0, None, None, 16, None, None, None, None) == -1
    assert lib.pp_cfg_sigma_step(0x1000, 0, 0.0, 0x2000, 0x3000, 0, 0x4000, 0x5000, None, None) == -1       # n <= 0
    assert lib.pp_cfg_sigma_step(0x1000, 0, 0.0, 0x2000, None, 16, 0x4000, 0x5000, None, None) == -1         # no noise pointer
    ok = (0x1000, 0x2000, 0x3000, 64, 0x4000, 2, 4, 64, 0, 0x5000, 9, 0, 1, 0x6000, 8)
    assert lib.pp_step_head_scaled(*ok, None, None) == -1                                                    # no in_div table
    assert lib.pp_step_head_scaled(*ok[:11], 6, *ok[12:], 0x7000, None) == -1                                # c0 + c > ldc
    assert lib.pp_step_head(*ok[:11], 6, *ok[12:], None) == -1
    # pp_cfg_sched_step keeps its kinds: 5 and 6 are not among them
    for kind in (5, 6):
        assert lib.pp_cfg_sched_step(0x1000, 0, 0.0, 0x2000, 0x3000, 16, kind, 0x4000, 0x5000, None, None) == -1


# ------------------------------------------------------------------------------------------------ oracle loops vs the fixture
def test_oracle_loops_with_the_restatement_reproduce_the_reference_calls():
    """The reference's own v1 and BrushNet `__call__` ran with the restated schedulers (tests/golden/make_ref_sigma.py); the
    oracle's loop bodies with the same schedulers give the same latents in fp32 and leave the generator in the same state.
    Bounds: those of tests/test_lcm.py for the same nets."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_ref_sigma as M
    G = torch.load(os.path.join(HERE, "golden", "ref_sigma.pt"), weights_only=False)
    assert sorted(G) == sorted(M.CASES)
    for name in M.CASES:
        out, nxt = M.oracle_run(name)
        ref = G[name]["latents"]
        assert torch.allclose(out, ref, atol=M.ATOL, rtol=M.RTOL), (name, float((out - ref).abs().max()))
        assert torch.equal(nxt, G[name]["next_draw"]), name
