"""CPU: Heun, DPM2, DPM2 ancestral and LMS on the sigma-space base -- the host side of pp_cfg_ksampler_step.  The product's grids
and table rows against the plain-torch restatement of the library classes (tests/ksampler_cases.py), the LMS coefficients against
the library's quadrature, the oracle's loop bodies with the restatement against the reference's own calls
(tests/golden/ref_ksamplers.pt), refusals, the loader and the entry point's argument checks."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ksampler_cases as KC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import schedulers as PS  # noqa: E402

NAMES = list(KC.CLASSES)
TWO_STAGE = NAMES[:3]
SD15 = dict(timestep_spacing="leading", steps_offset=1)


# ------------------------------------------------------------------------------------------------ grids
@pytest.mark.parametrize("karras", [False, True], ids=["plain", "karras"])
@pytest.mark.parametrize("spacing", ["linspace", "leading", "trailing"])
@pytest.mark.parametrize("name", NAMES)
def test_grids_equal_the_restatement(name, spacing, karras):
    """Both sides run the library's operations in the library's precision (fp32 tensors, fp32 `sigma_to_t` of the midpoints):
    the comparison is exact.  N = 1 is the single Euler row, N = 2 the shortest schedule with a second stage."""
    opts = dict(timestep_spacing=spacing, steps_offset=1 if spacing == "leading" else 0, use_karras_sigmas=karras)
    for n in (1, 2, 7):
        o, h = KC.CLASSES[name](**opts), getattr(PS, name)(**opts)
        assert h.order == o.order and float(h.init_noise_sigma) == pytest.approx(float(o.init_noise_sigma), rel=1e-6)
        o.set_timesteps(n)
        h.set_timesteps(n)
        rows = n if name == "LMSDiscreteScheduler" else 2 * n - 1
        assert len(h.timesteps) == rows and h.timesteps.dtype == torch.float32
        assert torch.equal(h.timesteps, o.timesteps), (n, h.timesteps, o.timesteps)
        want = torch.tensor(KC.eval_sigmas(o))
        assert torch.equal(h._row_sigma, want), (n, h._row_sigma, want)
        assert torch.equal(h._in_div, (want ** 2 + 1) ** 0.5)
        assert float(h.init_noise_sigma) == pytest.approx(float(o.init_noise_sigma), rel=1e-6)
        assert tuple(h._coef.shape) == (rows, 16) and bool(torch.isfinite(h._coef).all())
        if name == "KDPM2DiscreteScheduler" and n > 1 and not karras:
            assert any(t != round(t) for t in h.timesteps.tolist()), "DPM2's midpoint timesteps are fractional"
        x = torch.randn(1, 4, 2, 2, generator=torch.Generator().manual_seed(n))
        for i in (0, rows - 1):
            sc = getattr(PS, name)(**opts)
            sc.set_timesteps(n)
            first = int((sc.timesteps == sc.timesteps[i]).nonzero()[0])       # (no step taken yet: the first occurrence)
            assert torch.equal(sc.scale_model_input(x, sc.timesteps[i]), x / h._in_div[first])


# ------------------------------------------------------------------------------------------------ tables
def _replay(h, o, begin, rows, seed, tol_of=None):
    """Row by row: the product's table in the float64 row formula against the restatement's `step` on float64 tensors."""
    g = torch.Generator().manual_seed(seed)
    shape = (1, 4, 3, 5)
    x = torch.randn(shape, generator=g, dtype=torch.float64) * float(h._row_sigma[begin])
    g_o, g_z = torch.Generator().manual_seed(seed + 1), torch.Generator().manual_seed(seed + 1)
    xo = x.clone()
    xs, saved, H = x.numpy().copy(), np.zeros(shape), [np.zeros(shape) for _ in range(3)]
    worst = 0.0
    for r in range(begin, rows):
        e = torch.randn(shape, generator=g, dtype=torch.float64)
        z = torch.randn(shape, generator=g_z, dtype=torch.float64).numpy() if h.step_noise else None
        assert h.draws_noise_at(r) == bool(h.step_noise)
        hist = [a.copy() for a in H]
        xs, saved, H = KC.row_f64(xs, saved, H, e.numpy(), z, h._coef[r].double().numpy())
        xo = o.step(e, o.timesteps[r], xo, generator=g_o)[0]
        ref = xo.numpy()
        tol = 1e-6 * np.abs(ref) + 1e-12 if tol_of is None else tol_of(h._coef[r].double().numpy(), e.numpy(), hist, ref)
        ratio = float((np.abs(xs - ref) / tol).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (type(h).__name__, begin, r, ratio)
    if h.step_noise:
        assert o.draws == rows - begin                       # one draw per call, both stages
    return worst


@pytest.mark.parametrize("karras", [False, True], ids=["plain", "karras"])
@pytest.mark.parametrize("name", TWO_STAGE)
def test_two_stage_rows_replayed_in_float64_equal_the_restatements_step(name, karras):
    """1e-6 relative: the table's fp32 coefficients are the restatement's own fp32 scalars (same operations in the same order),
    what is left is float64 rounding.  Entered at step 2 of 5 (row 4) the first call carries the second occurrence of its
    timestep and starts a first stage."""
    opts = dict(SD15, use_karras_sigmas=karras)
    for begin in (0, 4):
        o, h = KC.CLASSES[name](**opts), getattr(PS, name)(**opts)
        o.set_timesteps(5)
        h.set_timesteps(5)
        if begin:
            h.set_begin_index(begin)
            assert h.begin_index == begin and torch.equal(h.timesteps, o.timesteps)
        _replay(h, o, begin, 9, seed=3 + begin)
    c = h._coef
    assert bool((c[0::2, 10] == 0).all()) and bool((c[1::2, 10] == 1).all())                 # B rows start from the saved sample
    assert bool((c[0:-1:2, 11] == 1).all()) and c[-1, 11] == 0 and bool((c[1::2, 11] == 0).all())
    assert bool((c[:, 4] != 0).any()) == (name == "KDPM2AncestralDiscreteScheduler") and bool((c[0::2, 4] == 0).all())
    assert bool((c[:, 9] >= 0).any()) == (name == "HeunDiscreteScheduler")


@pytest.mark.parametrize("karras", [False, True], ids=["plain", "karras"])
def test_lms_coefficients_against_the_quadrature(karras):
    """|exact - quad| <= 1e-4 |I| + 1.5e-8: `quad`'s own error contract at epsrel = 1e-4 and the default epsabs."""
    opts = dict(SD15, use_karras_sigmas=karras)
    o, h = KC.LMSDiscreteScheduler(**opts), PS.LMSDiscreteScheduler(**opts)
    o.set_timesteps(7)
    h.set_timesteps(7)
    worst = 0.0
    for i in range(7):
        order = min(i + 1, 4)
        for j in range(order):
            exact, quad = h.lms_coefficient(order, i, j), float(o.get_lms_coefficient(order, i, j))
            tol = 1e-4 * abs(exact) + 1.5e-8
            worst = max(worst, abs(exact - quad) / tol)
            assert abs(exact - quad) <= tol, (i, j, exact, quad)
            assert float(h._coef[i, j]) == pytest.approx(exact, rel=1e-6, abs=1e-12)
        assert bool((h._coef[i, order:4] == 0).all())
    print(f"LMS coefficients, karras {karras}: worst |exact - quad| / tolerance {worst:.3g}")


@pytest.mark.parametrize("begin", [0, 3])
def test_lms_rows_replayed_follow_the_librarys_history(begin):
    """The ring slots and, entered at step 3 of 7, the library's `zip` truncation (order 4 basis, one derivative in the list).
    Per row the tolerance is the coefficient contract carried through the sum: sum_j (1e-4 |C_j| + 1.5e-8) |d_j|."""
    o, h = KC.LMSDiscreteScheduler(**SD15), PS.LMSDiscreteScheduler(**SD15)
    o.set_timesteps(7)
    h.set_timesteps(7)
    if begin:
        h.set_begin_index(begin)
        assert bool((h._coef[begin, 1:4] == 0).all()) and h._coef[begin, 0] != 0
        assert float(h._coef[begin, 0]) == pytest.approx(h.lms_coefficient(4, begin, 0), rel=1e-6)
        assert bool((h._coef[begin + 1, 2:4] == 0).all()) and h._coef[begin + 1, 1] != 0

    def tol(row, e, hist, ref):
        c = np.abs(row[:4])
        d = [np.abs(e)] + [np.abs(hist[int(row[6 + k])]) for k in range(3)]
        return sum((1e-4 * c[k] + 1.5e-8) * d[k] for k in range(4)) + 1e-6 * np.abs(ref) + 1e-12

    _replay(h, o, begin, 7, seed=11, tol_of=tol)
    pushes = h._coef[begin:, 9].long().tolist()
    assert pushes == [(k % 3) for k in range(7 - begin)]
    for k, r in enumerate(range(begin, 7)):                  # a row pushes into the slot of the oldest entry it read
        assert int(h._coef[r, 8]) == int(h._coef[r, 9]) == k % 3


# ------------------------------------------------------------------------------------------------ oracle loops vs the fixture
def test_oracle_loops_with_the_restatement_reproduce_the_reference_calls():
    """The reference's own v1 and BrushNet `__call__` ran with the restated schedulers (tests/golden/make_ref_ksamplers.py); the
    oracle's loop bodies with the same schedulers give the same latents in fp32 and leave the generator in the same state.
    Gate: tests/test_sigma.py's, 2e-4 / 1e-4.  lms_karras once more with the product's exact coefficients in place of the
    quadrature: measured 2.9e-6 max-abs on latents up to 21.7 (0.007 of the gate), so the same gate holds there."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_ref_ksamplers as M
    G = torch.load(os.path.join(HERE, "golden", "ref_ksamplers.pt"), weights_only=False)
    assert sorted(G) == sorted(M.CASES) == sorted(["heun", "heun_karras_strength", "dpm2", "dpm2_a", "lms_karras"])
    assert (M.ATOL, M.RTOL) == (2e-4, 1e-4)
    for name in M.CASES:
        out, nxt = M.oracle_run(name)
        ref = G[name]["latents"]
        assert torch.allclose(out, ref, atol=M.ATOL, rtol=M.RTOL), (name, float((out - ref).abs().max()))
        assert torch.equal(nxt, G[name]["next_draw"]), name
    out, nxt = M.oracle_run("lms_karras", exact=True)
    ref = G["lms_karras"]["latents"]
    print(f"lms_karras, exact coefficients vs quadrature: final latents max-abs {float((out - ref).abs().max()):.3g}")
    assert torch.allclose(out, ref, atol=M.ATOL, rtol=M.RTOL), float((out - ref).abs().max())
    assert torch.equal(nxt, G["lms_karras"]["next_draw"])


# ------------------------------------------------------------------------------------------------ config and loading
PNDM_JSON = dict(_class_name="PNDMScheduler", _diffusers_version="0.6.0", beta_end=0.012, beta_schedule="scaled_linear",
                 beta_start=0.00085, num_train_timesteps=1000, set_alpha_to_one=False, skip_prk_steps=True, steps_offset=1,
                 trained_betas=None, clip_sample=False)


@pytest.mark.parametrize("name", NAMES)
def test_from_config_of_an_sd15_donor_and_refused_options(name):
    cls = getattr(PS, name)
    s = cls.from_config(PS.PNDMScheduler.from_config(PNDM_JSON).config)
    assert isinstance(s, cls) and s.config.timestep_spacing == "leading" and s.config.steps_offset == 1
    assert s.config.use_karras_sigmas is False and s.config.prediction_type == "epsilon"
    assert cls().config.timestep_spacing == "linspace"
    assert cls.from_config(PNDM_JSON, use_karras_sigmas=True).config.use_karras_sigmas is True
    for bad in (dict(prediction_type="v_prediction"), dict(beta_schedule="linear"), dict(final_sigmas_type="sigma_min"),
                dict(timestep_spacing="quadratic")):
        with pytest.raises(L.PPError):
            cls(**bad)
        with pytest.raises(L.PPError):
            cls.from_config(dict(PNDM_JSON, **bad))
        with pytest.raises(L.PPError):
            cls.from_config(PNDM_JSON, **bad)
    import inspect
    names = inspect.signature(s.step).parameters
    assert "generator" in names and "eta" not in names                        # prepare_extra_step_kwargs
    s.set_timesteps(2)
    with pytest.raises(L.PPError):
        s.step(torch.zeros(1, 4, 2, 2), s.timesteps[0], torch.zeros(1, 4, 2, 2))             # CPU tensors: no fallback
    assert s.kind == 7 + NAMES.index(name) and s.state_slots == 4
    assert s.discards_draw is False and bool(s.step_noise) == (name == "KDPM2AncestralDiscreteScheduler")


def test_lms_step_order_other_than_4_is_refused():
    s = PS.LMSDiscreteScheduler()
    s.set_timesteps(3)
    with pytest.raises(L.PPError):
        s.step(torch.zeros(1, 4, 2, 2), s.timesteps[0], torch.zeros(1, 4, 2, 2), order=2)


@pytest.mark.parametrize("name", NAMES)
def test_load_scheduler_reads_a_json_of_each_name(name, tmp_path):
    from powerpaint_amd import loaders
    cfg = dict(_class_name=name, _diffusers_version="0.27.0", beta_start=0.00085, beta_end=0.012,
               beta_schedule="scaled_linear", num_train_timesteps=1000, prediction_type="epsilon", steps_offset=1,
               timestep_spacing="leading", trained_betas=None, use_karras_sigmas=True)
    (tmp_path / "scheduler_config.json").write_text(json.dumps(cfg))
    s = loaders.load_scheduler(str(tmp_path))
    assert type(s) is getattr(PS, name) and s.config.steps_offset == 1 and s.config.use_karras_sigmas is True
    (tmp_path / "scheduler_config.json").write_text(json.dumps(dict(cfg, prediction_type="v_prediction")))
    with pytest.raises(L.PPError):
        loaders.load_scheduler(str(tmp_path))
    (tmp_path / "scheduler_config.json").write_text(json.dumps(dict(cfg, _class_name="DEISMultistepScheduler")))
    with pytest.raises(L.PPError):
        loaders.load_scheduler(str(tmp_path))
    assert name in PS.SCHEDULERS and "EulerDiscreteScheduler" not in PS.SCHEDULERS


# ------------------------------------------------------------------------------------------------ ABI
def test_ksampler_entry_rejects_bad_arguments_without_a_gpu():
    lib = L.lib()
    assert L.ABI_VERSION >= 27 and lib.pp_abi_version() == L.ABI_VERSION
    f = lib.pp_cfg_ksampler_step
    assert f(None, 0, 0.0, None, None, None, 16, None, None, None, None) == -1
    assert f(0x1000, 0, 0.0, 0x2000, 0x3000, 0x4000, 0, 0x5000, 0x6000, None, None) == -1        # n <= 0
    assert f(0x1000, 0, 0.0, 0x2000, 0x3000, 0x4000, -4, 0x5000, 0x6000, None, None) == -1
    assert f(0x1000, 0, 0.0, 0x2000, 0x3000, None, 16, 0x5000, 0x6000, None, None) == -1         # no noise pointer
    assert f(0x1000, 0, 0.0, 0x2000, None, 0x4000, 16, 0x5000, 0x6000, None, None) == -1         # no state
    assert f(0x1000, 0, 0.0, 0x2000, 0x3000, 0x4000, 16, None, 0x6000, None, None) == -1         # no table
    assert f(0x1000, 0, 0.0, 0x2000, 0x3000, 0x4000, 16, 0x5000, None, None, None) == -1         # no counter
    # pp_cfg_sched_step keeps its kinds: the new classes do not route through it
    for kind in (7, 8, 9, 10):
        assert lib.pp_cfg_sched_step(0x1000, 0, 0.0, 0x2000, 0x3000, 16, kind, 0x4000, 0x5000, None, None) == -1
