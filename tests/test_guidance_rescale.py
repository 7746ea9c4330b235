"""CPU: `guidance_rescale` off the device -- the step program `DenoiseLoop.bind` assembles with and without it, the argument
checks of pp_cfg_rescale and of the pipelines, the float64 restatement (tests/guidance_cases.py) against a direct transcription
of the library's three lines, and the arithmetic behind the GPU test's accuracy gate: an fp32 two-pass meets 64 * 2^-24 where
the mean is large against the spread, an fp32 one-pass sum of squares does not."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import guidance_cases as GC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import guidance as GDM  # noqa: E402
from powerpaint_amd import pipelines as PP  # noqa: E402
from powerpaint_amd import schedulers as PS  # noqa: E402
from powerpaint_amd.engine import Plan  # noqa: E402
from powerpaint_amd.pipelines._loop import DenoiseLoop  # noqa: E402

U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ program identity
def _host_tables(cls):
    """A scheduler of this package whose "device" tables live on the host: `bind` only takes their addresses."""
    class Host(cls):
        def _upload(self, device):
            super()._upload(device)
            self._coef_dev = self._coef.clone()
            self._ts_dev = self.timesteps.to(torch.float32).clone()
            self._step_dev = torch.zeros(1, dtype=torch.int32)
    return Host


class _Loop(DenoiseLoop):
    """DenoiseLoop with the networks replaced by one named launch: everything else of `bind` (the key, the tail) is the real
    code, and nothing of it touches a device."""

    def _prepare_runtimes(self, *a, **kw):
        if getattr(self, "_stub", None) is None:
            plan = Plan()
            plan.add("unet", None)
            self._stub = SimpleNamespace(step_plan=plan, outputs={"eps": 0x10000}, tome_blocks=lambda: [], ip_scales=lambda: (),
                                         net=SimpleNamespace(params=None))
        return self._stub, None, []

    def _head_launches(self, side_rts, rt, *a, **kw):
        return {id(rt): [(None, (), "step_head")]}, {id(rt): set()}


def _loop(cls=PS.DDIMScheduler, **kw):
    sch = _host_tables(cls)(**kw)
    sch.set_timesteps(3)
    unet = SimpleNamespace(net=SimpleNamespace(tome=None), device="cpu")
    return _Loop(unet, sch)


def _names(loop):
    return [c[2] for c in loop.program.calls]


@pytest.mark.parametrize("cls,step_name", [(PS.DDIMScheduler, "cfg_sched_step"), (PS.EulerAncestralDiscreteScheduler, "cfg_sigma_step"),
                                           (PS.HeunDiscreteScheduler, "cfg_ksampler_step"), (PS.LCMScheduler, "cfg_lcm_step")])
def test_program_with_and_without_the_rescale(cls, step_name):
    shape = (2, 4, 6, 10)
    loop = _loop(cls)
    loop.bind(shape, True, 7.5, None)
    parent = _names(loop)
    assert parent == ["step_head", "unet", step_name] and "cfg_rescale" not in parent
    parent_step = loop.program.calls[-1]
    assert parent_step[1][1] == 1                                   # the step launch does the CFG combine itself
    # guidance_rescale = 0.0: the same key, the same program object
    program0 = loop.program
    loop.bind(shape, True, 7.5, None, guidance_rescale=0.0)
    assert loop.program is program0 and _names(loop) == parent
    # 0.7 with CFG: one cfg_rescale in front of the step launch, which runs with cfg = 0
    loop.bind(shape, True, 7.5, None, guidance_rescale=0.7)
    names = _names(loop)
    assert names == ["step_head", "unet", "cfg_rescale", step_name]
    assert names.count("cfg_rescale") == 1 and "pag_combine" not in names
    fn, args, _ = loop.program.calls[2]
    assert fn is L.lib().pp_cfg_rescale
    assert args == (0x10000, 2, 7.5, None, loop._phi_cell.data_ptr(), loop._keep[1].data_ptr(), 2, 4 * 6 * 10)
    step = loop.program.calls[3]
    assert step[1][1] == 0 and step[1][0] == parent_step[1][0] and step[1][2:] == parent_step[1][2:]
    # another phi: data, not part of the key
    program7 = loop.program
    loop.bind(shape, True, 7.5, None, guidance_rescale=0.3)
    assert loop.program is program7 and loop._rescale == 0.3
    # back to 0: the parent's program, launch for launch
    loop.bind(shape, True, 7.5, None, guidance_rescale=0.0)
    assert _names(loop) == parent and loop.program.calls[-1] == parent_step and loop._rescale is None


def test_without_cfg_the_argument_has_no_effect():
    loop = _loop()
    loop.bind((1, 4, 8, 8), False, 1.0, None)
    parent, program0 = _names(loop), loop.program
    assert loop.program.calls[-1][1][1] == 0
    loop.bind((1, 4, 8, 8), False, 1.0, None, guidance_rescale=0.7)
    assert loop.program is program0 and _names(loop) == parent and loop._rescale is None
    # PAG without CFG, too: the two-way pag_combine stays, no rescale
    loop.bind((1, 4, 8, 8), False, 1.0, None, pag_scale=3.0, guidance_rescale=0.7)
    assert _names(loop) == ["step_head", "unet", "pag_combine", "cfg_sched_step"]


def test_with_pag_the_rescale_launch_replaces_pag_combine():
    loop = _loop()
    loop.bind((1, 4, 8, 8), True, 7.5, None, pag_scale=3.0)
    assert _names(loop) == ["step_head", "unet", "pag_combine", "cfg_sched_step"]
    loop.bind((1, 4, 8, 8), True, 7.5, None, pag_scale=3.0, guidance_rescale=0.7)
    assert _names(loop) == ["step_head", "unet", "cfg_rescale", "cfg_sched_step"]
    args = loop.program.calls[2][1]
    assert args[1] == 3 and args[3] == loop._pag_table.data_ptr() and args[5] == loop._keep[1].data_ptr()
    assert loop.program.calls[3][1][1] == 0


def test_the_blend_tail():
    """ppt-v1 with a 4-channel UNet: [cfg_rescale, cfg_sched_step, latent_blend, step_advance]."""
    loop = _loop()
    sh = (1, 4, 8, 8)
    blend = (torch.zeros(sh), torch.zeros(1, 1, 8, 8), torch.zeros(sh))
    loop.bind(sh, True, 7.5, None, blend=blend, guidance_rescale=0.7)
    assert _names(loop)[-4:] == ["cfg_rescale", "cfg_sched_step", "latent_blend", "step_advance"]


# ------------------------------------------------------------------------------------------------ rejections
def test_bad_args_are_rejected_without_a_gpu():
    lib = L.lib()
    # (eps, segs, guidance, pag_table, phi_dev, step_dev, batch, per)
    ok2 = (0x1000, 2, 7.5, None, 0x2000, None, 2, 16)
    ok3 = (0x1000, 3, 7.5, 0x3000, 0x2000, 0x4000, 2, 16)
    bad = [(ok2, 0, None), (ok2, 4, None), (ok3, 0, None), (ok3, 4, None),        # null eps / phi_dev
           (ok2, 1, 1), (ok2, 1, 4), (ok2, 1, 0), (ok2, 1, -2),                   # segs outside {2, 3}
           (ok3, 3, None), (ok2, 3, 0x3000),                                     # 3 without a table, 2 with one
           (ok3, 5, None),                                                      # a table without the step counter
           (ok2, 6, 0), (ok2, 6, -1), (ok3, 6, 0),                               # batch <= 0
           (ok2, 7, 1), (ok2, 7, 0), (ok2, 7, -8), (ok3, 7, 1),                   # per < 2
           (ok2, 0, 0x1001), (ok2, 0, 0x1002), (ok3, 0, 0x1003)]                 # eps not 4-byte aligned
    for base, i, v in bad:
        a = list(base)
        a[i] = v
        assert lib.pp_cfg_rescale(*a, None) == -1, (i, v)


@pytest.mark.parametrize("bad", [-0.1, float("nan"), float("inf"), -float("inf"), "x", None])
def test_check_inputs_raises_on_a_negative_or_non_finite_value(bad):
    pe = torch.zeros(1, 77, 768)
    v1 = PP.StableDiffusionInpaintPipeline(scheduler=PS.DDIMScheduler())
    cn = PP.StableDiffusionControlNetInpaintPipeline(scheduler=PS.DDIMScheduler())
    v2 = PP.StableDiffusionPowerPaintBrushNetPipeline(scheduler=PS.DDIMScheduler())
    for pipe in (v1, cn):
        pipe.check_inputs(None, 64, 64, 1.0, 1, None, pe, None, guidance_rescale=0.7)
        with pytest.raises(ValueError, match="guidance_rescale"):
            pipe.check_inputs(None, 64, 64, 1.0, 1, None, pe, None, guidance_rescale=bad)
    v2.check_inputs(guidance_rescale=0.7)
    with pytest.raises(ValueError, match="guidance_rescale"):
        v2.check_inputs(guidance_rescale=bad)
    with pytest.raises(ValueError, match="guidance_rescale"):
        GDM.check_guidance_rescale(bad)
    # ... and in `__call__`, before anything runs (no network is attached to these pipelines)
    for pipe in (v1, cn, v2):
        with pytest.raises(ValueError, match="guidance_rescale"):
            pipe(prompt_embeds=pe, height=64, width=64, guidance_rescale=bad)
    # the loop checks what it is handed, too -- where CFG is on
    with pytest.raises(ValueError, match="guidance_rescale"):
        _loop().bind((1, 4, 8, 8), True, 7.5, None, guidance_rescale=bad)


def test_zero_and_positive_values_pass():
    assert GDM.check_guidance_rescale(0) == 0.0 and GDM.check_guidance_rescale(0.7) == 0.7 and GDM.check_guidance_rescale(1) == 1.0
    import inspect
    for cls in (PP.StableDiffusionInpaintPipeline, PP.StableDiffusionControlNetInpaintPipeline,
                PP.StableDiffusionPowerPaintBrushNetPipeline):
        params = [p for p in inspect.signature(cls.__call__).parameters.values() if p.kind is not p.VAR_KEYWORD]
        assert params[-1].name == "guidance_rescale" and params[-1].default == 0.0 and params[-2].name == "pag_adaptive_scale"


# ------------------------------------------------------------------------------------------------ the restatement
def _library_lines(noise_cfg, noise_pred_text, guidance_rescale):
    """diffusers 0.27 `rescale_noise_cfg`, transcribed line by line, on float64 tensors."""
    std_text = noise_pred_text.std(dim=list(range(1, noise_pred_text.ndim)), keepdim=True)
    std_cfg = noise_cfg.std(dim=list(range(1, noise_cfg.ndim)), keepdim=True)
    noise_pred_rescaled = noise_cfg * (std_text / std_cfg)
    noise_cfg = guidance_rescale * noise_pred_rescaled + (1 - guidance_rescale) * noise_cfg
    return noise_cfg


@pytest.mark.parametrize("segs", [2, 3])
def test_restatement_agrees_with_the_library_lines(segs):
    gq = torch.Generator().manual_seed(3 + segs)
    B, shape = 3, (4, 6, 10)
    e = torch.randn(segs, B, *shape, generator=gq, dtype=torch.float64) * 2 + 0.5
    g, s, phi = 7.5, 2.5, 0.7
    cfg = e[0] + g * (e[1] - e[0]) + (s * (e[1] - e[2]) if segs == 3 else 0.0)
    want = _library_lines(cfg, e[1], phi).reshape(B, -1).numpy()
    got = GC.rescale_f64(e.reshape(segs, B, -1).numpy(), segs, g, s, phi)
    assert np.allclose(got, want, rtol=1e-13, atol=0)              # the ratio of SSDs is the ratio of torch.std's
    # the tensor forms: the oracle loops' and the package's own (the duck-typed scheduler path)
    assert np.allclose(GC.rescale_tensor(cfg, e[1], phi).reshape(B, -1).numpy(), want, rtol=1e-13, atol=0)
    assert np.allclose(GDM.rescale_noise_cfg(cfg, e[1], phi).reshape(B, -1).numpy(), want, rtol=1e-13, atol=0)
    # per sample: sample 1 alone gives sample 1's row
    alone = GC.rescale_f64(e[:, 1:2].reshape(segs, 1, -1).numpy(), segs, g, s, phi)
    assert np.array_equal(alone[0], got[1])
    # phi = 1: the result has the conditional prediction's deviation
    full = GC.rescale_f64(e.reshape(segs, B, -1).numpy(), segs, g, s, 1.0)
    assert np.allclose(full.std(axis=1, ddof=1), e[1].reshape(B, -1).numpy().std(axis=1, ddof=1), rtol=1e-12)


# ------------------------------------------------------------------------------------------------ the accuracy gate's arithmetic
def _pairwise32(x):
    x = np.asarray(x, dtype=np.float32)
    while x.size > 1:
        if x.size % 2:
            x = np.concatenate([x, np.zeros(1, np.float32)])
        x = (x[0::2] + x[1::2]).astype(np.float32)
    return np.float32(x[0])


def _sequential32(x):
    acc = np.float32(0.0)
    for v in np.asarray(x, dtype=np.float32):
        acc = np.float32(acc + v)
    return acc


def _two_pass32(x, total):
    x = np.asarray(x, dtype=np.float32)
    mean = np.float32(total(x) / np.float32(x.size))
    d = (x - mean).astype(np.float32)
    return total((d * d).astype(np.float32))


def _one_pass32(x, total):
    x = np.asarray(x, dtype=np.float32)
    s1 = total(x)
    s2 = total((x * x).astype(np.float32))
    return np.float32(s2 - np.float32(np.float32(s1 * s1) / np.float32(x.size)))


@pytest.mark.parametrize("per", [140, 16384])
def test_two_pass_fp32_meets_the_gate_and_one_pass_does_not(per):
    """The regime: values 8 + randn / 16 (the mean 128 standard deviations away from 0), g = 7.5.  In units of u = 2^-24:
    the fp32 two-pass ratio is within 64 u of the float64 one whatever the summation order (printed below per order; a
    16384-term running sum leaves its error in the mean, which enters the SSD only squared); the one-pass sum-of-squares
    form loses the deviation to cancellation and misses the gate by a wide margin."""
    gq = np.random.default_rng(per)
    g32 = np.float32(7.5)
    worst_two, best_one = {"_pairwise32": 0.0, "_sequential32": 0.0}, np.inf
    for trial in range(4):
        e = (8.0 + gq.standard_normal((2, 1, per)) / 16.0).astype(np.float32)
        m32 = (e[0, 0] + g32 * (e[1, 0] - e[0, 0]).astype(np.float32)).astype(np.float32)
        r64 = float(GC.ratio_f64(e, 2, 7.5, 0.0)[0, 0])
        for total in (_pairwise32, _sequential32):
            r32 = np.sqrt(np.float32(_two_pass32(e[1, 0], total) / _two_pass32(m32, total)), dtype=np.float32)
            worst_two[total.__name__] = max(worst_two[total.__name__], abs(float(r32) - r64) / r64 / U)
            with np.errstate(invalid="ignore", divide="ignore"):
                o32 = np.sqrt(np.float32(_one_pass32(e[1, 0], total) / _one_pass32(m32, total)), dtype=np.float32)
            err = abs(float(o32) - r64) / r64 / U
            best_one = min(best_one, err if np.isfinite(err) else np.inf)
    print(f"[guidance_rescale] per={per}: two-pass fp32 worst {worst_two['_pairwise32']:.1f} u pairwise, "
          f"{worst_two['_sequential32']:.1f} u sequential; one-pass fp32 best {best_one:.0f} u (gate 64 u)")
    assert max(worst_two.values()) <= 64.0
    assert best_one > 64.0
