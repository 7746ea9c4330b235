"""CPU: FreeU -- the four-bin closed form csrc/freeu.hip computes against the torch.fft restatement of diffusers'
`fourier_filter`, the network fixture, the argument checks of pp_freeu and the launch plan with FreeU on and off."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import freeu_cases as FC  # noqa: E402

GOLD_PATH = os.path.join(HERE, "golden", "ref_freeu.pt")


@pytest.mark.parametrize("H,W", FC.CPU_SIZES)
def test_closed_form_is_the_fourier_filter(H, W):
    """atol 5e-6 on unit-variance input: both sides are fp32 and differ by rounding only (7.2e-7 measured over these sizes
    with the pocketfft backend); the x7 margin covers other FFT backends."""
    g = torch.Generator("cpu").manual_seed(H * 100 + W)
    x = torch.randn(2, 5, H, W, generator=g) + 0.5
    for s in (0.9, 0.2, 1.7):
        ref = FC.fourier_filter(x, threshold=1, scale=s)
        got = FC.freeu_closed_form(x, s)
        assert (got - ref).abs().max().item() <= 5e-6, (H, W, s, (got - ref).abs().max().item())
    assert torch.equal(FC.freeu_closed_form(x, 1.0), x)


def test_apply_freeu_restatement_touches_the_first_two_stages_only():
    g = torch.Generator("cpu").manual_seed(3)
    h, r = torch.randn(1, 8, 4, 4, generator=g), torch.randn(1, 6, 4, 4, generator=g)
    for idx, (b, s) in ((0, (1.5, 0.9)), (1, (1.6, 0.2))):
        h2, r2 = FC.apply_freeu(idx, h.clone(), r.clone(), **FC.FREEU_FULL)
        assert torch.equal(h2[:, 4:], h[:, 4:]) and torch.allclose(h2[:, :4], h[:, :4] * b)
        assert torch.allclose(r2, FC.fourier_filter(r, 1, s))
    h2, r2 = FC.apply_freeu(2, h.clone(), r.clone(), **FC.FREEU_FULL)
    assert torch.equal(h2, h) and torch.equal(r2, r)


def test_fixture_discriminates():
    """Every FreeU output of the fixture FAILS the GPU test's gate against the plain output: a UNet that ignored
    enable_freeu could not pass."""
    G = torch.load(GOLD_PATH, weights_only=False)
    assert os.path.getsize(GOLD_PATH) < (1 << 20)
    assert G["settings"]["full"] == FC.FREEU_FULL
    for k, plain in (("eps9_full", "eps9_plain"), ("eps9_skip", "eps9_plain"), ("eps9_backbone", "eps9_plain"),
                     ("eps4_brush_full", "eps4_brush_plain")):
        assert G[k].shape == (2, 4, 64, 64) and G[k].dtype == torch.float32
        cos, err, ok = FC.close_gate(G[plain], G[k])
        assert not ok, (k, cos, err)
        m = G["margins"][k]
        assert abs(m["cos_vs_plain"] - cos) < 1e-6 and (m["cos_vs_plain"] < 0.999 or m["max_err_vs_plain"] > m["gate_err"])


def test_pp_freeu_rejects_bad_arguments_without_a_gpu():
    from powerpaint_amd import _lib as L
    lib = L.lib()
    hid, skip, out, bs, acc = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000      # (never dereferenced: every call is refused)

    def call(hidden=hid, hidden_out=hid, ch=1280, skp=skip, skip_out=out, cs=640, batch=2, h=16, w=16, bs_=bs, acc_=acc,
             groups=32, dtype=L.PP_DT_BF16):
        return lib.pp_freeu(hidden, hidden_out, ch, skp, skip_out, cs, batch, h, w, bs_, acc_, groups, dtype, None)

    bad = -1                                  # PP_ERR_BAD_ARG
    assert call(hidden=None) == bad and call(skp=None) == bad and call(skip_out=None) == bad and call(bs_=None) == bad
    assert call(hidden_out=None) == bad
    assert call(hidden=hid + 2, hidden_out=hid + 2) == bad and call(skp=skip + 1) == bad          # misaligned tensors
    assert call(acc_=acc + 4) == bad                                                              # misaligned accumulator
    assert call(h=1) == bad and call(w=1) == bad
    assert call(ch=1282) == bad                                                                   # Ch / 2 odd
    assert call(cs=641) == bad
    assert call(dtype=L.PP_DT_F32) == bad and call(dtype=7) == bad
    assert call(groups=7) == bad                                                                  # (Ch + Cs) % groups
    assert call(skip_out=hid) == bad                                                              # the tensors alias each other
    assert call(batch=0) == bad


def _plan_names(freeu, boc=(320, 320, 640, 640), L_=1, hw=64):
    from powerpaint_amd.engine import SDNet
    from powerpaint_amd.runtime import NetRuntime
    net = SDNet("unet", 9, block_out_channels=boc, layers_per_block=L_)
    net.load_state_dict(net.synthetic_state_dict(meta=True), "cpu", materialize=False)
    rt = NetRuntime(net, "cpu")
    rt.ensure(2, hw, hw, 77, 9, ("plain",), freeu=freeu)
    return rt, [c[2] for c in rt.step_plan.calls]


@pytest.mark.parametrize("boc,L_,n", [((320, 320, 640, 640), 1, 4), ((320, 640, 1280, 1280), 2, 6)])
def test_plan_gains_one_launch_per_affected_resnet(boc, L_, n):
    """FreeU costs exactly one launch in front of every resnet of up blocks 0 and 1 (4 at the fixture architecture, 6 on
    SD-1.5), which also hands norm1 its statistics: no groupnorm_stats launch appears, nothing else changes."""
    _, off = _plan_names(None, boc, L_)
    rt, on = _plan_names((0.9, 0.2, 1.5, 1.6), boc, L_)
    assert off.count("freeu") == 0 and on.count("freeu") == n
    assert on.count("groupnorm_stats") == 0 and off.count("groupnorm_stats") == 0
    assert len(on) == len(off) + n
    assert [x for x in on if x != "freeu"] == off
    # every pp_freeu launch carries an accumulator, and its (b, s) pointer is the block's pair of the device buffer
    base = rt.lay["freeu"]
    calls = [c for c in rt.step_plan.calls if c[2] == "freeu"]
    assert all(c[1][10] for c in calls)
    per_block = n // 2
    assert [c[1][9] for c in calls] == [base] * per_block + [base + 8] * per_block
    assert torch.equal(rt.arena.view(base, (4,), torch.float32), torch.tensor([1.5, 0.9, 1.6, 0.2]))
    # new values: the same plan object, the buffer rewritten
    plan = rt.step_plan
    rt.ensure(2, 64, 64, 77, 9, ("plain",), freeu=(0.9, 0.2, 1.2, 1.6))
    assert rt.step_plan is plan
    assert torch.equal(rt.arena.view(base, (4,), torch.float32), torch.tensor([1.2, 0.9, 1.6, 0.2]))
    # off again: the plan of a UNet without FreeU
    rt.ensure(2, 64, 64, 77, 9, ("plain",), freeu=None)
    assert [c[2] for c in rt.step_plan.calls] == off and "freeu" not in rt.lay


@pytest.mark.parametrize("kind", ["brushnet", "controlnet"])
def test_plan_with_side_network_residuals(kind):
    """The other two pipelines' UNet wirings.  BrushNet: the up_block_add_samples ride the producers' epilogues, so the hidden
    tensor a pp_freeu launch scales already holds the sum (unet_2d_blocks.py:2629-2630 of the reference).  ControlNet: the
    skip tensor it filters is the one the residual add wrote (unet_2d_condition.py:1263-1272)."""
    from powerpaint_amd.engine import SDNet
    from powerpaint_amd.runtime import NetRuntime
    net = SDNet("unet", 4 if kind == "brushnet" else 9, block_out_channels=(320, 320, 640, 640), layers_per_block=1)
    net.load_state_dict(net.synthetic_state_dict(meta=True), "cpu", materialize=False)
    rt = NetRuntime(net, "cpu")
    shapes = rt._residual_shapes(2, 64, 64, with_up=(kind == "brushnet"))
    wiring = (kind, {k: [0] * len(v) for k, v in shapes.items()})
    cin = 4 if kind == "brushnet" else 9
    rt.ensure(2, 64, 64, 77, cin, wiring)
    off = [c[2] for c in rt.step_plan.calls]
    rt.ensure(2, 64, 64, 77, cin, wiring, freeu=(0.9, 0.2, 1.5, 1.6))
    calls = rt.step_plan.calls
    on = [c[2] for c in calls]
    assert on.count("freeu") == 4
    if kind == "brushnet":
        assert [n for n in on if n != "freeu"] == off and on.count("groupnorm_stats") == 0
    else:
        # the sums pp_add_bf16 writes have no epilogue to take statistics in: without FreeU every up-block norm1 keeps its
        # statistics launch; the four FreeU'd resnets lose theirs to the pp_freeu launch
        assert len(on) == len(off) and on.count("groupnorm_stats") == off.count("groupnorm_stats") - 4
        added = {c[1][2] for c in calls if c[2] == "add"}               # outputs of the residual adds
        assert all(c[1][3] in added for c in calls if c[2] == "freeu")  # ... are the skip tensors FreeU filters


def test_freeu_at_a_latent_size_whose_levels_are_odd():
    """576^2 images: the 8x8 level is 9x9 (72x72 latents).  The launches still carry the statistics (the kernel needs no
    whole 64-row tiles), so no groupnorm_stats launch appears at the FreeU'd resnets that was not there without FreeU."""
    _, off = _plan_names(None, hw=72)
    _, on = _plan_names((0.9, 0.2, 1.5, 1.6), hw=72)
    assert on.count("freeu") == 4 and on.count("groupnorm_stats") == off.count("groupnorm_stats") - 4


def test_model_methods_follow_the_reference_truthiness_rule():
    from powerpaint_amd.models import UNet2DConditionModel as U
    u = U.__new__(U)                       # (the methods touch no device state)
    assert u._freeu_values() is None
    assert u.enable_freeu(s1=0.9, s2=0.2, b1=1.5, b2=1.6) is u and u._freeu_values() == (0.9, 0.2, 1.5, 1.6)
    for kw in (dict(s1=0, s2=0.2, b1=1.5, b2=1.6), dict(s1=0.9, s2=0.2, b1=1.5, b2=None)):
        u.enable_freeu(**kw)
        assert u._freeu_values() is None          # any value of 0 or None: off, as `getattr(...) and ...` in the up blocks
    u.enable_freeu(0.9, 0.2, 1.5, 1.6)
    u.disable_freeu()
    assert u._freeu_values() is None
    from powerpaint_amd.models import BrushNetModel, ControlNetModel
    assert not hasattr(BrushNetModel, "enable_freeu") and not hasattr(ControlNetModel, "enable_freeu")
