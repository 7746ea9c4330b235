"""-m gpu: FreeU on the HIP path -- the pp_freeu kernel against the torch.fft restatement, the UNet with
`enable_freeu` against the reference's own UNet (tests/golden/ref_freeu.pt), the launch plan, and the fused loop.

Achieved parity numbers are printed and appended to profiles/freeu_parity_achieved.txt before anything is asserted.
"""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import freeu_cases as FC  # noqa: E402
from powerpaint_amd import models as PM  # noqa: E402
from powerpaint_amd import ops  # noqa: E402
from powerpaint_amd import pipelines as PP  # noqa: E402
from powerpaint_amd import schedulers as PS  # noqa: E402

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
FULL = (0.9, 0.2, 1.5, 1.6)          # (s1, s2, b1, b2)


def record(line: str):
    print(line)
    try:
        with open(os.path.join(ROOT, "profiles", "freeu_parity_achieved.txt"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


# ------------------------------------------------------------------------------------------------ 1. the op
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", FC.OP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pp_freeu_against_the_restatement(shape, dtype):
    """The restatement runs in fp32 on the 16-bit inputs and is rounded once.  |out - ref| <= ulp16(ref) + 1e-5 max|x|: both
    sides are fp32 before one rounding, an fp32 discrepancy can flip that rounding by one unit, and the absolute term is x14
    over the 7.2e-7 fp32 discrepancy between the closed form and the FFT (tests/test_freeu.py).
    Statistics: the accumulator against the exact sums of the STORED outputs, and through pp_groupnorm_apply_acc against
    torch's group_norm of the stored outputs, both at rtol 1e-4 / atol 1e-2 (the bounds of the epilogue-statistics test,
    tests/test_ops_gpu.py).  The norm's gamma is ~0.2 so that |y| < 2 (|z| < 6 over a group that mixes scaled and plain
    channels, gamma < 0.3): the bound then covers the one rounding of y to 16 bits (half a bf16 ulp below 2 is 3.9e-3) next
    to the ~1e-4 the statistics may be off."""
    B, H, W, Ch, Cs = shape
    b, s = 1.5, 0.2
    hid, skip = (t.to(DEV) for t in FC.op_inputs(shape, dtype))
    Ct, groups = Ch + Cs, 32
    with_stats = Ct // groups >= 8
    acc = torch.zeros(B, groups, 2, dtype=torch.int64, device=DEV) if with_stats else None
    ho, so = ops.freeu(hid, skip, b, s, acc=acc, groups=groups)
    torch.cuda.synchronize()
    # outputs
    ref_h = hid.float().clone()
    ref_h[..., :Ch // 2] *= b
    ref_s = FC.fourier_filter(skip.float().permute(0, 3, 1, 2), threshold=1, scale=s).permute(0, 2, 3, 1)
    assert torch.equal(ho[..., Ch // 2:], hid[..., Ch // 2:]), "untouched backbone channels changed"
    assert torch.equal(ho[..., :Ch // 2], ref_h[..., :Ch // 2].to(dtype)), "scaled backbone half: fp32 product, one rounding"
    err = (so.float() - ref_s).abs()
    tol = FC.ulp16(ref_s, dtype) + 1e-5 * float(skip.float().abs().max())
    record(f"[freeu] op {shape} {dtype}: skip max err {float(err.max()):.4g}, worst err / tol {float((err / tol).max()):.3f}, "
           f"moved by the filter {float((ref_s - skip.float()).abs().max()):.3g}")
    assert (err <= tol).all(), (shape, float(err.max()), float((err / tol).max()))
    assert float((ref_s - skip.float()).abs().max()) > 0.05          # (the filter really acts on this data)
    # in place (what the launch plans do): the same bits
    h2, s2 = hid.clone(), skip.clone()
    acc2 = torch.zeros_like(acc) if with_stats else None
    ops.freeu(h2, s2, b, s, acc=acc2, groups=groups, inplace=True)
    assert torch.equal(h2, ho) and torch.equal(s2, so)
    if not with_stats:
        return
    assert torch.equal(acc2, acc)                                    # integer accumulation: order-independent
    cat = torch.cat([ho, so], -1).double().reshape(B, H * W, groups, Ct // groups)
    want = torch.stack([cat.sum((1, 3)), (cat ** 2).sum((1, 3))], -1)
    got = torch.stack([acc[..., 0].double() / 2 ** 24, acc[..., 1].double() / 2 ** 20], -1)
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-2), (shape, float((got - want).abs().max()))
    g = torch.Generator("cpu").manual_seed(5)
    gamma = (0.2 * (1 + 0.1 * torch.randn(Ct, generator=g))).to(DEV)
    beta = (0.1 * torch.randn(Ct, generator=g)).to(DEV)
    y = ops.groupnorm_apply_acc(ho, acc, gamma, beta, 1e-5, False, groups=groups, x2=so)
    ref_y = F.group_norm(torch.cat([ho, so], -1).float().permute(0, 3, 1, 2), groups, gamma, beta, 1e-5).permute(0, 2, 3, 1)
    assert float(ref_y.abs().max()) < 2.0
    assert torch.allclose(y.float(), ref_y, rtol=1e-4, atol=1e-2), (shape, float((y.float() - ref_y).abs().max()))


# ------------------------------------------------------------------------------------------------ 2. the network
@functools.lru_cache(maxsize=None)
def _oracle_state_dicts():
    import make_ref_wiring as W
    u9, u4 = W.oracle_models()
    cfg = dict(W.CFG)
    cfg.pop("attention_head_dim")
    return u9.state_dict(), u4.state_dict(), cfg


@functools.lru_cache(maxsize=None)
def _gold():
    return torch.load(os.path.join(HERE, "golden", "ref_freeu.pt"), weights_only=False)


def _gate(out, ref, what):
    """The gate tests/test_golden.py applies to this architecture: cosine >= 0.999, max err <= 3e-2 max(1, max|ref|)."""
    cos, err, ok = FC.close_gate(out, ref)
    record(f"[freeu] {what}: cosine {cos:.6f}  max-abs {err:.4g}  (max|ref| {float(ref.abs().max()):.4g})")
    assert ok, f"{what}: cos {cos:.6f} err {err:.4g}"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_unet_with_freeu_reproduces_the_reference(dtype):
    """The 9-channel UNet under the three settings of the fixture, then `disable_freeu` -> the bits of a forward pass taken
    before FreeU was ever enabled.  On a tree without the feature the method does not exist, and the plain output misses
    the gate by the margins the fixture carries."""
    sd9, _, cfg = _oracle_state_dicts()
    G, inp = _gold(), FC.net_inputs()
    h9 = PM.UNet2DConditionModel(in_channels=9, device=DEV, dtype=dtype, **cfg).load_state_dict(sd9)
    run = lambda: h9(inp["x9"].to(DEV), inp["t"], inp["ehs"].to(DEV), return_dict=False)[0].clone()      # noqa: E731
    before = run()
    _gate(before, G["eps9_plain"], f"9-channel UNet plain {dtype}")
    for name, kw in G["settings"].items():
        h9.enable_freeu(**kw)
        out = run()
        _gate(out, G[f"eps9_{name}"], f"9-channel UNet FreeU {name} {dtype}")
        assert not FC.close_gate(before, G[f"eps9_{name}"])[2]
    h9.disable_freeu()
    assert torch.equal(run(), before)
    h9.enable_freeu(s1=0.9, s2=0.2, b1=1.5, b2=0)          # one falsy value: off
    assert torch.equal(run(), before)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_fork_unet_with_brushnet_residuals_and_freeu(dtype):
    """The hidden tensor FreeU scales is the sum with the up_block_add_samples (unet_2d_blocks.py:2629-2630 of the reference)."""
    _, sd4, cfg = _oracle_state_dicts()
    G, inp = _gold(), FC.net_inputs()
    h4 = PM.UNet2DConditionModel(in_channels=4, device=DEV, dtype=dtype, **cfg).load_state_dict(sd4)
    dev = lambda lst: [t.to(DEV) for t in lst]      # noqa: E731
    run = lambda: h4(inp["x4"].to(DEV), inp["t"], inp["ehs"].to(DEV), down_block_add_samples=dev(inp["down"]),      # noqa: E731
                     mid_block_add_sample=inp["mid"].to(DEV), up_block_add_samples=dev(inp["up"]), return_dict=False)[0].clone()
    before = run()
    _gate(before, G["eps4_brush_plain"], f"fork UNet + residuals plain {dtype}")
    h4.enable_freeu(**FC.FREEU_FULL)
    _gate(run(), G["eps4_brush_full"], f"fork UNet + residuals FreeU full {dtype}")
    h4.disable_freeu()
    assert torch.equal(run(), before)


# ------------------------------------------------------------------------------------------------ 3. the plan
def test_plan_launch_names_before_and_after_enable_freeu():
    sd9, _, cfg = _oracle_state_dicts()
    inp = FC.net_inputs()
    h9 = PM.UNet2DConditionModel(in_channels=9, device=DEV, **cfg).load_state_dict(sd9)
    names = lambda: [c[2] for c in h9.prepare(tuple(inp["x9"].shape), inp["ehs"].to(DEV)).step_plan.calls]      # noqa: E731
    off = names()
    h9.enable_freeu(*FULL)
    on = names()
    assert on.count("freeu") == 4 and off.count("freeu") == 0          # one per resnet of up blocks 0 and 1 (6 on full SD-1.5)
    assert on.count("groupnorm_stats") == 0
    assert len(on) <= len(off) + 4 and [n for n in on if n != "freeu"] == off
    h9.disable_freeu()
    assert names() == off


# ------------------------------------------------------------------------------------------------ 4. the fused loop
def _duck_loop(unet, lat, mask2, mil2, pe, steps, g_scale):
    """The step-by-step loop over `unet.forward` with the oracle's DDIM scheduler on the host (ppt-v1 loop body,
    pipeline_PowerPaint.py:990-1023 of the reference)."""
    from oracle import schedulers as OS
    sch = OS.DDIMScheduler()
    sch.set_timesteps(steps)
    lat = lat.clone() * sch.init_noise_sigma
    for t in sch.timesteps:
        x = torch.cat([torch.cat([lat] * 2), mask2, mil2], 1)
        eps = unet(x.to(DEV), t, pe.to(DEV), return_dict=False)[0].float().cpu()
        u, c = eps.chunk(2)
        lat = sch.step(u + g_scale * (c - u), t, lat)[0]
    return lat


def test_fused_loop_follows_enable_freeu_value_changes_and_disable():
    """v1 pipeline, 64x64 latents, 3 DDIM steps, captured graph.  FreeU on: the fused loop against the step-by-step loop
    over unet.forward within the bound tests/test_golden.py uses for fused against duck-typed (cosine >= 0.9997), and beyond
    that bound away from the plain latents.  New values (b1 1.5 -> 1.2) reach the captured graph; disable -> the first run's
    bits."""
    sd9, _, cfg = _oracle_state_dicts()
    h9 = PM.UNet2DConditionModel(in_channels=9, device=DEV, **cfg).load_state_dict(sd9)
    hd = PM.UNet2DConditionModel(in_channels=9, device=DEV, **cfg).load_state_dict(sd9)      # (the step-by-step side: its own plans)
    g = torch.Generator("cpu").manual_seed(11)
    s = 64
    lat = torch.randn(1, 4, s, s, generator=g)
    mask = torch.zeros(1, 1, s, s)
    mask[:, :, 16:48, 16:48] = 1
    mil = torch.randn(1, 4, s, s, generator=g) * 0.5
    pe = torch.randn(2, 77, 768, generator=g)
    pipe = PP.StableDiffusionInpaintPipeline(unet=h9, scheduler=PS.DDIMScheduler())
    assert pipe.use_graph

    def fused():
        return pipe(prompt_embeds=pe[1:].to(DEV), negative_prompt_embeds=pe[:1].to(DEV), height=s * 8, width=s * 8,
                    num_inference_steps=3, guidance_scale=7.5, latents=lat.to(DEV), mask_latents=mask.to(DEV),
                    masked_image_latents=mil.to(DEV), output_type="latent", return_dict=False)[0].float().cpu().clone()

    cosine = lambda a, b: F.cosine_similarity(a.flatten(), b.flatten(), dim=0).item()      # noqa: E731
    plain = fused()
    h9.enable_freeu(*FULL)
    on = fused()
    graph = pipe._loop.graph
    assert graph is not None
    duck = _duck_loop(hd.enable_freeu(*FULL), lat, torch.cat([mask] * 2), torch.cat([mil] * 2), pe, 3, 7.5)
    record(f"[freeu] fused loop, FreeU on: cosine vs step-by-step {cosine(on, duck):.6f}, vs plain {cosine(on, plain):.6f}")
    assert cosine(on, duck) >= 0.9997
    assert cosine(on, plain) < 0.9997
    h9.enable_freeu(s1=0.9, s2=0.2, b1=1.2, b2=1.6)
    on2 = fused()
    assert pipe._loop.graph is graph          # the values are read from device memory: the captured graph is replayed as it is
    duck2 = _duck_loop(hd.enable_freeu(s1=0.9, s2=0.2, b1=1.2, b2=1.6), lat, torch.cat([mask] * 2), torch.cat([mil] * 2), pe, 3, 7.5)
    record(f"[freeu] fused loop, b1 = 1.2: cosine vs step-by-step {cosine(on2, duck2):.6f}, vs b1 = 1.5 {cosine(on2, on):.6f}")
    assert not torch.equal(on2, on) and cosine(on2, duck2) >= 0.9997
    h9.disable_freeu()
    assert torch.equal(fused(), plain)
