"""-m gpu: the sub-pixel form of Upsample2D's `nearest 2x -> conv3x3` (PPGemmArgs.subpix: four 2x2 convs over the source image
on weights folded by pp_upconv_fold, csrc/conv_gn.hip NMODE 4) through the C ABI, and in the step plans.

Checkers per operator case, references computed once per (shape, dtype) on the CPU in fp32 (tests/upconv_cases.py):
  fold     ops.upconv_fold == the torch fold, bit for bit (fp32 sums in the same order, one rounding)
  exact    the launch against four fp32 2x2 convs ON THE FOLDED 16-bit WEIGHTS: the same operands on both sides, only the order
           of the fp32 sums and the output rounding differ -> the kernel-against-kernel gate, 2 ulp + 1.5 ulp |ref|; the border
           rows and columns of the output (where each parity's padding acts) are also judged on their own
  op       the same output against fp32 upsample + conv3x3 on the UNFOLDED weights at the gate of this op against fp32 torch,
           3e-2 tol + 1e-2 tol |ref| (tol 1 bf16, 0.25 fp16): what the second rounding of the folded weights adds lies inside
The shapes are the smallest that reach every branch: 64- / 128- / 256-row tiles, one to five 64-channel chunks (the three-stage
weight ring wraps at every chunk count that is no multiple of three), two images, a partial column tile, 2 .. 5 halo strips
per wave, non-square.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import engine as ENG  # noqa: E402
from powerpaint_amd import ops  # noqa: E402
import upconv_cases as U  # noqa: E402

DEV = "cuda"
SHAPES = [
    (2, 8, 8, 128, 160),       # 64-row tile, two chunks, two images
    (1, 16, 16, 192, 320),     # 256-row tile, three chunks = one full period of the weight ring + wrap
    (2, 16, 16, 64, 96),       # partial column tile, a single chunk
    (1, 8, 16, 128, 160),      # non-square (128-row tile)
    (1, 32, 32, 320, 160),     # 5 halo strips per wave; five chunks; four tiles per image
]
DTYPES = [torch.bfloat16, torch.float16]
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator("cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@functools.lru_cache(maxsize=None)
def case(shape, dtype):
    """Inputs, the launch's output and both fp32 references of one (shape, dtype); computed once, never modified."""
    B, H, W, C, Cout = shape
    x = rnd(B, H, W, C, seed=1).to(dtype)
    w = rnd(Cout, 9 * C, seed=2, scale=(9 * C) ** -0.5).to(dtype).contiguous()
    bias = rnd(Cout, seed=3)
    wf_ref = U.fold(w, dtype)
    assert ops.upconv_subpix_supported(x.to(DEV), Cout) >= 1
    wf = ops.upconv_fold(w.to(DEV))
    out = ops.conv3x3_up_subpix(x.to(DEV), wf, bias.to(DEV))
    torch.cuda.synchronize()
    return dict(x=x, w=w, bias=bias, wf_ref=wf_ref, wf=wf.cpu(), out=out.float().cpu(),
                ref_fold=U.subpix_conv(x, wf_ref, bias), ref_op=U.up_conv(x, w, bias))


def check(out, ref, atol, rtol, what):
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    err = (out - ref).abs()
    bad = err > atol + rtol * ref.abs()
    print(f"{what}: max abs err {float(err.max()):.4g}, worst err / gate {float((err / (atol + rtol * ref.abs())).max()):.3f}, "
          f"ref max {float(ref.abs().max()):.4g}")
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off; max abs err {float(err.max()):.4g}"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fold_kernel_is_the_torch_fold(shape, dtype):
    c = case(shape, dtype)
    assert c["wf"].shape == (4, shape[4], 4 * shape[3])
    assert torch.equal(c["wf"], c["wf_ref"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_subpix_conv_against_fp32_2x2_convs_on_the_folded_weights(shape, dtype):
    c = case(shape, dtype)
    out, ref, ulp = c["out"], c["ref_fold"], ULP[dtype]
    check(out, ref, 2 * ulp, 1.5 * ulp, "sub-pixel conv vs fp32 2x2 convs on the folded weights")
    # the two outermost rows / columns on every side hold the border pixels of all four parities
    for name, sl in (("top", (slice(None), slice(0, 2))), ("bottom", (slice(None), slice(-2, None))),
                     ("left", (slice(None), slice(None), slice(0, 2))), ("right", (slice(None), slice(None), slice(-2, None)))):
        check(out[sl], ref[sl], 2 * ulp, 1.5 * ulp, f"border {name}")
    for a in (0, 1):
        for b in (0, 1):
            check(out[:, a::2, b::2], ref[:, a::2, b::2], 2 * ulp, 1.5 * ulp, f"parity ({a}, {b})")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_subpix_conv_against_fp32_upsample_conv_on_the_unfolded_weights(shape, dtype):
    c = case(shape, dtype)
    tol = 1.0 if dtype == torch.bfloat16 else 0.25
    check(c["out"], c["ref_op"], 3e-2 * tol, 1e-2 * tol, "sub-pixel conv vs fp32 upsample + conv3x3")


def stats_of(out, cg, c0, groups):
    """int64-valued (sum, sum of squares) per (batch item, group) of the STORED output [B,H,W,N] as a consumer whose groups are
    cg channels wide and that sees column n as its channel c0 + n would accumulate them (fixed point of PPGemmArgs.gn_acc)."""
    B, N = out.shape[0], out.shape[3]
    o = out.double().reshape(B, -1, N)
    gi = (torch.arange(N) + c0) // cg
    acc = torch.zeros(B, groups, 2, dtype=torch.float64)
    acc[:, :, 0].index_add_(1, gi, o.sum(1) * 2 ** 24)
    acc[:, :, 1].index_add_(1, gi, (o * o).sum(1) * 2 ** 20)
    return acc


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape,groups", [((1, 16, 16, 192, 320), 32), ((2, 8, 8, 128, 160), 16), ((1, 32, 32, 320, 160), 16)],
                         ids=["16x16", "8x8x2", "32x32"])
def test_epilogue_operands_and_output_statistics(shape, groups, dtype):
    """bias, res1, res2 (the BrushNet add_up residual rides here) and two statistics subscriptions, one of them a concatenated
    consumer: deterministic, equal to the plain launch + the operands, and accumulators that describe the stored output."""
    B, H, W, C, Cout = shape
    c = case(shape, dtype)
    x, wf, bias = c["x"].to(DEV), c["wf"].to(DEV), c["bias"].to(DEV)
    res1 = rnd(B, 2 * H, 2 * W, Cout, seed=5).to(dtype).to(DEV)
    res2 = rnd(B, 2 * H, 2 * W, Cout, seed=6).to(dtype).to(DEV)

    def subs():
        A = [torch.zeros(B, groups, 2, dtype=torch.int64, device=DEV) for _ in range(2)]
        return A, [(A[0], (Cout + 320) // groups, 320, groups), (A[1], Cout // groups, 0, groups)]

    A1, s1 = subs()
    out = ops.conv3x3_up_subpix(x, wf, bias, res1=res1, res2=res2, gn=s1)
    A2, s2 = subs()
    out2 = ops.conv3x3_up_subpix(x, wf, bias, res1=res1, res2=res2, gn=s2)
    assert torch.equal(out, out2), "not deterministic"
    ulp = ULP[dtype]
    ref = c["ref_fold"] + res1.float().cpu() + res2.float().cpu()
    check(out.float().cpu(), ref, 2 * ulp, 1.5 * ulp, "with bias + res1 + res2")
    for k, (_, cg, c0, g_) in enumerate(s1):
        assert torch.equal(A1[k], A2[k]), f"accumulators of subscription {k} differ between two runs"
        want = stats_of(out.cpu(), cg, c0, g_)
        rel = ((A1[k].cpu().double() - want).abs() / (want.abs() + 2.0 ** 20)).max().item()
        print(f"subscription {k}: accumulators vs the stored output, rel {rel:.3g}")
        assert rel < 2e-3, f"output GroupNorm statistics (consumer {k}) do not describe the stored output: {rel:.3g}"


def test_unsupported_requests_are_refused_and_launch_nothing():
    """A source narrower than the loader's 8-pixel strips and a forced split: PP_ERR_UNSUPPORTED from the form resolution, in
    front of any launch (the output buffer keeps its bytes)."""
    import ctypes as C
    lib = L.lib()
    for (B, H, W, Cin, Cout, splitk) in [(2, 4, 4, 128, 160, 0), (2, 16, 16, 128, 160, 2)]:
        x = rnd(B, H, W, Cin, seed=1).bfloat16().to(DEV)
        wf = torch.zeros(4, Cout, 4 * Cin, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(L.PPError, match="PP_ERR_UNSUPPORTED"):
            ops.conv3x3_up_subpix(x, wf, splitk=splitk)
        out = torch.full((B, 2 * H, 2 * W, Cout), 3.0, dtype=torch.bfloat16, device=DEV)
        a = L.conv3x3_args(L.PP_DT_BF16, B, H, W, Cin, Cout, x.data_ptr(), w=wf.data_ptr(), out=out.data_ptr())
        a.K, a.subpix, a.splitk = 4 * Cin, 1, splitk
        assert lib.pp_gemm_bf16(C.byref(a), torch.cuda.current_stream().cuda_stream) == -2
        torch.cuda.synchronize()
        assert bool((out == 3.0).all())
    assert ops.upconv_subpix_supported(torch.empty(2, 4, 4, 128, dtype=torch.bfloat16, device=DEV), 160) == 0


# ---------------------------------------------------------------------------------------------------------- in the step plans
from oracle import sd_modules as OM  # noqa: E402
from powerpaint_amd import models as PM  # noqa: E402
from test_models_gpu import TINY, _record_achieved, bf16_weights_, close, gen  # noqa: E402

HL = 32       # latents: the reduced network's only upsampler then reads a 16 x 16 x 640 source, which the plans route


def subpix_launches(h):
    out = []
    for fn, args, name in h.rt.step_plan.calls:
        a = getattr(args[0], "_obj", None) if args else None
        if isinstance(a, L.PPGemmArgs) and a.subpix:
            out.append((name, a))
    return out


def up_launches(h):
    return [a for fn, args, name in h.rt.step_plan.calls
            for a in [getattr(args[0], "_obj", None) if args else None] if isinstance(a, L.PPGemmArgs) and a.up]


@functools.lru_cache(maxsize=None)
def tiny_unet():
    torch.manual_seed(0)
    o = bf16_weights_(OM.UNet2DConditionModel(in_channels=9, **TINY)).eval()
    x, e = gen(2, 9, HL, HL, seed=1), gen(2, 77, 768, seed=2)
    with torch.no_grad():
        ref = o(x, 500, e)[0]
    return o, x, e, ref


def hip_unet(sd):
    return PM.UNet2DConditionModel(in_channels=9, device=DEV, **TINY).load_state_dict(sd)


def test_unet_with_the_form_on_and_off_against_the_oracle(monkeypatch):
    o, x, e, ref = tiny_unet()
    h_on = hip_unet(o.state_dict())
    out_on = h_on(x.to(DEV), 500, e.to(DEV), return_dict=False)[0]
    on = subpix_launches(h_on)
    assert len(on) == 1 and on[0][0] == "conv3x3" and not up_launches(h_on), "the 16 -> 32 upsampler did not take the form"
    a = on[0][1]
    assert (a.hin, a.win, a.c1, a.N, a.K, a.M) == (HL // 2, HL // 2, 640, 640, 4 * 640, 2 * (HL // 2) ** 2)
    assert any(name == "upconv_fold" for _, _, name in h_on.rt.setup_plan.calls)
    monkeypatch.setattr(ENG, "UPCONV_SUBPIX", False)
    h_off = hip_unet(o.state_dict())
    out_off = h_off(x.to(DEV), 500, e.to(DEV), return_dict=False)[0]
    assert not subpix_launches(h_off) and len(up_launches(h_off)) == 1
    assert not any(name == "upconv_fold" for _, _, name in h_off.rt.setup_plan.calls)
    assert len(h_off.rt.step_plan.calls) == len(h_on.rt.step_plan.calls)
    cos_on, err_on = close(out_on, ref, "unet tiny 32x32, sub-pixel upsampler")
    cos_off, err_off = close(out_off, ref, "unet tiny 32x32, nine-tap upsampler")
    cos = torch.nn.functional.cosine_similarity(out_on.float().flatten(), out_off.float().flatten(), dim=0).item()
    d = (out_on.float() - out_off.float()).abs().max().item()
    print(f"on vs off: cosine {cos:.7f} max-abs {d:.4g}; vs oracle on {cos_on:.7f} / {err_on:.4g}, off {cos_off:.7f} / {err_off:.4g}")
    _record_achieved("unet tiny 32x32, sub-pixel upsampler on vs off", cos, d, out_off.float().abs().max().item(), "none", float("nan"))
    # the plan's `flops` stay the algorithm's; what the launches execute is 5/9 of the routed conv's MACs less
    p_on, p_off = h_on.rt.step_plan, h_off.rt.step_plan
    assert p_on.flops == p_off.flops == p_off.flops_executed
    assert p_on.flops - p_on.flops_executed == 5 * 2.0 * a.M * a.N * a.K


def test_brushnet_into_unet_both_take_the_form():
    """Both kinds: the BrushNet's own upsampler, and the UNet's with the BrushNet `add_up` residual in its epilogue (res2 at the
    scattered output rows)."""
    torch.manual_seed(0)
    ob = bf16_weights_(OM.randomize_zero_convs(OM.BrushNetModel(in_channels=4, conditioning_channels=5, **TINY))).eval()
    hb = PM.BrushNetModel(in_channels=4, conditioning_channels=5, device=DEV, **TINY).load_state_dict(ob.state_dict())
    torch.manual_seed(1)
    ou = bf16_weights_(OM.UNet2DConditionModel(in_channels=4, **TINY)).eval()
    hu = PM.UNet2DConditionModel(in_channels=4, device=DEV, **TINY).load_state_dict(ou.state_dict())
    x, e, eu, cond = gen(2, 4, HL, HL, seed=1), gen(2, 77, 768, seed=2), gen(2, 77, 768, seed=3), gen(2, 5, HL, HL, seed=4)
    with torch.no_grad():
        dn, md, up = ob(x, 321, e, cond, conditioning_scale=0.8)
        ref = ou(x, 321, eu, down_block_add_samples=list(dn), mid_block_add_sample=md, up_block_add_samples=list(up))[0]
    hdn, hmd, hup = hb(x.to(DEV), 321, e.to(DEV), cond.to(DEV), conditioning_scale=0.8, return_dict=False)
    for i, (a, b) in enumerate(zip(hdn + [hmd] + hup, list(dn) + [md] + list(up))):
        close(a, b, f"brushnet 32x32 (sub-pixel upsampler) residual {i}", cos_min=0.998)
    out = hu(x.to(DEV), 321, eu.to(DEV), down_block_add_samples=list(hdn), mid_block_add_sample=hmd,
             up_block_add_samples=list(hup), return_dict=False)[0]
    close(out, ref, "unet(+brushnet) 32x32, sub-pixel upsamplers")
    assert len(subpix_launches(hb)) == 1 and len(subpix_launches(hu)) == 1
    assert subpix_launches(hu)[0][1].res2, "the add_up residual did not ride the sub-pixel launch"


def _step(h, x, e, use_graph):
    rt = h.prepare(tuple(x.shape), e)
    rt.load_input([(x, 0)])
    rt.set_timestep(500)
    rt.run_step(use_graph=use_graph)
    return rt.eps_tensor().clone()


def test_graph_replay_equals_eager_with_the_form_on():
    o, x, e, _ = tiny_unet()
    h = hip_unet(o.state_dict())
    xd, ed = x.to(DEV), e.to(DEV)
    eager = _step(h, xd, ed, False)
    assert subpix_launches(h)
    graph = _step(h, xd, ed, True)
    assert h.rt.graph is not None and torch.equal(eager, graph)
    assert torch.equal(graph, _step(h, xd, ed, True))


def test_rewritten_upsampler_weight_reaches_the_folded_buffer():
    """The folded buffer is a cache of the packed weight: after an in-place rewrite + params_changed() the model answers as
    one freshly loaded with that weight (a stale fold would leave the old upsampler in the captured step)."""
    o, x, e, _ = tiny_unet()
    key = "up_blocks.0.upsamplers.0.conv.weight"
    h = hip_unet(o.state_dict())
    xd, ed = x.to(DEV), e.to(DEV)
    before = _step(h, xd, ed, True)
    assert subpix_launches(h)
    h.net.params.tensor(key).mul_(-0.5)          # (exact in the 16-bit format: the fresh model packs the same bits)
    h.params_changed()
    after = _step(h, xd, ed, True)
    sd = {k: v.clone() for k, v in o.state_dict().items()}
    sd[key] = sd[key] * -0.5
    fresh = _step(hip_unet(sd), xd, ed, True)
    assert not torch.equal(before, after)
    assert torch.equal(after, fresh)
