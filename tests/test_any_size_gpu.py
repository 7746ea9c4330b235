"""-m gpu: latent sizes that are no multiple of 2^(levels - 1) on the HIP path.

  1. PP_X_CONV3X3 with up = 1 and a cropped target (ABI v29), and the stride-2 conv on an odd input, against fp64 torch under
     the derived gate of tests/gemm_cases.py
  2. the other entry points the odd-size step plans launch, each at its smallest odd shape under the gate of its existing test
  3. UNet / BrushNet / ControlNet against the reference's own networks (tests/golden/ref_any_size.pt), bf16 and fp16, eager
     and graph replay; FreeU at 13x10
  4. the three pipelines against the reference's own `__call__`s at a 104x80 image, twin prefix asked for and not
  5. the VAE at 130 and 99 tokens, pad columns of P on a poisoned arena
  6. the controller with a 4:3 photo

Every comparison prints its achieved numbers and appends them to profiles/any_size_parity_achieved.txt before it asserts.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import freeu_cases as FC  # noqa: E402
import gemm_cases as GC  # noqa: E402
import norm_cases as NC  # noqa: E402
from oracle import vae as OV  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import engine as ENG  # noqa: E402
from powerpaint_amd import models as PM  # noqa: E402
from powerpaint_amd import ops  # noqa: E402
from powerpaint_amd import pipelines as PP  # noqa: E402
from powerpaint_amd import schedulers as PS  # noqa: E402

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
SIZES = [(13, 10), (9, 11), (10, 12)]


def record(line: str):
    print(line)
    try:
        with open(os.path.join(ROOT, "profiles", "any_size_parity_achieved.txt"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator("cpu").manual_seed(seed)) * scale


def check(out, ref, atol, rtol, what):
    """|out - ref| <= atol + rtol |ref| elementwise (tests/test_ops_gpu.py::check), achieved numbers recorded first."""
    out, ref = out.float().cpu(), ref.float().cpu()
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    err = (out - ref).abs()
    worst = float((err / (atol + rtol * ref.abs())).max())
    record(f"[any size] {what}: max abs err {float(err.max()):.4g}, worst err / gate {worst:.3f}, max|ref| {float(ref.abs().max()):.4g}")
    assert torch.isfinite(out).all() and worst <= 1.0, (what, float(err.max()), worst)


def derived(out, ref64, A64, K, splits, what):
    """The derived gate of tests/gemm_cases.py for a K-deep contraction in out's format (gate_rpm), recorded, then asserted."""
    g = GC.gate_rpm(ref64, A64, K, splits, out.dtype)
    r = GC.worst_ratio(out.cpu().reshape(ref64.shape), ref64, g)
    record(f"[any size] {what}: error / derived gate {r:.3f} (K {K}, splits <= {splits})")
    assert r <= 1.0, (what, r)


# ------------------------------------------------------------------------------------------------ 1. the convs
def resize_conv64(x, w, size, stride=1):
    """F.conv2d(F.interpolate(x, size=size), w, padding=1) in fp64 on NHWC x [B,H,W,C], w [Cout, 9 C] (k = (ky*3+kx)*C + c);
    size None: no resize."""
    cout, cin = w.shape[0], x.shape[3]
    xi = x.double().permute(0, 3, 1, 2)
    if size is not None:
        xi = F.interpolate(xi, size=size, mode="nearest")
    w4 = w.double().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    return F.conv2d(xi, w4, None, stride=stride, padding=1).permute(0, 2, 3, 1)


UP_CASES = [((4, 3), (7, 5)), ((4, 3), (8, 5)), ((7, 5), (13, 10)), ((7, 5), (14, 10)), ((8, 8), (15, 16)), ((8, 8), (16, 15))]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ch", [64, 320])
@pytest.mark.parametrize("src,dst", UP_CASES, ids=lambda s: "x".join(map(str, s)))
def test_up_conv_with_a_resize_target(src, dst, ch, dtype):
    """Batch 2; cropped on both axes, on one, on none (7x5 -> 14x10: the geometry of ABI v28, here through `up_size`).  8x8 ->
    15x16 / 16x15: 16 columns would send the exact request to the halo-tile loop, which declines a cropped target -- the
    tap-major kernels run it.  The launch as the plans make it (automatic tile and split) and forced to a single pass."""
    (h, w_), (ho, wo) = src, dst
    x = rnd(2, h, w_, ch, seed=1).to(dtype)
    w = rnd(ch, 9 * ch, seed=2, scale=(9 * ch) ** -0.5).to(dtype).contiguous()
    bias = rnd(ch, seed=3)
    ref = resize_conv64(x, w, dst) + bias.double()
    A = resize_conv64(x.abs(), w.abs(), dst) + bias.double().abs()
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    assert not ops.conv_halo_routed(xd, ch, up=True, up_size=dst) or dst == (2 * h, 2 * w_)
    for splitk in (0, 1):
        out = ops.conv3x3(xd, wd, bd, up=True, up_size=dst, splitk=splitk)
        assert out.shape == (2, ho, wo, ch)
        derived(out, ref, A, 9 * ch, splitk or 8, f"up conv {h}x{w_} -> {ho}x{wo} C {ch} {IDS[DTYPES.index(dtype)]} splitk {splitk}")
    if dst == (2 * h, 2 * w_):      # the unchanged geometry: the bits of the request without a target
        assert torch.equal(out, ops.conv3x3(xd, wd, bd, up=True, splitk=1))
    else:                           # cropping a 2x conv is a different function: its last row / column sees no padding
        full = ops.conv3x3(xd, wd, bd, up=True, splitk=1)[:, :ho, :wo]
        d = (full.float() - out.float()).abs()
        ulp = (2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11) * float(out.float().abs().max())
        inner, edge = float(d[:, :ho - 1, :wo - 1].max()), float(d.max())
        record(f"[any size] 2x conv cropped to {ho}x{wo} against the resize conv: interior {inner:.3g}, border {edge:.3g} (ulp {ulp:.3g})")
        assert inner <= 2 * ulp and edge > 16 * ulp


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_target_equals_the_sub_pixel_form(dtype):
    """The geometry that does not change, 2 h x 2 w, at the smallest source the sub-pixel form takes (rows of 8 pixels: it
    answers 0 for the 7x5 source of the 14x10 case above, asserted here) -- the nine-tap request with `up_size` and the
    sub-pixel launch against fp32 upsample + conv at that form's existing gate (tests/test_upconv_subpix_gpu.py), and each
    other."""
    B, h, w_, ch = 2, 8, 8, 128
    x = rnd(B, h, w_, ch, seed=1).to(dtype).to(DEV)
    w = rnd(160, 9 * ch, seed=2, scale=(9 * ch) ** -0.5).to(dtype).contiguous().to(DEV)
    bias = rnd(160, seed=3).to(DEV)
    assert ops.upconv_subpix_supported(torch.empty(2, 7, 5, 320, dtype=dtype, device=DEV), 320) == 0
    assert ops.upconv_subpix_supported(x, 160) >= 1
    nine = ops.conv3x3(x, w, bias, up=True, up_size=(2 * h, 2 * w_))
    sub = ops.conv3x3_up_subpix(x, ops.upconv_fold(w), bias)
    ref = (resize_conv64(x.cpu(), w.cpu(), (2 * h, 2 * w_)) + bias.cpu().double()).float()
    tol = 1.0 if dtype == torch.bfloat16 else 0.25
    check(nine, ref, 3e-2 * tol, 1e-2 * tol, f"nine-tap up conv, exact target, vs fp32 {IDS[DTYPES.index(dtype)]}")
    check(sub, ref, 3e-2 * tol, 1e-2 * tol, f"sub-pixel form vs fp32 {IDS[DTYPES.index(dtype)]}")
    check(nine, sub.float(), 3e-2 * tol, 1e-2 * tol, f"nine-tap up conv vs the sub-pixel form {IDS[DTYPES.index(dtype)]}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ch", [64, 320])
@pytest.mark.parametrize("src", [(13, 10), (9, 11), (7, 5)], ids=lambda s: "x".join(map(str, s)))
def test_stride_2_conv_on_an_odd_input(src, ch, dtype):
    """Downsample2D: 13x10 -> 7x5, 9x11 -> 5x6, 7x5 -> 4x3 (the last output row / column reads one row of padding)."""
    h, w_ = src
    ho, wo = (h - 1) // 2 + 1, (w_ - 1) // 2 + 1
    x = rnd(2, h, w_, ch, seed=4).to(dtype)
    w = rnd(ch, 9 * ch, seed=5, scale=(9 * ch) ** -0.5).to(dtype).contiguous()
    bias = rnd(ch, seed=6)
    ref = resize_conv64(x, w, None, stride=2) + bias.double()
    A = resize_conv64(x.abs(), w.abs(), None, stride=2) + bias.double().abs()
    for splitk in (0, 1):
        out = ops.conv3x3(x.to(DEV), w.to(DEV), bias.to(DEV), stride=2, splitk=splitk)
        assert out.shape == (2, ho, wo, ch)
        derived(out, ref, A, 9 * ch, splitk or 8, f"stride-2 conv {h}x{w_} -> {ho}x{wo} C {ch} {IDS[DTYPES.index(dtype)]} splitk {splitk}")


# ------------------------------------------------------------------------------------------------ 2. the audit
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fuse", [False, True], ids=["combine-launch", "combine-in-kernel"])
def test_split_k_combines_at_the_small_odd_levels(fuse, dtype):
    """4x3 and 2x2 images of 640 channels at batch 2: 24 and 8 rows of a K = 5760 contraction, the weight streams the plans
    split.  Forced 4-way, with the separate combine launch and the in-kernel one, and the automatic choice."""
    ch = 640
    for (h, w_) in ((4, 3), (2, 2)):
        x = rnd(2, h, w_, ch, seed=7).to(dtype)
        w = rnd(ch, 9 * ch, seed=8, scale=(9 * ch) ** -0.5).to(dtype).contiguous()
        bias, res = rnd(ch, seed=9), rnd(2, h, w_, ch, seed=10).to(dtype)
        ref = resize_conv64(x, w, None) + bias.double() + res.double()
        A = resize_conv64(x.abs(), w.abs(), None) + bias.double().abs() + res.double().abs()
        for splitk in (4, 0):
            out = ops.conv3x3(x.to(DEV), w.to(DEV), bias.to(DEV), res1=res.to(DEV), splitk=splitk, fuse_combine=fuse)
            derived(out, ref, A, 9 * ch, splitk or 8,
                    f"split-K conv {h}x{w_} C {ch} {IDS[DTYPES.index(dtype)]} splitk {splitk} fused {fuse}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H,W", [(13, 10), (9, 11)])
def test_conv_out_fused_and_unfused(H, W, dtype):
    """pp_gn_conv3x3_smallcout (8x8 output patches: 2x2 patches with ragged right and bottom ones) and the pair it replaces,
    pp_groupnorm_apply_acc + pp_conv3x3_smallcout, at C = 320 -- the checks of test_fused_groupnorm_silu_conv_out."""
    B, Cc, groups = 2, 320, 32
    x = (rnd(B, H, W, Cc, seed=1, scale=2.0) + 0.5).to(dtype).to(DEV)
    xf = x.float().reshape(B, H * W, groups, Cc // groups)
    acc = torch.stack([(xf.sum((1, 3)).double() * 2 ** 24).round().long(),
                       ((xf * xf).sum((1, 3)).double() * 2 ** 20).round().long()], -1).contiguous()
    g, b = (rnd(Cc, seed=2) * 0.3 + 1.0).to(DEV), (rnd(Cc, seed=3) * 0.2).to(DEV)
    w = rnd(4, 9 * Cc, seed=4, scale=(9 * Cc) ** -0.5).to(dtype).contiguous().to(DEV)
    bias = rnd(4, seed=5).to(DEV)
    out = ops.gn_conv3x3_smallcout(x, acc, g, b, 1e-5, w, bias)
    y = ops.groupnorm_apply_acc(x, acc, g, b, 1e-5, True)
    old = ops.conv3x3_smallcout(y, w, bias)
    tol = 1.0 if dtype == torch.bfloat16 else 0.25
    tag = f"{H}x{W} {IDS[DTYPES.index(dtype)]}"
    check(out, old, 2e-4, 1e-4, f"fused conv_out vs groupnorm_apply_acc + conv3x3_smallcout {tag}")
    yn = F.silu(F.group_norm(x.float().permute(0, 3, 1, 2), groups, g, b, 1e-5))
    ref = F.conv2d(yn, w.float().reshape(4, 3, 3, Cc).permute(0, 3, 1, 2), bias, padding=1)
    check(out, ref, 3e-2 * tol, 1e-2 * tol, f"fused conv_out vs fp32 {tag}")
    check(old, ref, 3e-2 * tol, 1e-2 * tol, f"unfused conv_out vs fp32 {tag}")
    ref2 = F.conv2d(y.float().permute(0, 3, 1, 2), w.float().reshape(4, 3, 3, Cc).permute(0, 3, 1, 2), bias, padding=1)
    check(old, ref2, 1e-3, 1e-3, f"conv3x3_smallcout alone {tag}")         # (the gate of test_conv_smallcout)


@pytest.mark.parametrize("C1,C2,H,W", [(320, 0, 13, 10), (320, 320, 7, 5), (640, 320, 4, 3), (640, 640, 2, 2), (320, 0, 9, 11)])
@pytest.mark.parametrize("silu", [True, False])
def test_groupnorm_stats_and_apply(C1, C2, H, W, silu):
    """pp_groupnorm_stats + pp_groupnorm_apply (hw = 130, 35, 12, 4, 99: chunks of hw / 16 pixels with a remainder, fewer
    pixels than one chunk) under the derived gate of tests/norm_cases.py, as test_groupnorm."""
    B, Cc = 2, C1 + C2
    x1 = (rnd(B, H, W, C1, seed=1) * 2 + 0.5).bfloat16().to(DEV)
    x2 = rnd(B, H, W, C2, seed=2).bfloat16().to(DEV) if C2 else None
    g, b = rnd(Cc, seed=3).to(DEV), rnd(Cc, seed=4).to(DEV)
    eps = 1e-5 if silu else 1e-6
    out = ops.groupnorm(x1, g, b, eps, silu, x2=x2)
    f = lambda t: t.reshape(B, H * W, -1) if t is not None else None      # noqa: E731
    ref, gate = NC.gate_groupnorm(f(x1), f(x2), 32, g, b, eps, silu, torch.bfloat16, NC.stats_eps(H * W, Cc, 32))
    r = NC.worst_ratio(out.reshape(B, H * W, Cc), ref, gate)
    record(f"[any size] groupnorm {C1}+{C2} {H}x{W} silu {silu}: error / derived gate {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("cin,cout,stride,H,W", [(9, 320, 1, 13, 10), (16, 32, 2, 13, 10), (32, 96, 2, 9, 11), (8, 8, 1, 13, 10)])
def test_conv_direct_on_odd_images(cin, cout, stride, H, W):
    """pp_conv3x3_direct: conv_in's shape, the stride-2 convs of the conditioning embedding on an ODD input (the plans only
    meet even ones there: 8x the latent), the VAE's 8-channel convs at a 13x10 latent.  The gate of test_conv_direct."""
    B = 2
    x = rnd(B, H, W, cin, seed=1).bfloat16().to(DEV)
    w = rnd(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5).bfloat16().to(DEV)
    b = rnd(cout, seed=3).to(DEV)
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    add = rnd(B, ho, wo, cout, seed=4).bfloat16().to(DEV)
    out = ops.conv3x3_direct(x, w.permute(2, 3, 1, 0).contiguous(), b, stride, True, add)
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.float(), b, stride=stride, padding=1).permute(0, 2, 3, 1)
    assert out.shape == (B, ho, wo, cout)
    check(out, F.silu(ref + add.float()), 2e-2, 1e-2, f"conv direct {cin}->{cout} s{stride} {H}x{W}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("hw", [130, 99])
def test_step_head_and_layout_kernels(hw, dtype):
    """pp_step_head at hw = 130 / 99 is the three launches it replaces, bit for bit (test_step_head_is_the_three_launches_it_
    replaces); pp_step_head_scaled on divided latents; pp_nchw_to_nhwc / pp_nhwc_to_nchw round trips."""
    B, Cc, ldc, rows, steps = 2, 4, 64, 1280, 5
    table, lat = rnd(steps, rows, seed=1).to(DEV), rnd(B, Cc, hw, seed=2).to(DEV)
    step = torch.tensor([3], dtype=torch.int32, device=DEV)
    temb = torch.full((rows,), -1.0, device=DEV)
    x = torch.full((2 * B, hw, ldc), 3.0, device=DEV).to(dtype)
    acc = torch.full((37,), 7, dtype=torch.int64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    L.check(L.lib().pp_step_head(table.data_ptr(), step.data_ptr(), temb.data_ptr(), rows, lat.data_ptr(), 2 * B, Cc, hw, B,
                                 x.data_ptr(), ldc, 0, L.dtype_code(dtype), acc.data_ptr(), acc.numel(), st), "pp_step_head")
    ref = torch.cat([lat, lat]).permute(0, 2, 1).to(dtype)
    assert torch.equal(temb, table[3]) and int(acc.abs().sum()) == 0
    assert torch.equal(x[:, :, :Cc], ref) and bool((x[:, :, Cc:] == 3.0).all())
    div = (torch.rand(steps, generator=torch.Generator("cpu").manual_seed(3)) * 14 + 1).to(DEV)      # (one divisor per step)
    x2 = torch.full_like(x, 3.0)
    L.check(L.lib().pp_step_head_scaled(table.data_ptr(), step.data_ptr(), temb.data_ptr(), rows, lat.data_ptr(), 2 * B, Cc, hw,
                                        B, x2.data_ptr(), ldc, 0, L.dtype_code(dtype), acc.data_ptr(), acc.numel(),
                                        div.data_ptr(), st), "pp_step_head_scaled")
    assert torch.equal(x2[:, :, :Cc], (torch.cat([lat, lat]).cpu() / div[3].cpu()).permute(0, 2, 1).to(dtype).to(DEV))
    y = ops.nchw_to_nhwc(lat.reshape(B, Cc, hw, 1), batch=2 * B, ldc=9, c0=0) if dtype == torch.bfloat16 else None
    if y is not None:
        assert torch.equal(y[:B, :, :, :Cc], lat.reshape(B, Cc, hw, 1).permute(0, 2, 3, 1).bfloat16())
        assert torch.equal(y[B:], y[:B]) and torch.count_nonzero(y[..., Cc:]) == 0
    z = rnd(B, 13 if hw == 130 else 9, 10 if hw == 130 else 11, 320, seed=5).to(dtype).to(DEV)
    assert torch.equal(ops.nhwc_to_nchw(z), z.float().permute(0, 3, 1, 2))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d,n", [(40, 130), (40, 99), (40, 120), (80, 35), (80, 30), (80, 12), (80, 9), (80, 4)])
def test_self_attention_at_odd_token_counts(d, n, dtype):
    """nq = nk = H W of the levels of 13x10, 9x11 and 10x12: V^T rows padded to 8 by pp_transpose_v where n % 8 != 0 (the
    plans' unfused route), the gates of test_attention and test_attention_fp16."""
    B, Hh = 2, 8
    Cc = Hh * d
    q, k, v = (rnd(B * n, Cc, seed=s).to(dtype).to(DEV) for s in (1, 2, 3))
    vt = ops.transpose_v(v, B, n)
    ldvt = vt.shape[-1]
    assert ldvt == (n + 7) // 8 * 8 and torch.count_nonzero(vt[..., n:]) == 0
    assert torch.equal(vt[..., :n].reshape(B, Cc, n), v.view(B, n, Cc).transpose(1, 2))
    out = ops.attention(q, k, vt, B, Hh, n, n, d)
    sh = lambda t: t.float().view(B, n, Hh, d).transpose(1, 2)      # noqa: E731
    ref = F.scaled_dot_product_attention(sh(q), sh(k), sh(v)).transpose(1, 2).reshape(B * n, Cc)
    atol, rtol = (2e-2, 2e-2) if dtype == torch.bfloat16 else (5e-3, 2.5e-3)      # (test_attention / test_attention_fp16)
    check(out, ref, atol, rtol, f"self-attention d {d} n {n} {IDS[DTYPES.index(dtype)]}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 4, 3, 640, 640), (2, 2, 2, 640, 640), (2, 5, 6, 320, 640), (1, 3, 3, 640, 320)],
                         ids=lambda s: "x".join(map(str, s)))
def test_pp_freeu_at_the_odd_levels(shape, dtype):
    """pp_freeu at the up-block levels of 13x10 (2x2, 4x3) and 9x11 (3x3, 5x6) against the torch.fft restatement under the gate
    of test_pp_freeu_against_the_restatement."""
    B, H, W, Ch, Cs = shape
    b, s = 1.5, 0.2
    hid, skip = (t.to(DEV) for t in FC.op_inputs(shape, dtype))
    acc = torch.zeros(B, 32, 2, dtype=torch.int64, device=DEV)
    ho, so = ops.freeu(hid, skip, b, s, acc=acc, groups=32)
    ref_s = FC.fourier_filter(skip.float().permute(0, 3, 1, 2), threshold=1, scale=s).permute(0, 2, 3, 1)
    assert torch.equal(ho[..., Ch // 2:], hid[..., Ch // 2:])
    assert torch.equal(ho[..., :Ch // 2], (hid.float()[..., :Ch // 2] * b).to(dtype))
    err = (so.float() - ref_s).abs()
    tol = FC.ulp16(ref_s, dtype) + 1e-5 * float(skip.float().abs().max())
    record(f"[any size] pp_freeu {shape} {IDS[DTYPES.index(dtype)]}: skip max err {float(err.max()):.4g}, worst err / tol "
           f"{float((err / tol).max()):.3f}")
    assert (err <= tol).all()
    cat = torch.cat([ho, so], -1).double().reshape(B, H * W, 32, (Ch + Cs) // 32)
    want = torch.stack([cat.sum((1, 3)), (cat ** 2).sum((1, 3))], -1)
    got = torch.stack([acc[..., 0].double() / 2 ** 24, acc[..., 1].double() / 2 ** 20], -1)
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-2)


# ------------------------------------------------------------------------------------------------ 3. the networks
@functools.lru_cache(maxsize=None)
def gold():
    return torch.load(os.path.join(HERE, "golden", "ref_any_size.pt"), weights_only=False)


@functools.lru_cache(maxsize=None)
def state_dicts():
    import make_ref_any_size as M
    import make_ref_wiring as MW
    u9, u4 = MW.oracle_models()
    return u9.state_dict(), u4.state_dict(), M.brushnet_of(u4).state_dict(), M.controlnet().state_dict()


def net_gate(out, ref, what, dtype, residual=False):
    """tests/test_models_gpu.py::close for bf16 (cosine >= 0.999, 0.998 for a side network's residual; max-abs <= 3e-2
    max(1, max|ref|)); tests/test_fp16_gpu.py for fp16 (0.99999, residuals 0.9999; 7.5e-3)."""
    out, ref = out.float().cpu(), ref.float().cpu()
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    cos_min, rel = ((0.998 if residual else 0.999), 3e-2) if dtype == torch.bfloat16 else ((0.9999 if residual else 0.99999), 7.5e-3)
    cos = F.cosine_similarity(out.flatten(), ref.flatten(), dim=0).item()
    err = (out - ref).abs().max().item()
    bound = rel * max(1.0, ref.abs().max().item())
    record(f"[any size] {what}: cosine {cos:.7f} (gate {cos_min})  max-abs {err:.4g} (gate {bound:.4g})  max|ref| {float(ref.abs().max()):.4g}")
    assert torch.isfinite(out).all() and cos >= cos_min and err <= bound, (what, cos, err)


def summary_gate(t, want, what, dtype):
    """A residual against its stored summary (mean, std, max-abs, first 32 values): the first 32 values under the network gate
    scaled by the tensor's max-abs, the three moments within 3e-2 (7.5e-3 in fp16) of max(1, max-abs)."""
    t = t.float().cpu().flatten()
    rel = 3e-2 if dtype == torch.bfloat16 else 7.5e-3
    scale = max(1.0, float(want[2]))
    got = torch.cat([torch.stack([t.mean(), t.std(), t.abs().max()]), t[:32]])
    err = float((got - want).abs().max())
    record(f"[any size] {what}: summary max err {err:.4g} (gate {rel * scale:.4g}), max|ref| {float(want[2]):.4g}")
    assert torch.isfinite(t).all() and err <= rel * scale, (what, err)


def _hip(kind, dtype):
    import make_ref_any_size as M
    sd9, sd4, sdb, sdc = state_dicts()
    if kind == "u9":
        return PM.UNet2DConditionModel(in_channels=9, device=DEV, dtype=dtype, **M.CFG).load_state_dict(sd9)
    if kind == "u4":
        return PM.UNet2DConditionModel(in_channels=4, device=DEV, dtype=dtype, **M.CFG).load_state_dict(sd4)
    if kind == "bn":
        return PM.BrushNetModel(in_channels=4, conditioning_channels=5, device=DEV, dtype=dtype, **M.CFG).load_state_dict(sdb)
    return PM.ControlNetModel(in_channels=4, device=DEV, dtype=dtype, **M.CN_HIP_CFG).load_state_dict(sdc)


def _replay(rt, out_fn):
    """The step once more as a captured graph: bit-equal to what the eager run left."""
    eager = [t.clone() for t in out_fn()]
    rt.run_step(use_graph=True)
    assert rt.graph is not None
    graph = [t.clone() for t in out_fn()]
    assert all(torch.equal(a, b) for a, b in zip(eager, graph)), "graph replay differs from the eager step"
    rt.run_step(use_graph=True)
    assert all(torch.equal(a, b) for a, b in zip(graph, out_fn()))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_networks_against_the_reference(hw, dtype):
    """(a) the 9- and the 4-channel UNet; (b) BrushNet: every residual, then epsilon of the UNet fed with them (zero-copy);
    (d) ControlNet: every residual, then epsilon.  Each step eager and as a replayed graph, bit-equal."""
    import make_ref_any_size as M
    G, inp = gold()["nets"][M.key(hw)], M.net_inputs(hw)
    tag = f"{M.key(hw)} {IDS[DTYPES.index(dtype)]}"
    dev = lambda t: t.to(DEV)      # noqa: E731
    u9, u4, bn, cn = (_hip(k, dtype) for k in ("u9", "u4", "bn", "cn"))
    # (a)
    out = u9(dev(inp["x9"]), inp["t"], dev(inp["ehs"]), return_dict=False)[0]
    net_gate(out, G["eps9"], f"9-channel UNet {tag}", dtype)
    _replay(u9.rt, lambda: [u9.rt.eps_tensor()])
    out = u4(dev(inp["x4"]), inp["t"], dev(inp["ehs"]), return_dict=False)[0]
    net_gate(out, G["eps4_plain"], f"4-channel UNet {tag}", dtype)
    # (b)
    dn, md, up = bn(dev(inp["x4"]), inp["t"], dev(inp["ehs_b"]), dev(inp["cond"]), conditioning_scale=inp["scale"],
                    return_dict=False)
    res = list(dn) + [md] + list(up)
    assert [tuple(t.shape) for t in res] == [tuple(s) for s in G["res_shapes"]]
    for i, t in enumerate(res):
        summary_gate(t, G["res_summary"][i], f"BrushNet residual {i} {tuple(t.shape)} {tag}", dtype)
    _replay(bn.rt, lambda: [t for t in bn.outputs()[0]] + [bn.outputs()[1]] + [t for t in bn.outputs()[2]])
    out = u4(dev(inp["x4"]), inp["t"], dev(inp["ehs"]), down_block_add_samples=list(dn), mid_block_add_sample=md,
             up_block_add_samples=list(up), return_dict=False)[0]
    net_gate(out, G["eps4_brush"], f"UNet + BrushNet residuals {tag}", dtype)
    _replay(u4.rt, lambda: [u4.rt.eps_tensor()])
    # (d)
    cd, cm = cn(dev(inp["x9"][:, :4]), inp["t"], dev(inp["ehs"]), dev(inp["ctrl"]), conditioning_scale=inp["cn_scale"],
                return_dict=False)
    assert [tuple(t.shape) for t in list(cd) + [cm]] == [tuple(s) for s in G["ctrl_shapes"]]
    for i, t in enumerate(list(cd) + [cm]):
        summary_gate(t, G["ctrl_summary"][i], f"ControlNet residual {i} {tuple(t.shape)} {tag}", dtype)
    out = u9(dev(inp["x9"]), inp["t"], dev(inp["ehs"]), down_block_additional_residuals=cd, mid_block_additional_residual=cm,
             return_dict=False)[0]
    net_gate(out, G["eps9_ctrl"], f"UNet + ControlNet residuals {tag}", dtype)
    _replay(u9.rt, lambda: [u9.rt.eps_tensor()])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_padding_the_latent_is_a_different_function(dtype):
    """Not an implementation of these sizes: the 13x10 latent zero-padded to 16x16, run, cropped.  It misses the gate the real thing
    passes by an order of magnitude -- the fixture tells the two apart."""
    import make_ref_any_size as M
    G, inp = gold()["nets"]["13x10"], M.net_inputs((13, 10))
    u9 = _hip("u9", dtype)
    xp = F.pad(inp["x9"], (0, 6, 0, 3))
    out = u9(xp.to(DEV), inp["t"], inp["ehs"].to(DEV), return_dict=False)[0][:, :, :13, :10].float().cpu()
    err = float((out - G["eps9"]).abs().max())
    record(f"[any size] pad to 16x16 and crop, 9-channel UNet {IDS[DTYPES.index(dtype)]}: max-abs {err:.4g} on max|ref| "
           f"{float(G['eps9'].abs().max()):.4g} (gate 3e-2)")
    assert err > 10 * 3e-2 * max(1.0, float(G["eps9"].abs().max()))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_freeu_at_13x10(dtype):
    """Up block 0 filters 2x2 skips, up block 1 4x3 ones.  Against the reference UNet whose up blocks call the restated filter of
    tests/freeu_cases.py, under that module's gate; the plain output misses it (asserted when the fixture was made, and here)."""
    import make_ref_any_size as M
    G, inp = gold()["nets"]["13x10"], M.net_inputs((13, 10))
    u9 = _hip("u9", dtype)
    run = lambda: u9(inp["x9"].to(DEV), inp["t"], inp["ehs"].to(DEV), return_dict=False)[0].clone()      # noqa: E731
    before = run()
    u9.enable_freeu(**FC.FREEU_FULL)
    out = run()
    assert [c[2] for c in u9.rt.step_plan.calls].count("freeu") == 4
    cos, err, ok = FC.close_gate(out, G["eps9_freeu"])
    record(f"[any size] 9-channel UNet with FreeU 13x10 {IDS[DTYPES.index(dtype)]}: cosine {cos:.6f}  max-abs {err:.4g}  "
           f"(max|ref| {float(G['eps9_freeu'].abs().max()):.4g})")
    assert ok and not FC.close_gate(before, G["eps9_freeu"])[2]
    _replay(u9.rt, lambda: [u9.rt.eps_tensor()])
    u9.disable_freeu()
    assert torch.equal(run(), before)


# ------------------------------------------------------------------------------------------------ 4. the pipelines
def _close_latents(out, want, what, cos_min=0.9997, rel=4.5e-2):
    """The free-running gate of the loop tests (tests/test_golden.py::_close_latents)."""
    cos = F.cosine_similarity(out.float().cpu().flatten(), want.flatten(), dim=0).item()
    err = (out.float().cpu() - want).abs().max().item()
    bound = rel * max(1.0, want.abs().max().item())
    record(f"[any size] {what}: cosine {cos:.7f} (gate {cos_min})  max-abs {err:.4g} (gate {bound:.4g})  max|ref| {float(want.abs().max()):.4g}")
    assert cos >= cos_min and err <= bound, (what, cos, err)


@functools.lru_cache(maxsize=None)
def _text_vae():
    import make_ref_pipeline_call as MP
    tok, enc, _, vae = MP.components()
    hv = PM.AutoencoderKL(device=DEV, **MP.VAE_CFG).load_state_dict(vae.state_dict())
    he = PM.CLIPTextModel(device=DEV, vocab_size=enc.config.vocab_size, num_hidden_layers=1, eos_token_id=enc.config.eos_token_id)
    he.load_state_dict(enc.state_dict())
    return tok, he, hv


def _prefix_launches(model):
    """Launches of the CFG twin prefix in a network's step plan: the ones that store their output rows twice."""
    return [a for fn, args, name in model.rt.step_plan.calls
            for a in [getattr(args[0], "_obj", None) if args else None] if isinstance(a, L.PPGemmArgs) and a.out_dup_rows > 0]


@pytest.mark.parametrize("twin", [True, False], ids=["twin", "no-twin"])
@pytest.mark.parametrize("case", ["v1_ddim", "v1_dpm", "v2_ddim", "v2_dpm", "cn_ddim"])
def test_pipelines_against_the_reference_calls(case, twin, monkeypatch):
    """104x80 image, 13x10 latents, 4 steps, guidance 7.5, two images per prompt.  130 rows per item are no whole 128-row
    tiles: the plans decline the twin prefix (asserted), with it asked for (the product) and switched off."""
    import make_ref_any_size as M
    monkeypatch.setattr(ENG, "TWIN_PREFIX", twin)
    tok, he, hv = _text_vae()
    img, mask, lat, ctrl = M.call_inputs()
    g = torch.Generator().manual_seed(M.SEED)
    sch = M.scheduler(case, PS)
    if case.startswith("v1"):
        pipe = PP.StableDiffusionInpaintPipeline(vae=hv, text_encoder=he, tokenizer=tok, unet=_hip("u9", torch.bfloat16), scheduler=sch)
        out = pipe(image=img, mask=mask, latents=lat.to(DEV), generator=g, output_type="latent", return_dict=False,
                   **M.CALLS["v1"])[0]
    elif case.startswith("v2"):
        pipe = PP.StableDiffusionPowerPaintBrushNetPipeline(vae=hv, text_encoder=he, text_encoder_brushnet=he, tokenizer=tok,
                                                            unet=_hip("u4", torch.bfloat16), brushnet=_hip("bn", torch.bfloat16),
                                                            scheduler=sch)
        pre, mask3 = img * (mask < 0.5), (mask * 2 - 1).repeat(1, 3, 1, 1)
        dist = hv.encode(torch.cat([pre.repeat(M.NB, 1, 1, 1)] * 2).to(DEV)).latent_dist
        torch.manual_seed(9)
        noise = torch.randn(dist.mean.shape)                       # CPU global RNG, as in the reference run
        cl = (dist.mean + dist.std * noise.to(DEV)) * hv.config.scaling_factor
        keep = (torch.cat([mask3.repeat(M.NB, 1, 1, 1)] * 2).sum(1)[:, None] < 0).float()
        cond = torch.cat([cl, F.interpolate(keep, size=cl.shape[-2:]).to(DEV)], 1)
        assert cond.shape[-2:] == (13, 10)
        out = pipe(conditioning_latents=cond, latents=lat.to(DEV), generator=g, output_type="latent", return_dict=False,
                   **M.CALLS["v2"])[0]
        assert not _prefix_launches(pipe.brushnet)
    else:
        pipe = PP.StableDiffusionControlNetInpaintPipeline(vae=hv, text_encoder=he, tokenizer=tok, unet=_hip("u9", torch.bfloat16),
                                                           controlnet=_hip("cn", torch.bfloat16), scheduler=sch)
        out = pipe(image=img, mask=mask, control_image=ctrl, latents=lat.to(DEV), generator=g, output_type="latent",
                   return_dict=False, **M.CALLS["cn"])[0]
        assert not _prefix_launches(pipe.controlnet)
    assert tuple(out.shape) == (M.NB, 4, 13, 10)
    assert (pipe.unet.rt.H, pipe.unet.rt.W) == (13, 10) and not _prefix_launches(pipe.unet), "the plan took the twin prefix at 130 rows per item"
    assert not pipe.unet.net.twin_prefix_ok(L.lib(), 2 * M.NB, 13, 10, 77)
    _close_latents(out, gold()["calls"][case], f"{case} pipeline, 104x80, twin prefix {'asked for' if twin else 'off'}")


# ------------------------------------------------------------------------------------------------ 5. the VAE
SMALL_VAE = dict(block_out_channels=(64, 128, 256, 256), layers_per_block=1)


def _vae_close(got, want, what, cos_min=0.999, rel_max=0.05):
    """The gate of the VAE parity tests (tests/test_vae.py::_close)."""
    got, want = got.float().cpu().flatten(), want.float().cpu().flatten()
    cos = F.cosine_similarity(got, want, dim=0).item()
    rel = ((got - want).abs().max() / want.abs().max()).item()
    record(f"[any size] {what}: cosine {cos:.6f} (gate {cos_min})  max-abs / max|ref| {rel:.4f} (gate {rel_max})")
    assert cos >= cos_min and rel <= rel_max, (what, cos, rel)


def _oracle_vae(net, sd):
    o = OV.AutoencoderKL(**SMALL_VAE).eval()
    o.load_state_dict({k: v.float() for k, v in sd.items()})
    with torch.no_grad():
        for p in o.parameters():
            if p.dim() >= 2:
                p.copy_(p.to(torch.bfloat16).float())
    return o


def _poison_attention_buffers(rt):
    """NaN into everything the mid-block attention keeps in the arena between launches -- K with its pad rows, V^T, S, P:
    whatever the plan relies on it must write."""
    calls = rt.plan.calls
    tv = [c[1] for c in calls if c[2] == "transpose_v"][0]
    sm = [c[1] for c in calls if c[2] == "softmax_rows"][0]
    qk = [c[1][0]._obj for c in calls if c[2] == "attn_qk"]
    (B, n, Cc, vt, npad), (s, p) = (tv[2], tv[3], tv[4], tv[5], tv[6]), (sm[0], sm[5])
    nan = float("nan")
    rt.arena.view(vt, (B * Cc * npad,), torch.bfloat16).fill_(nan)
    rt.arena.view(s, (n * npad,), torch.float32).fill_(nan)
    rt.arena.view(p, (n * npad,), torch.bfloat16).fill_(nan)
    rt.arena.view(qk[0].w, ((B * n + npad - n) * Cc,), torch.bfloat16).fill_(nan)
    return rt.arena.view(p, (n, npad), torch.bfloat16), n, npad


@pytest.mark.parametrize("H,W", [(104, 80), (72, 88)])
def test_vae_at_token_counts_off_the_grid(H, W):
    """n = 130 and n = 99 tokens in the mid-block attention (padded to 192 and 128 keys), batch 2, against oracle/vae.py under
    the gate of the existing parity tests; then once more on poisoned attention buffers: the same bits, and exact zeros in
    the pad columns of P."""
    vae = PM.AutoencoderKL(device=DEV, **SMALL_VAE)
    sd = vae.net.synthetic_state_dict(seed=11)
    vae.load_state_dict(sd)
    o = _oracle_vae(vae.net, sd)
    g = torch.Generator().manual_seed(5)
    z = torch.randn(2, 4, H // 8, W // 8, generator=g) * 3.0
    img = torch.rand(2, 3, H, W, generator=g) * 2 - 1
    with torch.no_grad():
        want_d = o.decode(z.to(torch.bfloat16).float(), return_dict=False)[0]
        want_e = o.moments(img.to(torch.bfloat16).float())
    got_d = vae.decode(z.to(DEV), return_dict=False)[0].clone()
    assert got_d.shape == (2, 3, H, W)
    _vae_close(got_d, want_d, f"VAE decode {H}x{W} ({H * W // 64} tokens)")
    dist = vae.encode(img.to(DEV)).latent_dist
    got_e = torch.cat([dist.mean, dist.logvar], 1).clone()
    _vae_close(got_e, torch.cat([want_e[:, :4], want_e[:, 4:].clamp(-30, 20)], 1), f"VAE encode {H}x{W} ({H * W // 64} tokens)")
    for rt, run, before in ((vae._dec, lambda: vae.decode(z.to(DEV), return_dict=False)[0], got_d),
                            (vae._enc, lambda: torch.cat([(d := vae.encode(img.to(DEV)).latent_dist).mean, d.logvar], 1), got_e)):
        P, n, npad = _poison_attention_buffers(rt)
        assert (n, npad) == (H * W // 64, (H * W // 64 + 63) // 64 * 64) and npad > n
        again = run()
        torch.cuda.synchronize()
        assert torch.equal(again, before), f"{rt.direction}: the result depends on what the arena held"
        # P is scratch the layers behind the attention reuse: poison again and stop the plan behind its last softmax (the input
        # buffer still holds the image)
        P, n, npad = _poison_attention_buffers(rt)
        last = max(i for i, c in enumerate(rt.plan.calls) if c[2] == "softmax_rows")
        for fn, args, name in rt.plan.calls[:last + 1]:
            L.check(fn(*args, torch.cuda.current_stream().cuda_stream), name)
        torch.cuda.synchronize()
        assert torch.count_nonzero(P[:, n:]) == 0 and not torch.isnan(P.float()).any(), "pad columns of P are not exact zeros"
        assert torch.allclose(P[:, :n].float().sum(1), torch.ones(n, device=DEV), atol=2e-2)


def test_softmax_rows_writes_its_pad_columns():
    """pp_softmax_rows (ABI v29): columns [n, ldp) of P are written as zeros over whatever was there; ldp = n writes nothing
    more (the call of the sizes accepted before)."""
    rows, n, npad = 37, 130, 192
    s = torch.randn(rows, npad, device=DEV) * 30
    s[:, n:] = float("nan")
    p = torch.full((rows + 1, npad), float("nan"), dtype=torch.bfloat16, device=DEV)
    L.check(L.lib().pp_softmax_rows(s.data_ptr(), npad, rows, n, 0.3, p.data_ptr(), npad, L.PP_DT_BF16,
                                    torch.cuda.current_stream().cuda_stream), "pp_softmax_rows")
    want = torch.softmax(s[:, :n].double() * 0.3, dim=-1)
    assert torch.allclose(p[:rows, :n].double(), want, atol=2e-3, rtol=2 ** -7)
    assert torch.count_nonzero(p[:rows, n:]) == 0 and torch.isnan(p[rows].float()).all()      # (the row behind: untouched)


# ------------------------------------------------------------------------------------------------ 6. the controller
def test_controller_with_a_4_to_3_photo():
    """A 4:3 PIL image and mask through PowerPaintController.predict, text-guided, reduced nets, 2 steps: fit_short_side +
    snap_to_eight make it 848x640 (106x80 latents: 106 % 8 = 2, refused before; the upsampler 27 -> 53 is cropped).  Pixel-identical to the same request driven through
    the pipeline by hand (the pattern of tests/test_controller.py)."""
    from test_controller import make_inputs
    from powerpaint_amd.controller import PowerPaintController, _set_seed, add_task, fit_short_side, snap_to_eight
    tok, he, hv = _text_vae()
    import make_ref_any_size as M
    hu = PM.UNet2DConditionModel(in_channels=9, device=DEV, **M.CFG)        # four levels: 106 -> 53 -> 27 -> 14
    hu.load_state_dict(hu.net.synthetic_state_dict(seed=3))
    pipe = PP.StableDiffusionInpaintPipeline(vae=hv, text_encoder=he, tokenizer=tok, unet=hu, scheduler=PS.DDIMScheduler())
    ctl = PowerPaintController(pipe, version="ppt-v1")
    inp = make_inputs(160, 120, seed=7)
    keep = {"image": inp["image"].copy(), "mask": inp["mask"].copy()}
    out, res = ctl.predict(inp, "a red cat", 0.7, 2, 6.5, 123, "blurry", "text-guided")
    assert len(out) == 1 and out[0].size == (848, 640) and out[0].mode == "RGB" and len(res) == 2
    assert (pipe.unet.rt.H, pipe.unet.rt.W) == (80, 106) and np.array(out[0]).std() > 1.0
    image = fit_short_side(keep["image"], False)
    image, mask, (w, h) = snap_to_eight(image, keep["mask"])
    assert (w, h) == (848, 640)
    pA, pB, nA, nB = add_task("a red cat", "blurry", "text-guided", "ppt-v1")
    _set_seed(123)
    again = pipe(promptA=pA, promptB=pB, tradoff=0.7, tradoff_nag=0.7, negative_promptA=nA, negative_promptB=nB,
                 image=image.convert("RGB"), mask=mask.convert("RGB"), width=w, height=h, guidance_scale=6.5,
                 num_inference_steps=2).images[0]
    assert np.array_equal(np.array(out[0]), np.array(again))
