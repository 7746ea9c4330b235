"""GPU: the kernels AsymmetricAutoencoderKL adds (csrc/asym_vae.hip), probed exactly.

pp_conv4x4s2 -- small-integer activations and weights (|x| <= 3, |w| <= 2, K = 16 Cin <= 2048 terms: every partial sum is an
integer below 2^24, exact in the fp32 accumulator in ANY summation order), bias in halves: the kernel must reproduce float64
`F.conv2d(stride=2, padding=1)`, rounded once to the 16-bit format, bit for bit.  Outputs sit inside poisoned guard bands.

pp_mask_blend -- out = fma(s, m, c * (1 - m)) in fp32, three roundings (1 - m, c * (1 - m), the fma), each a relative error of
at most u = 2^-24, so against the float64 value e of s m + c (1 - m)
        |r32 - e| <= ((1 + u)^3 - 1) (|s m| + |c (1 - m)|) =: E32,
and the stored value, r32 rounded to nearest in the 16-bit format (unit roundoff u16 = 2^-8 bf16, 2^-11 fp16; fp16 subnormal
spacing 2^-24), satisfies |stored - e| <= E32 + u16 (|e| + E32) + 2^-25.  The accumulators are compared with float64 sums of the
STORED values: a thread adds the 8 values of a channel it owns in fp32 (error <= 7 u sum|v|, the squares v^2 themselves are
exact: 16 or 22 significant bits) and converts to fixed point (error <= 2^-25 resp. 2^-21 per partial); the rest is integer.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
POISON = 0x7B5A          # a 16-bit pattern no probe produces (bf16 2.8e36 / fp16 60224)


def _lib():
    from powerpaint_amd import _lib as L
    return L, L.lib()


def _guarded(n_elems, guard=4096):
    """int16 buffer [guard | n_elems | guard] filled with the poison; returns (buffer, pointer of the payload)."""
    buf = torch.full((n_elems + 2 * guard,), POISON, dtype=torch.int16, device="cuda")
    return buf, buf.data_ptr() + 2 * guard, guard


CONV_CASES = [
    # B, Cin, Cout, H, W, relu_in
    (1, 64, 64, 8, 8, False),
    (1, 64, 64, 24, 40, True),          # non-square, output 12 x 20
    (3, 128, 256, 24, 40, True),        # 720 output rows: no multiple of the 128-row tile; two column tiles
    (1, 64, 192, 8, 8, False),          # out channels: one and a half column tiles
    (2, 64, 64, 9, 13, True),           # odd sides: the last window hangs over the right / bottom edge by the padding only
]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("B,Cin,Cout,H,W,relu", CONV_CASES)
def test_conv4x4s2_is_exact_on_integer_probes(dt, B, Cin, Cout, H, W, relu):
    L, lib = _lib()
    from powerpaint_amd.vae_asym import conv4x4_igemm
    dtype = DT[dt]
    g = torch.Generator().manual_seed(B * 1000 + Cin + Cout + H)
    x = torch.randint(-3, 4, (B, Cin, H, W), generator=g).double()
    w = torch.randint(-2, 3, (Cout, Cin, 4, 4), generator=g).double()
    bias = torch.randint(-8, 9, (Cout,), generator=g).double() / 2
    want = F.conv2d(F.relu(x) if relu else x, w, bias, stride=2, padding=1)            # float64: exact
    assert want.abs().max() < 2 ** 24
    want16 = want.permute(0, 2, 3, 1).contiguous().to(dtype)                            # one rounding
    Ho, Wo = want.shape[-2:]
    assert (Ho, Wo) == ((H - 2) // 2 + 1, (W - 2) // 2 + 1)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()
    wd = conv4x4_igemm(w).contiguous().to(dtype).cuda()
    bd = bias.float().cuda()
    buf, out_ptr, guard = _guarded(B * Ho * Wo * Cout)
    L.check(lib.pp_conv4x4s2(xd.data_ptr(), B, H, W, Cin, wd.data_ptr(), bd.data_ptr(), Cout, int(relu), out_ptr,
                             L.dtype_code(dtype), torch.cuda.current_stream().cuda_stream), "pp_conv4x4s2")
    torch.cuda.synchronize()
    got = buf[guard:-guard].view(dtype).view(B, Ho, Wo, Cout).cpu()
    assert torch.equal(got.view(torch.int16), want16.view(torch.int16)), \
        f"{(got.double() - want16.double()).abs().max().item()} off at most"
    assert bool((buf[:guard] == POISON).all()) and bool((buf[-guard:] == POISON).all()), "guard band written"
    if relu:                                                                            # the operand itself is not rewritten
        assert torch.equal(xd.cpu(), x.permute(0, 2, 3, 1).contiguous().to(dtype))


def test_conv4x4s2_refuses_what_it_cannot_run():
    L, lib = _lib()
    x = torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(64, 16 * 64, dtype=torch.bfloat16, device="cuda")
    o = torch.zeros(1, 4, 4, 64, dtype=torch.bfloat16, device="cuda")
    args = lambda cin, cout, dt: (x.data_ptr(), 1, 8, 8, cin, w.data_ptr(), None, cout, 0, o.data_ptr(), dt, None)   # noqa: E731
    assert lib.pp_conv4x4s2(*args(48, 64, 1)) == -1 and lib.pp_conv4x4s2(*args(64, 62, 1)) == -1
    assert lib.pp_conv4x4s2(*args(64, 64, 0)) == -1
    assert lib.pp_conv4x4s2(None, 1, 8, 8, 64, w.data_ptr(), None, 64, 0, o.data_ptr(), 1, None) == -1


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_relu_and_masked_image_pack(dt):
    L, lib = _lib()
    dtype = DT[dt]
    code = L.dtype_code(dtype)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5 * 7 * 64, generator=g).to(dtype)
    x[:4] = torch.tensor([0.0, -0.0, float("inf"), float("-inf")]).to(dtype)
    buf, ptr, guard = _guarded(x.numel())
    xd = x.cuda()
    L.check(lib.pp_relu(xd.data_ptr(), ptr, x.numel(), code, st), "pp_relu")
    got = buf[guard:-guard].view(dtype).cpu()
    assert torch.equal(got.float(), F.relu(x.float()))                  # max(x, 0) value for value, infinities included
    assert got.view(torch.int16)[:4].tolist() == [0, 0, x.view(torch.int16)[2].item(), 0]      # -0 -> +0 (include/pp_hip.h)
    assert bool((buf[:guard] == POISON).all()) and bool((buf[-guard:] == POISON).all())
    # (1 - mask) * image, fp32 math, one rounding; pad channels zero
    B, C, H, W = 2, 3, 9, 21
    img = torch.rand(B, C, H, W, generator=g) * 2 - 1
    m = torch.rand(B, 1, H, W, generator=g)
    m[0, :, :4] = 1.0
    m[1, :, 5:] = 0.0
    buf, ptr, guard = _guarded(B * H * W * 8)
    imgd, md = img.cuda(), m.cuda()
    L.check(lib.pp_masked_image_pack(imgd.data_ptr(), md.data_ptr(), B, C, H, W, ptr, code, st), "pack")
    got = buf[guard:-guard].view(dtype).view(B, H, W, 8).cpu()
    want = ((1.0 - m) * img).permute(0, 2, 3, 1).to(dtype)                               # the same two fp32 operations
    assert torch.equal(got[..., :3], want) and bool((got[..., 3:] == 0).all())
    assert bool((buf[:guard] == POISON).all()) and bool((buf[-guard:] == POISON).all())


def _blend_inputs(B, C, h, w, f, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    s = (torch.randn(B, h, w, C, generator=g) * 2).to(dtype)
    c = (torch.randn(B, h, w, C, generator=g) * 2 + 0.5).to(dtype)
    H, W = h * f, w * f
    mask = torch.rand(B, H, W, generator=g)                   # fractional, and different for every batch item
    mask[0, : H // 3] = 1.0
    mask[-1, :, W // 2:] = 0.0
    return s, c, mask


def _check_acc(acc, stored, groups, parts_per_channel):
    """acc: int64 [B][groups][2] against float64 sums of `stored` [B][h][w][C]."""
    B, h, w, C = stored.shape
    cg = C // groups
    v = stored.double().reshape(B, h * w, groups, cg)
    u = 2.0 ** -24
    got_s = acc[..., 0].double() / 2 ** 24
    got_q = acc[..., 1].double() / 2 ** 20
    want_s, want_q = v.sum((1, 3)), (v * v).sum((1, 3))
    tol_s = 7 * u * v.abs().sum((1, 3)) + parts_per_channel * cg * 2.0 ** -25
    tol_q = 7 * u * want_q + parts_per_channel * cg * 2.0 ** -21
    assert bool(((got_s - want_s).abs() <= tol_s).all()), ((got_s - want_s).abs() / tol_s).max().item()
    assert bool(((got_q - want_q).abs() <= tol_q).all()), ((got_q - want_q).abs() / tol_q).max().item()


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("C,groups", [(64, 32), (192, 32)])       # 192 / 32 = 6 channels per group: groups straddle the 8-channel chunks and the 64-channel slabs
@pytest.mark.parametrize("f", [1, 2, 4, 8])
def test_mask_blend_elementwise_bound_and_statistics(dt, C, groups, f):
    L, lib = _lib()
    dtype = DT[dt]
    B, Hm, Wm = 2, 32, 48
    h, w = Hm // f, Wm // f                                   # 1536 (six workgroups), 384 (a partial one), 96, 24 pixels
    s, c, mask = _blend_inputs(B, C, h, w, f, dtype, seed=f * 100 + C)
    sd, cd, md = s.cuda(), c.cuda(), mask.cuda()
    buf, out_ptr, guard = _guarded(s.numel())
    acc = torch.zeros(B, groups, 2, dtype=torch.int64, device="cuda")
    L.check(lib.pp_mask_blend(sd.data_ptr(), cd.data_ptr(), md.data_ptr(), out_ptr, B, h, w, C, Hm, Wm, acc.data_ptr(), groups,
                              L.dtype_code(dtype), torch.cuda.current_stream().cuda_stream), "pp_mask_blend")
    torch.cuda.synchronize()
    got = buf[guard:-guard].view(dtype).view(B, h, w, C).cpu()
    assert bool((buf[:guard] == POISON).all()) and bool((buf[-guard:] == POISON).all()), "guard band written"
    # nearest: source index floor(i * H / h) = i * f
    m = mask[:, ::f, ::f].double().unsqueeze(-1)
    assert torch.equal(m[..., 0].float(), F.interpolate(mask[:, None], size=(h, w), mode="nearest")[:, 0])
    a, b = s.double() * m, c.double() * (1 - m)
    e = a + b
    u, u16 = 2.0 ** -24, (2.0 ** -8 if dt == "bf16" else 2.0 ** -11)
    e32 = ((1 + u) ** 3 - 1) * (a.abs() + b.abs())
    bound = e32 + u16 * (e.abs() + e32) + 2.0 ** -25
    err = (got.double() - e).abs()
    assert bool((err <= bound).all()), f"max err / bound {(err / bound).max().item():.3f}"
    parts = (h * w + 255) // 256 * 32                          # threads that own a channel: 32 per 256-pixel workgroup
    _check_acc(acc.cpu(), got, groups, parts)
    # exact ends of the blend: m = 1 hands the sample on, m = 0 the condition (values, whatever the sign of a zero)
    one, zero = (m[..., 0] == 1.0), (m[..., 0] == 0.0)
    assert bool(one.any()) and bool(zero.any())
    assert torch.equal(got[one].float(), s[one].float()) and torch.equal(got[zero].float(), c[zero].float())
    # a second launch adds to the accumulators: exactly twice the first
    first = acc.clone()
    L.check(lib.pp_mask_blend(sd.data_ptr(), cd.data_ptr(), md.data_ptr(), out_ptr, B, h, w, C, Hm, Wm, acc.data_ptr(), groups,
                              L.dtype_code(dtype), torch.cuda.current_stream().cuda_stream), "pp_mask_blend")
    assert torch.equal(acc, 2 * first)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_mask_blend_in_place_and_statistics_only(dt):
    L, lib = _lib()
    dtype = DT[dt]
    code, st = L.dtype_code(dtype), torch.cuda.current_stream().cuda_stream
    B, C, h, w, f, groups = 2, 128, 12, 20, 2, 32
    s, c, mask = _blend_inputs(B, C, h, w, f, dtype, seed=9)
    sd, cd, md = s.cuda(), c.cuda(), mask.cuda()
    out = torch.empty_like(sd)
    acc = torch.zeros(B, groups, 2, dtype=torch.int64, device="cuda")
    L.check(lib.pp_mask_blend(sd.data_ptr(), cd.data_ptr(), md.data_ptr(), out.data_ptr(), B, h, w, C, h * f, w * f,
                              acc.data_ptr(), groups, code, st), "out of place")
    inpl, acc2 = sd.clone(), torch.zeros_like(acc)
    L.check(lib.pp_mask_blend(inpl.data_ptr(), cd.data_ptr(), md.data_ptr(), inpl.data_ptr(), B, h, w, C, h * f, w * f,
                              acc2.data_ptr(), groups, code, st), "in place")
    assert torch.equal(inpl.view(torch.int16), out.view(torch.int16)) and torch.equal(acc, acc2)
    # no condition tensor: nothing is written, the accumulators get the sums of the sample -- the same sums a blend with a mask
    # of ones takes (it stores the sample's values)
    acc3, keep = torch.zeros_like(acc), sd.clone()
    L.check(lib.pp_mask_blend(sd.data_ptr(), None, None, None, B, h, w, C, 0, 0, acc3.data_ptr(), groups, code, st), "stats")
    assert torch.equal(sd.view(torch.int16), keep.view(torch.int16))
    _check_acc(acc3.cpu(), s, groups, (h * w + 255) // 256 * 32)
    acc4, ones = torch.zeros_like(acc), torch.ones_like(md)
    L.check(lib.pp_mask_blend(sd.data_ptr(), cd.data_ptr(), ones.data_ptr(), out.data_ptr(), B, h, w, C, h * f, w * f,
                              acc4.data_ptr(), groups, code, st), "ones")
    assert torch.equal(acc3, acc4)
    # refusals: a mask that is no whole multiple of the sample, channels off the 64 grid, nothing to do
    bad = lambda *a: lib.pp_mask_blend(*a, code, st)      # noqa: E731
    assert bad(sd.data_ptr(), cd.data_ptr(), md.data_ptr(), out.data_ptr(), B, h, w, C, h * f + 1, w * f, None, 0) == -1
    assert bad(sd.data_ptr(), cd.data_ptr(), md.data_ptr(), out.data_ptr(), B, h, w, 96, h * f, w * f, None, 0) == -1
    assert bad(sd.data_ptr(), None, None, None, B, h, w, C, 0, 0, None, 0) == -1
