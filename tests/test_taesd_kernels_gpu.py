"""GPU: the kernels AutoencoderTiny adds (csrc/taesd.hip), probed exactly.

pp_conv3x3_c64 -- small-integer activations and weights (x in [-3, 3], w in [-2, 2], K = 576 terms: |sum| <= 3456), bias in
halves in [-4, 4], residual in [-8, 8]: every partial sum is an integer or a half-integer below 2^13, exact in the fp32
accumulator in ANY summation order.  The kernel must reproduce float64 `F.conv2d` (stride 2 / behind `F.interpolate(nearest,
2x)` for modes 1 / 2) + bias + residual, ReLU, rounded once to the 16-bit format, bit for bit.  Outputs sit inside poisoned
guard bands; the operands must come back unmodified.

pp_taesd_pack -- fp32 arithmetic, one rounding.  (x + 1) / 2 on the grid x = k / 128 - 1 is exact in fp32 and in both 16-bit
formats (k / 256, k < 2^8): bit for bit.  On random inputs the fp32 value is within a few fp32 ulps of the float64 one, far
below a 16-bit ulp, so the stored value is one of the two 16-bit neighbours of the float64 value (only a near-tie can pick the
other one).
"""
import pytest
import torch
import torch.nn.functional as F

import taesd_cases as TC

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
POISON = 0x7B5A          # a 16-bit pattern no probe produces (bf16 2.8e36 / fp16 60224)


def _lib():
    from powerpaint_amd import _lib as L
    return L, L.lib()


def _guarded(n_elems, guard=4096):
    """int16 buffer [guard | n_elems | guard] filled with the poison; returns (buffer, pointer of the payload, guard)."""
    buf = torch.full((n_elems + 2 * guard,), POISON, dtype=torch.int16, device="cuda")
    return buf, buf.data_ptr() + 2 * guard, guard


def _probe(B, H, W, mode, bias, res, seed):
    """Integer probe in float64 NCHW: x, w, bias | None, res | None (of the output's shape), the exact result before ReLU."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (B, 64, H, W), generator=g).double()
    w = torch.randint(-2, 3, (64, 64, 3, 3), generator=g).double()
    b = torch.randint(-8, 9, (64,), generator=g).double() / 2 if bias else None
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if mode == 2 else x
    want = F.conv2d(xin, w, b, stride=2 if mode == 1 else 1, padding=1)
    r = None
    if res:
        r = torch.randint(-8, 9, tuple(want.shape), generator=g).double()
        want = want + r
    assert want.abs().max() < 2 ** 13
    return x, w, b, r, want


def _nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(dtype)


def _run(lib, L, dtype, xd, B, H, W, wd, bd, rd, mode, relu, n_out):
    buf, out_ptr, guard = _guarded(n_out)
    L.check(lib.pp_conv3x3_c64(xd.data_ptr(), B, H, W, wd.data_ptr(), bd.data_ptr() if bd is not None else None,
                               rd.data_ptr() if rd is not None else None, mode, int(relu), out_ptr, L.dtype_code(dtype),
                               torch.cuda.current_stream().cuda_stream), "pp_conv3x3_c64")
    torch.cuda.synchronize()
    assert bool((buf[:guard] == POISON).all()) and bool((buf[-guard:] == POISON).all()), "guard band written"
    return buf[guard:-guard].clone()


def _check_conv(dt, B, H, W, mode, bias, res, relu):
    from powerpaint_amd.engine import _conv_igemm
    L, lib = _lib()
    dtype = DT[dt]
    x, w, b, r, want = _probe(B, H, W, mode, bias, res, seed=1000 * mode + 100 * B + H + W + 7 * bias + 3 * res)
    if relu:
        assert bool((want < 0).any()) and bool((want > 0).any())
        want = F.relu(want)
    Ho, Wo = want.shape[-2:]
    assert (Ho, Wo) == ((H, W), ((H - 1) // 2 + 1, (W - 1) // 2 + 1), (2 * H, 2 * W))[mode]
    want16 = _nhwc(want, dtype)                                                          # one rounding
    x16, w16 = _nhwc(x, dtype), _conv_igemm(w).contiguous().to(dtype)
    r16 = _nhwc(r, dtype) if res else None
    xd, wd = x16.cuda(), w16.cuda()
    bd = b.float().cuda() if bias else None
    rd = r16.cuda() if res else None
    got = _run(lib, L, dtype, xd, B, H, W, wd, bd, rd, mode, relu, want16.numel()).view(dtype).view(B, Ho, Wo, 64).cpu()
    bad = (got.view(torch.int16) != want16.view(torch.int16))
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} values differ, first at {bad.nonzero()[0].tolist()}, " \
                                f"{(got.double() - want16.double()).abs().max().item()} off at most"
    # the operands come back unmodified
    assert torch.equal(xd.cpu().view(torch.int16), x16.view(torch.int16)) and torch.equal(wd.cpu().view(torch.int16), w16.view(torch.int16))
    if bias:
        assert torch.equal(bd.cpu(), b.float())
    if res:
        assert torch.equal(rd.cpu().view(torch.int16), r16.view(torch.int16))


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B,H,W", TC.CONV_SHAPES)
def test_conv3x3_c64_is_exact_on_integer_probes(dt, mode, B, H, W):
    for bias, res, relu in TC.pairwise_flags():
        _check_conv(dt, B, H, W, mode, bias, res, relu)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_conv3x3_c64_persistent_workgroups_walk_more_than_one_tile(dt):
    _check_conv(dt, *TC.CONV_BIG, 0, 1, 1, 1)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_conv3x3_c64_item_of_a_batch_has_the_bits_of_the_item_alone(dt, mode):
    """Non-integer data (the sums are rounded in fp32): the same bits whatever the batch and the item's place in it."""
    L, lib = _lib()
    dtype = DT[dt]
    B, H, W = 3, 17, 33
    g = torch.Generator().manual_seed(40 + mode)
    x = torch.randn(B, H, W, 64, generator=g).to(dtype).cuda()
    w = (torch.randn(64, 576, generator=g) / 24).to(dtype).cuda()
    b = torch.randn(64, generator=g).cuda()
    Ho, Wo = ((H, W), ((H - 1) // 2 + 1, (W - 1) // 2 + 1), (2 * H, 2 * W))[mode]
    r = torch.randn(B, Ho, Wo, 64, generator=g).to(dtype).cuda()
    per = Ho * Wo * 64
    full = _run(lib, L, dtype, x, B, H, W, w, b, r, mode, True, B * per).view(B, per)
    for i in range(B):
        alone = _run(lib, L, dtype, x[i:i + 1].contiguous(), 1, H, W, w, b, r[i:i + 1].contiguous(), mode, True, per)
        assert torch.equal(alone, full[i]), f"item {i}"
    assert len(torch.unique(full)) > 1000


def test_conv3x3_c64_refuses_what_it_cannot_run():
    L, lib = _lib()
    x = torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(64, 576, dtype=torch.bfloat16, device="cuda")
    o = torch.zeros(1, 16, 16, 64, dtype=torch.bfloat16, device="cuda")
    X, Wt, O = x.data_ptr(), w.data_ptr(), o.data_ptr()
    call = lambda x_, b, h, w_, wt, mode, out, dt: lib.pp_conv3x3_c64(x_, b, h, w_, wt, None, None, mode, 0, out, dt, None)   # noqa: E731
    assert call(X, 1, 8, 8, Wt, 0, O, 1) == 0
    assert call(X, 1, 8, 8, Wt, 0, O, 0) == -1 and call(X, 1, 8, 8, Wt, 0, O, 7) == -1          # dtype: fp32, unknown
    assert call(None, 1, 8, 8, Wt, 0, O, 1) == -1 and call(X, 1, 8, 8, None, 0, O, 1) == -1 and call(X, 1, 8, 8, Wt, 0, None, 1) == -1
    assert call(X, 1, 8, 8, Wt, 3, O, 1) == -1 and call(X, 1, 8, 8, Wt, -1, O, 1) == -1         # mode outside 0..2
    assert call(X, 0, 8, 8, Wt, 0, O, 1) == -1 and call(X, 1, 0, 8, Wt, 0, O, 1) == -1 and call(X, 1, 8, -2, Wt, 0, O, 1) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------
def _pack(lib, L, src, mode, dtype, c=None):
    B, C, H, W = src.shape
    sdt = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[src.dtype]
    buf, ptr, guard = _guarded(B * H * W * 8)
    sd = src.cuda()
    L.check(lib.pp_taesd_pack(sd.data_ptr(), sdt, B, C, H, W, mode, ptr, L.dtype_code(dtype),
                              torch.cuda.current_stream().cuda_stream), "pp_taesd_pack")
    torch.cuda.synchronize()
    assert bool((buf[:guard] == POISON).all()) and bool((buf[-guard:] == POISON).all()), "guard band written"
    assert torch.equal(sd.cpu(), src)
    got = buf[guard:-guard].view(dtype).view(B, H, W, 8).cpu()
    assert bool((got[..., C:].view(torch.int16) == 0).all()), "pad channels are not zero"      # over a poisoned destination
    return got[..., :C].permute(0, 3, 1, 2)


def _neighbours(e, dtype):
    """The two values of `dtype` around the float64 tensor e (equal where e is representable)."""
    n = e.to(dtype)                                            # nearest
    up = torch.nextafter(n, torch.full_like(n, float("inf")))
    dn = torch.nextafter(n, torch.full_like(n, float("-inf")))
    other = torch.where(n.double() < e, up, torch.where(n.double() > e, dn, n))
    return n, other


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_pack_image_map_is_exact_on_the_grid(dt):
    L, lib = _lib()
    dtype = DT[dt]
    k = (torch.arange(2 * 3 * 257 * 2) % 257).float()                                          # every k in [0, 256]
    src = (k / 128 - 1).view(2, 3, 257, 2)                                                     # 514 pixels: three workgroups
    got = _pack(lib, L, src, 0, dtype)
    want = ((src.double() + 1) / 2).to(dtype)
    assert torch.equal(want.double(), (src.double() + 1) / 2)                                  # representable: no rounding at all
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("src_dt", [torch.float32, torch.bfloat16, torch.float16])
def test_pack_stores_a_neighbour_of_the_float64_value(dt, mode, src_dt):
    L, lib = _lib()
    dtype = DT[dt]
    g = torch.Generator().manual_seed(11 + mode)
    C = 3 if mode == 0 else 4
    src = (torch.rand(2, C, 9, 21, generator=g) * 2 - 1 if mode == 0 else torch.randn(2, C, 9, 21, generator=g) * 4).to(src_dt)
    got = _pack(lib, L, src, mode, dtype)
    e = (src.double() + 1) / 2 if mode == 0 else 3 * torch.tanh(src.double() / 3)
    n, other = _neighbours(e, dtype)
    ok = (got == n) | (got == other)
    assert bool(ok.all()), f"{int((~ok).sum())} values are no neighbour of the float64 value"
    assert (got != n).float().mean() < 0.01                                                     # ... and nearly all the nearest


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_pack_latent_map_saturates_and_refusals(dt):
    L, lib = _lib()
    dtype = DT[dt]
    src = torch.tensor([float("inf"), float("-inf"), 0.0, 1e30, -1e30, 3.0, -3.0, 1e-3]).view(1, 1, 2, 4)
    got = _pack(lib, L, src, 1, dtype)
    want = torch.tensor([3.0, -3.0, 0.0, 3.0, -3.0, 3 * 0.7615941559557649, -3 * 0.7615941559557649, 1e-3]).to(dtype)
    assert torch.equal(got.flatten()[:5], want[:5])
    n, other = _neighbours(torch.tensor([3 * 0.7615941559557649, -3 * 0.7615941559557649, 3 * torch.tanh(torch.tensor(1e-3 / 3,
                           dtype=torch.float64)).item()], dtype=torch.float64), dtype)
    assert bool(((got.flatten()[5:] == n) | (got.flatten()[5:] == other)).all())
    o = torch.zeros(64, dtype=torch.int16, device="cuda")
    s = src.cuda()
    code = L.dtype_code(dtype)
    assert lib.pp_taesd_pack(s.data_ptr(), 0, 1, 1, 2, 4, 2, o.data_ptr(), code, None) == -1      # mode
    assert lib.pp_taesd_pack(s.data_ptr(), 3, 1, 1, 2, 4, 0, o.data_ptr(), code, None) == -1      # source dtype
    assert lib.pp_taesd_pack(s.data_ptr(), 0, 1, 9, 2, 4, 0, o.data_ptr(), code, None) == -1      # more than 8 channels
    assert lib.pp_taesd_pack(None, 0, 1, 1, 2, 4, 0, o.data_ptr(), code, None) == -1
    assert lib.pp_taesd_pack(s.data_ptr(), 0, 1, 1, 2, 4, 0, o.data_ptr(), 0, None) == -1         # 16-bit destination only
