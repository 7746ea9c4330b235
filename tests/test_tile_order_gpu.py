"""-m gpu: the grouped tile order (csrc/tile_order.h, PPGemmArgs.tile_group_m) on the three GEMM-class kernels, through the C ABI.

A tile's arithmetic does not depend on the workgroup that runs it, so every forced group height -- 1 (M-major), 2, one that does
not divide the M tiles of the launch, and the M tiles themselves (N-major) -- must give the group_m = 1 result bit for bit, and
that result must EQUAL the fp64 model cast once (the exact integer probes of tests/gemm_cases.py: every partial sum is an
integer below 2^24).  Outputs are windows of sentinel-filled buffers: a tile the decode never reaches leaves the sentinel inside
the window (not equal to the model), a tile reached twice or misplaced writes outside it or over another tile.

Shapes: the smallest at which an order can go wrong -- 5 x 3 tiles with ragged last rows and columns (plain GEMM, one pass and
two K splits behind the separate combine), 8 x 2 tiles with the in-kernel combine (its splits must still share an XCD), the
tap-major conv on 3 x 2 tiles, the halo-tile conv on 6 x 2 tiles of 128 rows and 9 x 2 tiles of 64 rows (a plain conv reaches
the halo-tile loop only with the automatic tile, which takes 128 rows at 16x16; 64-row tiles at 16x12), the fused-norm conv on
12 x 2 tiles of 64 rows, and the sub-pixel form (four parities in front of the decode).  bf16 and fp16.

The fused-norm case has an exact model too: gamma = beta = 0 makes every normalised activation SiLU(0) = 0 whatever the
(random) input holds, so the result is the 1x1 tail over integer x3 plus integer bias, row vector and residual -- computed by
the halo-tile kernel's tail phase and epilogue at the position the decode gives it.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gemm_cases as GC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import ops  # noqa: E402

DEV = "cuda"

#        case                                                                             M tiles  group heights
CASES = [(GC.Case("plain", "E", 300, 400, 128, 0, 32, 1), 5, (1, 2, 3, 5)),
         (GC.Case("plain", "E", 300, 400, 128, 0, 32, 2), 5, (1, 2, 3, 5)),
         (GC.Case("plain", "E", 1024, 320, 256, 0, 54, 2, side="fuse"), 8, (1, 2, 3, 8)),
         (GC.Case("conv", "E", 0, 200, 64, 0, 32, 1, B=3, H=8, W=8), 3, (1, 2, 3)),
         (GC.Case("conv", "E", 0, 200, 64, 0, 0, 0, B=3, H=16, W=16), 6, (1, 2, 4, 6)),
         (GC.Case("conv", "E", 0, 200, 64, 0, 0, 0, B=3, H=12, W=16), 9, (1, 2, 4, 9)),
         (GC.Case("subpix", "E", 0, 160, 64, 0, 0, 0, B=3, H=8, W=8), 3, (1, 2, 3))]


def _nhwc(b, B, H, W):
    return b.full.as_strided((B, H, W, b.cols), (H * W * b.ld, W * b.ld, b.ld, 1), b.base)


def _bits(x):
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)


def _launch(c, t, out, ws, group_m):
    kw = dict(tile=c.tile, splitk=c.splitk, tile_group_m=group_m, workspace=ws)
    if c.kind == "plain":
        ops.gemm(t["x1"].view, t["w"][:c.N], None, out=out.view, fuse_combine="force" if c.side == "fuse" else False, **kw)
    elif c.kind == "subpix":
        ops.conv3x3_up_subpix(_nhwc(t["x1"], c.B, c.H, c.W), t["w"][:4 * c.N].view(4, c.N, -1),
                              out=_nhwc(out, c.B, 2 * c.H, 2 * c.W), **kw)
    else:
        ops.conv3x3(_nhwc(t["x1"], c.B, c.H, c.W), t["w"][:c.N], None, out=_nhwc(out, c.B, c.H, c.W), **kw)


def _order_of(c, group_m):
    """what the library says it runs: the request as the wrappers build it, asked through pp_gemm_tile_group_m"""
    import ctypes as C
    if c.kind == "plain":
        a = L.gemm_args(L.PP_DT_BF16, c.M, c.N, c.K1, 0x1000, 0x2000, 0x3000)
    else:
        a = L.conv3x3_args(L.PP_DT_BF16, c.B, c.H, c.W, c.K1, c.N, 0x1000, w=0x2000, out=0x3000)
        if c.kind == "subpix":
            a.K, a.subpix = 4 * c.K1, 1
    a.tile, a.splitk, a.tile_group_m = c.tile, c.splitk, group_m
    return L.lib().pp_gemm_tile_group_m(C.byref(a))


@pytest.mark.parametrize("dtype,fmt", GC.DTYPES, ids=[f for _, f in GC.DTYPES])
@pytest.mark.parametrize("c,tiles_m,groups", CASES, ids=[c.id for c, _, _ in CASES])
def test_every_group_height_gives_the_same_bits(c, tiles_m, groups, dtype, fmt):
    t = GC.build(c, dtype, DEV)
    expected = GC.expected_windows(c, t, dtype)["out"]
    orows = c.rows * (4 if c.kind == "subpix" else 1)
    words = 8 * c.rows * c.N + ((c.rows + 63) // 64) * ((c.N + 159) // 160) * 6144 // 4
    first = None
    for g in groups + (tiles_m + 7,):                  # (a height beyond the M tiles is clamped to them)
        assert _order_of(c, g) == min(g, tiles_m), (c.id, g, "the form has other M tiles than the case means")
        out = GC.sentinel_out(orows, c.N, GC.PAD_COLS, dtype).to(DEV)
        ws = torch.zeros(words, dtype=torch.float32, device=DEV)
        _launch(c, t, out, ws, g)
        torch.cuda.synchronize()
        if c.side == "fuse":
            assert ops.last_combine["fused"], (c.id, g, "the launch did not combine in-kernel")
            assert ops.combine_faults(DEV) == 0, (c.id, g, "splits of a tile on different XCDs")
        got = out.view.clone()
        assert bool((_bits(out.full)[out.outside()] == GC.SENTINEL16).all()), (c.id, fmt, g, "bytes outside the window were written")
        ne = got.double() != expected
        assert not bool(ne.any()), (c.id, fmt, f"group_m {g}", "not equal to the fp64 model", int(ne.sum()), "elements; first",
                                    ne.nonzero()[0].tolist())
        if first is None:
            first = got
        assert torch.equal(_bits(got), _bits(first)), (c.id, fmt, f"group_m {g} differs from group_m 1")


@pytest.mark.parametrize("dtype,fmt", GC.DTYPES, ids=[f for _, f in GC.DTYPES])
def test_fused_norm_conv_in_every_group_height(dtype, fmt):
    """3 images of 16x16 on 64-row tiles (12 x 2 tiles), 64 -> 200 channels + a 64-channel 1x1 tail; see the module docstring"""
    B, H, W, C, C3, N = 3, 16, 16, 64, 64, 200
    g = torch.Generator("cpu").manual_seed(11)
    x = torch.randn(B, H, W, C, generator=g).to(dtype).to(DEV)
    x3 = torch.randint(-2, 3, (B, H, W, C3), generator=g).to(dtype).to(DEV)
    w = torch.randint(-2, 3, (N, 9 * C + C3), generator=g).to(dtype).to(DEV)
    bias = torch.randint(-8, 9, (N,), generator=g).float().to(DEV)
    rowvec = torch.randint(-8, 9, (B, N), generator=g).float().to(DEV)
    res = torch.randint(-8, 9, (B, H, W, N), generator=g).to(dtype).to(DEV)
    xf = x.double().reshape(B, H * W, 32, C // 32)
    acc = torch.stack([(xf.sum((1, 3)) * 2 ** 24).round().long(), ((xf * xf).sum((1, 3)) * 2 ** 20).round().long()], -1).contiguous()
    gb = ops.gn_gamma_beta(torch.zeros(C, device=DEV), torch.zeros(C, device=DEV))
    model = (x3.double().reshape(-1, C3) @ w[:, 9 * C:].double().t() + bias.double() + rowvec.double().repeat_interleave(H * W, 0)
             + res.double().reshape(-1, N)).to(dtype).double()
    first = None
    for gm in (1, 2, 5, 12):
        out = GC.sentinel_out(B * H * W, N, GC.PAD_COLS, dtype).to(DEV)
        ops.conv3x3(x, w, bias, x3=x3, rowvec=rowvec, res1=res, tile=L.PP_TILE_64x160, splitk=1, tile_group_m=gm,
                    gn_in=(acc, gb, 32, 1e-5), out=_nhwc(out, B, H, W))
        torch.cuda.synchronize()
        got = out.view.clone()
        assert bool((_bits(out.full)[out.outside()] == GC.SENTINEL16).all()), (fmt, gm, "bytes outside the window were written")
        ne = got.double() != model
        assert not bool(ne.any()), (fmt, f"group_m {gm}", "not equal to the fp64 model", int(ne.sum()), ne.nonzero()[0].tolist())
        if first is None:
            first = got
        assert torch.equal(_bits(got), _bits(first)), (fmt, f"group_m {gm} differs from group_m 1")


def test_a_negative_group_height_is_refused():
    x = torch.zeros(64, 64, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(160, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(L.PPError, match="PP_ERR_BAD_ARG"):
        ops.gemm(x, w, tile_group_m=-1)
