"""-m gpu: the kernels of the CLIP vision tower through the C ABI, in bf16 and fp16 -- pp_vit_patchify (bit for bit against
F.unfold), pp_vit_embed_ln (against fp64 at pp_layernorm's gate plus the one fp32 sum in front of it, and an exact probe) and
the GEMM's PP_ACT_GELU epilogue under every tile form and split count of tests/gemm_cases.py.  Derivations:
tests/vit_cases.py.  Outputs are windows of sentinel-filled buffers; every achieved / gate ratio is printed before it is
asserted."""
import os
import sys
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gemm_cases as GC  # noqa: E402
import norm_cases as NC  # noqa: E402
import vit_cases as VC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import ops  # noqa: E402

DEV = "cuda"
SENT = -1232.0          # (a value both 16-bit formats hold exactly)
IDS = [n for _, n in VC.DTYPES]
DT = [d for d, _ in VC.DTYPES]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------ pp_vit_patchify
@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("src_dtype", [torch.float32, None], ids=["f32src", "16src"])
@pytest.mark.parametrize("shape", VC.PATCHIFY_SHAPES, ids=["x".join(map(str, s)) for s in VC.PATCHIFY_SHAPES])
def test_patchify_is_unfold_bit_for_bit(shape, src_dtype, dtype):
    B, H, W, P = shape
    g = torch.Generator().manual_seed(B * 1000 + H + W)
    px = torch.randint(-256, 257, (B, 3, H, W), generator=g).float()          # representable in bf16 and fp16
    src = px.to(src_dtype or dtype)
    assert torch.equal(src.float(), px)
    gh, gw, K = H // P, W // P, 3 * P * P
    rows, cols, guard = B * gh * gw, (K + 63) // 64 * 64, 8
    full = torch.full((rows + 1, cols + guard), SENT, dtype=dtype)            # a guard row, guard columns beyond `cols`
    full[:rows, K:cols] = float("nan")                                        # the pad columns must be WRITTEN
    full = full.to(DEV)
    out = ops.vit_patchify(src.to(DEV), P, out=full[:rows, :cols])
    torch.cuda.synchronize()
    assert out.data_ptr() == full.data_ptr()
    got = full.cpu()
    want = F.unfold(px[:, :, :gh * P, :gw * P], kernel_size=P, stride=P).transpose(1, 2).reshape(rows, K).to(dtype)
    assert torch.equal(got[:rows, :K].view(torch.int16), want.view(torch.int16))
    assert bool((got[:rows, K:cols].view(torch.int16) == 0).all()), "pad columns are not exact (+) zeros"
    assert bool((got[rows:] == SENT).all()) and bool((got[:, cols:] == SENT).all()), "guards were written"


# ------------------------------------------------------------------------------------------------ pp_vit_embed_ln
def _embed_inputs(B, npatch, C, dtype, ldp):
    g = _gen(B, npatch, C)
    patches = torch.full((B * npatch, ldp), 1000.0, dtype=dtype)              # poisoned row pads
    patches[:, :C] = (torch.randn(B * npatch, C, generator=g) * 1.5 + 0.3).to(dtype)
    cls = torch.randn(C, generator=g).to(dtype)
    pos = (torch.randn(npatch + 1, C, generator=g) * 0.5).to(dtype)
    gamma, beta = torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g) * 0.2
    return patches, cls, pos, gamma, beta


def _embed_sum64(patches, cls, pos, B, npatch, C):
    e = torch.empty(B, npatch + 1, C, dtype=torch.float64)
    e[:, 0] = cls.double() + pos[0].double()
    e[:, 1:] = patches[:, :C].double().view(B, npatch, C) + pos[1:].double()
    return e.view(B * (npatch + 1), C)


def _run_embed(patches, cls, pos, gamma, beta, B, C, dtype, eps=1e-5):
    npatch = patches.shape[0] // B
    rows = B * (npatch + 1)
    full = torch.full((rows + 2, C), SENT, dtype=dtype, device=DEV)           # (dense by the ABI: guard rows behind)
    pd = patches.to(DEV)
    ops.vit_embed_ln(pd[:, :C], cls.to(DEV), pos.to(DEV), B, gamma.to(DEV), beta.to(DEV), eps, out=full[:rows])
    torch.cuda.synchronize()
    got = full.cpu()
    assert bool((got[rows:] == SENT).all()), "rows behind the last were written"
    assert torch.equal(pd.cpu().view(torch.int16), patches.view(torch.int16))
    return got[:rows]


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("shape", VC.EMBED_SHAPES, ids=["x".join(map(str, s)) for s in VC.EMBED_SHAPES])
def test_embed_ln_against_float64(shape, dtype):
    B, npatch, C = shape
    worst = {}
    for ldp in (C, C + 24):                                                   # dense patches, and a row stride > C
        patches, cls, pos, gamma, beta = _embed_inputs(B, npatch, C, dtype, ldp)
        got = _run_embed(patches, cls, pos, gamma, beta, B, C, dtype)
        ref, gate = VC.gate_embed_ln(_embed_sum64(patches, cls, pos, B, npatch, C), gamma, beta, 1e-5, dtype)
        assert bool(torch.isfinite(got.float()).all())
        worst[ldp] = NC.worst_ratio(got, ref, gate)
        print(f"[vit] embed_ln B {B} np {npatch} C {C} ldp {ldp} {str(dtype)[6:]}: worst err / gate {worst[ldp]:.3f}")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_embed_ln_exact_probe(dtype):
    """Integer data whose mean and variance are exactly representable: every row of e is a permutation of C/2 values m + 4 and
    C/2 values m - 4 (mean m, variance 16 exactly, every fp32 partial sum an integer below 2^24), gamma = 1, beta = 0, eps = 0
    -- so rstd = 1/4 exactly and the class row and a patch row must EQUAL the fp64 result rounded once: +-1."""
    B, npatch, C = 2, 3, 320
    g = _gen("probe")
    sign = torch.ones(B * (npatch + 1), C)
    for r in range(sign.shape[0]):
        sign[r, torch.randperm(C, generator=g)[:C // 2]] = -1.0
    m = torch.tensor([3.0, -2.0, 5.0, 0.0, 7.0, -6.0, 1.0, 2.0])[:, None]     # the row means
    e = (m + 4.0 * sign).view(B, npatch + 1, C)                               # what class + pos / patch + pos must sum to
    pos = torch.randint(-8, 9, (npatch + 1, C), generator=g).float()
    pos[0] = e[0, 0] - torch.randint(-8, 9, (C,), generator=g).float()
    cls = e[0, 0] - pos[0]
    e[:, 0] = e[0, 0]                                                         # (one class embedding for every image)
    patches = (e[:, 1:] - pos[1:]).reshape(B * npatch, C)
    assert float(patches.abs().max()) <= 64 and float(cls.abs().max()) <= 64  # integers a 16-bit format holds exactly
    patches, cls, pos = patches.to(dtype), cls.to(dtype), pos.to(dtype)
    gamma, beta = torch.ones(C), torch.zeros(C)
    got = _run_embed(patches, cls, pos, gamma, beta, B, C, dtype, eps=0.0)
    e64 = _embed_sum64(patches, cls, pos, B, npatch, C)
    mean = e64.mean(-1, keepdim=True)
    var = ((e64 - mean) ** 2).mean(-1, keepdim=True)              # (torch.var's running update is not exact)
    assert bool((var == 16.0).all()) and bool((mean == mean.round()).all())
    want = ((e64 - mean) / var.sqrt()).to(dtype)
    assert bool((want.float().abs() == 1.0).all())
    for row in (0, 1, npatch + 1, B * (npatch + 1) - 1):                      # a class row, a patch row, the second image's
        assert torch.equal(got[row].view(torch.int16), want[row].view(torch.int16)), row
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


# ------------------------------------------------------------------------------------------------ PP_ACT_GELU
def _gelu_case(M, N, K, dtype, key, exact=False):
    g = _gen("gelu", M, N, K, key)
    if exact:      # x in {-1, 0, 1}, w in {-1, 0, 1} with three non-zeros per row, bias in 0 .. 3: pre = an exact integer in [-3, 6]
        x = torch.randint(-1, 2, (M, K), generator=g).float()
        w = torch.zeros(N, K)
        idx = torch.randint(0, K, (N, 3), generator=g)
        w.scatter_(1, idx, torch.randint(-1, 2, (N, 3), generator=g).float())
        bias = torch.randint(0, 4, (N,), generator=g).float()
    else:
        x = torch.randn(M, K, generator=g)
        w = torch.randn(N, K, generator=g) * K ** -0.5
        bias = torch.randn(N, generator=g)
    x, w = x.to(dtype), w.to(dtype)
    pre = x.double() @ w.double().t() + bias.double()
    A = x.double().abs() @ w.double().abs().t() + bias.double().abs()
    return x, w, bias, pre, A


def _run_gelu(x, w, bias, tile, splitk, dtype, act=None):
    M, N = x.shape[0], w.shape[0]
    full = torch.full((M + 2, N + 8), SENT, dtype=dtype, device=DEV)
    ops.gemm(x.to(DEV), w.to(DEV), bias.to(DEV), act=L.PP_ACT_GELU if act is None else act, tile=tile, splitk=splitk,
             out=full[:M, :N])
    torch.cuda.synchronize()
    got = full.cpu()
    assert bool((got[M:] == SENT).all()) and bool((got[:, N:] == SENT).all()), "bytes outside the window were written"
    return got[:M, :N]


@pytest.mark.parametrize("dtype", DT, ids=IDS)
@pytest.mark.parametrize("tile", GC.TILE_IDS)
def test_gelu_epilogue_under_every_tile_form_and_split(tile, dtype):
    """Every tile id of gemm_cases.TILE_IDS x every split count of gemm_cases.SPLITS at the smallest M / N / K of the plain
    matrix (40 rows; 160 columns -- 36 where the register-staged kernel or the library's choice takes them; K = 64 in one
    pass, 704 under K splits: ragged slices, 8 splits leave slices of 2, 1 and 0 K tiles): the random regime at the derived
    gate and the integer probe, where the pre-activation is an exact small integer (vit_cases: from -3 up) and the output
    must be fp64 x Phi(x) to within one unit of the 16-bit format."""
    u = GC.unit_roundoff(dtype)
    v2 = bool(tile) and GC.TILES[tile][2]
    M, N = GC.PLAIN_M[0], (GC.PLAIN_N[1] if v2 else GC.PLAIN_N[0])
    worst = {}
    for sk in VC.SPLITS:
        K = GC.PLAIN_K[0] if sk == 1 else GC.PLAIN_K[2]
        x, w, bias, pre, A = _gelu_case(M, N, K, dtype, sk)
        got = _run_gelu(x, w, bias, tile, sk, dtype)
        ref, gate = VC.gate_gelu(pre, A, K, sk, u)
        worst[sk] = GC.worst_ratio(got, ref, gate)
        x, w, bias, pre, A = _gelu_case(M, N, K, dtype, sk, exact=True)
        assert bool((pre == pre.round()).all()) and VC.PROBE_MIN <= float(pre.min()) and float(pre.max()) <= 6
        got = _run_gelu(x, w, bias, tile, sk, dtype).double()
        ref = VC.gelu64(pre)
        ulp = 2.0 * u * torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -14))))   # one unit in the last place of ref
        bad = (got - ref).abs() > ulp
        assert not bool(bad.any()), (tile, sk, pre[bad][:4], got[bad][:4], ref[bad][:4])
        assert bool((got[pre == 0] == 0).all())
    print(f"[vit] gelu tile {tile} {str(dtype)[6:]}: worst err / gate per split {worst}")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("dtype", DT, ids=IDS)
def test_gelu_epilogue_at_257_rows(dtype):
    """fc1 of the tower at 257 tokens (ragged last tile in every tile height), the library's own choice of form."""
    M, N, K = 257, 640, 320
    x, w, bias, pre, A = _gelu_case(M, N, K, dtype, 0)
    got = _run_gelu(x, w, bias, 0, 0, dtype)
    ref, gate = VC.gate_gelu(pre, A, K, 8, GC.unit_roundoff(dtype))           # (whatever split count the library took: <= 8)
    r = GC.worst_ratio(got, ref, gate)
    print(f"[vit] gelu 257 x 640 x 320 {str(dtype)[6:]}: worst err / gate {r:.3f}")
    assert r <= 1.0, r
    none = _run_gelu(x, w, bias, 0, 0, dtype, act=L.PP_ACT_NONE)
    assert not torch.equal(none, got)
    with pytest.raises(L.PPError, match="PP_ERR_BAD_ARG"):
        _run_gelu(x, w, bias, 0, 0, dtype, act=5)
