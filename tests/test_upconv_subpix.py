"""CPU: the algebra of the sub-pixel upsampling conv (PPGemmArgs.subpix), independently of any kernel:
`nearest 2x -> conv3x3` equals four 2x2 convs over the source image on the tap sums R[a][dy] x R[b][dx], and the zero padding
of the upsampled image coincides with zero padding of the source.  fp32 on both sides, so only the order of the sums differs
(measured 1.6e-5 max-abs on outputs of max-abs ~5); and the host-side answers of the library about the form."""
import ctypes as C

import pytest
import torch

import upconv_cases as U


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 8, 8, 64, 160), (1, 8, 16, 128, 96)])
def test_four_2x2_convs_on_folded_weights_are_the_upsampling_conv(B, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(B * 1000 + Cin)
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, 9 * Cin, generator=g) * (9 * Cin) ** -0.5
    bias = torch.randn(Cout, generator=g)
    ref = U.up_conv(x, w, bias)
    out = U.subpix_conv(x, U.fold(w), bias)
    err = (out - ref).abs()
    print(f"max-abs {err.max().item():.3g} on |ref| <= {ref.abs().max().item():.3g}")
    assert err.max().item() <= 1e-4
    # every border row and column of the output on its own: the padding claim
    for name, e in (("top", err[:, :2]), ("bottom", err[:, -2:]), ("left", err[:, :, :2]), ("right", err[:, :, -2:])):
        assert e.max().item() <= 1e-4, name


def test_fold_layout():
    """fold() puts tap (dy, dx) of parity 2a + b at columns (dy*2+dx)*C ..; a weight with a single non-zero tap shows where
    every tap goes: tap (ky, kx) appears in parity (a, b) exactly once, at the (dy, dx) with ky in R[a][dy], kx in R[b][dx]."""
    Cin, Cout = 8, 4
    for ky in range(3):
        for kx in range(3):
            w = torch.zeros(Cout, 3, 3, Cin)
            w[:, ky, kx, :] = 1.0
            f = U.fold(w.reshape(Cout, 9 * Cin)).reshape(4, Cout, 2, 2, Cin)
            for a in (0, 1):
                for b in (0, 1):
                    want = torch.zeros(2, 2)
                    for dy in (0, 1):
                        for dx in (0, 1):
                            if ky in U.R[a][dy] and kx in U.R[b][dx]:
                                want[dy, dx] = 1.0
                    assert want.sum() == 1.0
                    assert torch.equal(f[2 * a + b, 0, :, :, 0], want), (ky, kx, a, b)


def _req(B, H, W, Cin, Cout, splitk=0):
    from powerpaint_amd import _lib as L
    a = L.conv3x3_args(L.PP_DT_BF16, B, H, W, Cin, Cout, 0x1000, w=0x5000, out=0x6000)
    a.K, a.subpix, a.splitk = 4 * Cin, 1, splitk
    return a


def test_the_library_answers_about_the_form_without_a_gpu():
    """pp_upconv_subpix_supported and the refusals of pp_gemm_bf16 are host logic.  The SD-1.5 upsamplers at batch 8: 16 -> 32
    and 32 -> 64 are routed (2), 8 -> 16 runs but stays on the nine-tap weight stream (1); a source narrower than the loader's
    8-pixel strips, channels off the 64 grid and a forced split are refused before anything is launched."""
    from powerpaint_amd import _lib as L
    lib = L.lib()
    sup = lambda B, H, W, c, n: lib.pp_upconv_subpix_supported(B, H, W, c, n, L.PP_DT_BF16)      # noqa: E731
    assert sup(8, 16, 16, 1280, 1280) == 2 and sup(8, 32, 32, 640, 640) == 2 and sup(8, 8, 8, 1280, 1280) == 1
    assert sup(2, 4, 4, 128, 160) == 0 and sup(2, 8, 12, 128, 160) == 0 and sup(2, 8, 8, 96, 160) == 0
    assert sup(1, 8, 16, 128, 160) == 2 and sup(3, 8, 8, 128, 160) == 1 and sup(1, 32, 32, 320, 160) == 2
    assert lib.pp_gemm_bf16(C.byref(_req(2, 4, 4, 128, 160)), None) == -2                 # PP_ERR_UNSUPPORTED: W_src = 4
    assert lib.pp_gemm_bf16(C.byref(_req(2, 16, 16, 128, 160, splitk=2)), None) == -2     # a forced split
    a = _req(2, 16, 16, 128, 160)
    a.up = 1
    assert lib.pp_gemm_bf16(C.byref(a), None) == -1                                       # PP_ERR_BAD_ARG: subpix with up
    a = _req(2, 16, 16, 128, 160)
    a.K = 9 * 128
    assert lib.pp_gemm_bf16(C.byref(a), None) == -1                                       # the nine-tap K on a subpix request
    assert lib.pp_gemm_workspace_bytes(C.byref(_req(2, 16, 16, 128, 160))) == 0           # one pass, no slabs
    # the nine-tap request of the same conv is answered as before: routed to the halo-tile loop from 16 output pixels of width
    b = L.conv3x3_args(L.PP_DT_BF16, 8, 16, 16, 1280, 1280, 0x1000, up=True, w=0x5000, out=0x6000)
    assert lib.pp_conv_gn_supported(C.byref(b)) == 2
