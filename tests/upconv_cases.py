"""Shared by tests/test_upconv_subpix.py (CPU) and tests/test_upconv_subpix_gpu.py: the sub-pixel form of Upsample2D's
`nearest 2x -> conv3x3` written out in torch, independently of any kernel.

Output pixel (2i + a, 2j + b) reads, through tap ky, upsampled row 2i + a + ky - 1 = source row floor((2i + a + ky - 1) / 2):
row i - 1 for (a, ky) = (0, 0), row i + 1 for (1, 2), row i otherwise -- so tap ky lands on dy = 0 (source row i + a - 1) or
dy = 1 (source row i + a) as R[a][dy] below says; columns likewise."""
import torch
import torch.nn.functional as F

R = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}      # R[a][dy] = the taps ky that read source row i + a - 1 + dy


def fold(w: torch.Tensor, dtype=None) -> torch.Tensor:
    """w [Cout, 9*C] (k = (ky*3+kx)*C + c, any float dtype) -> [4, Cout, 4*C] (p = 2a + b, k = (dy*2+dx)*C + c): fp32 sums in
    the order ky outer, kx inner, rounded once to `dtype` (None: left in fp32)."""
    cout, C = w.shape[0], w.shape[1] // 9
    w9 = w.float().reshape(cout, 3, 3, C)
    out = torch.zeros(4, cout, 2, 2, C, dtype=torch.float32, device=w.device)
    for a in (0, 1):
        for b in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    acc = torch.zeros(cout, C, dtype=torch.float32, device=w.device)
                    for ky in R[a][dy]:
                        for kx in R[b][dx]:
                            acc = acc + w9[:, ky, kx, :]
                    out[2 * a + b, :, dy, dx, :] = acc
    out = out.reshape(4, cout, 4 * C)
    return out if dtype is None else out.to(dtype)


def subpix_conv(x: torch.Tensor, wfold: torch.Tensor, bias=None) -> torch.Tensor:
    """x NHWC [B,H,W,C], wfold [4, Cout, 4*C] -> fp32 NHWC [B,2H,2W,Cout]: four 2x2 convs over the zero-padded source, parity
    (a, b) reading the window whose top-left pixel is (i + a - 1, j + b - 1), outputs interleaved."""
    B, H, W, C = x.shape
    cout = wfold.shape[1]
    xp = F.pad(x.float().permute(0, 3, 1, 2), (1, 1, 1, 1))           # source pixel (r, s) sits at (r + 1, s + 1)
    out = torch.zeros(B, 2 * H, 2 * W, cout, dtype=torch.float32, device=x.device)
    for a in (0, 1):
        for b in (0, 1):
            k = wfold[2 * a + b].float().reshape(cout, 2, 2, C).permute(0, 3, 1, 2)
            y = F.conv2d(xp[:, :, a:a + H + 1, b:b + W + 1], k)       # [B, Cout, H, W]
            out[:, a::2, b::2, :] = y.permute(0, 2, 3, 1)
    return out if bias is None else out + bias.float()


def up_conv(x: torch.Tensor, w: torch.Tensor, bias=None) -> torch.Tensor:
    """The op itself: F.interpolate(scale_factor=2, mode="nearest") -> F.conv2d(3x3, padding=1), fp32, NHWC in and out."""
    cout, C = w.shape[0], w.shape[1] // 9
    xu = F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    k = w.float().reshape(cout, 3, 3, C).permute(0, 3, 1, 2)
    return F.conv2d(xu, k, None if bias is None else bias.float(), padding=1).permute(0, 2, 3, 1)
