"""Shared by the FreeU tests and the fixture generator (not a test file).

FreeU as the reference runs it: `UNet2DConditionModel.enable_freeu(s1, s2, b1, b2)` (powerpaint/models/unet_2d_condition.py:
835-866 of the reference) sets four attributes on every up block; both up-block classes then call diffusers-0.27
`apply_freeu` per resnet, right before `torch.cat([hidden_states, res_hidden_states], 1)` (powerpaint/models/
unet_2d_blocks.py:2563-2587 and 2706-2730).  diffusers itself is not a dependency of this repository, so the two functions
are restated here from their contract:

  * `fourier_filter`: fftn -> fftshift -> mask (== scale on rows H//2-1 : H//2+1 and columns W//2-1 : W//2+1, 1 elsewhere)
    -> ifftshift -> ifftn -> .real.  Computed in fp32 here for every size (diffusers upcasts only the non-power-of-two ones).
  * `apply_freeu`: resolution_idx 0 -> hidden[:, :C//2] *= b1 (an in-place slice assignment), res = filter(res, 1, s1);
    resolution_idx 1 -> the same with b2, s2; other blocks untouched.

`freeu_closed_form` is what csrc/freeu.hip computes: after the shift index H//2 is frequency 0 for even and odd H alike, so
the mask scales the four bins (u, v) in {-1, 0}^2 and
    y = x + (s - 1) / (H W) * Re sum_{(u,v)} X(u,v) e^{+2 pi i (u h / H + v w / W)}
is seven real sums per plane and one multiply-add pass.
"""
import math

import torch

# sizes of the CPU closed-form check: even, odd (centre index), non-square, the 2x2 alias case, the 32x32 level
CPU_SIZES = [(8, 8), (16, 16), (9, 9), (12, 20), (2, 2), (3, 5), (32, 32)]

# (B, H, W, Ch, Cs) of the op test
OP_SHAPES = [
    (2, 8, 8, 1280, 1280),      # SD-1.5 up block 0
    (2, 16, 16, 1280, 640),     # up block 1's last resnet: groups of 60 channels straddle Ch / 2 and Ch
    (1, 9, 9, 320, 320),        # odd size, centre index; Ch / 2 = 160 is no multiple of the 64-channel slab
    (2, 12, 20, 320, 160),      # non-square, non-power-of-two; a partial slab; groups of 15 channels (odd)
    (1, 32, 32, 640, 640),      # the 1024^2 level: the slab does not fit the LDS copy
    (3, 2, 2, 64, 64),          # -1 aliases +1
]

FREEU_FULL = dict(s1=0.9, s2=0.2, b1=1.5, b2=1.6)
FREEU_SKIP_ONLY = dict(s1=0.9, s2=0.2, b1=1.0, b2=1.0)
FREEU_BACKBONE_ONLY = dict(s1=1.0, s2=1.0, b1=1.5, b2=1.6)


def fourier_filter(x_in: torch.Tensor, threshold: int, scale: float) -> torch.Tensor:
    """[B, C, H, W] -> the same shape and dtype (restatement of diffusers-0.27 `fourier_filter`, fp32 throughout)."""
    x = x_in.to(torch.float32)
    B, C, H, W = x.shape
    x_freq = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones((B, C, H, W), device=x.device)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    x_freq = torch.fft.ifftshift(x_freq * mask, dim=(-2, -1))
    return torch.fft.ifftn(x_freq, dim=(-2, -1)).real.to(x_in.dtype)


def apply_freeu(resolution_idx, hidden_states, res_hidden_states, **freeu_kwargs):
    """Restatement of diffusers-0.27 `apply_freeu` (the slice of hidden_states is assigned in place, as there)."""
    for idx, (b, s) in enumerate((("b1", "s1"), ("b2", "s2"))):
        if resolution_idx == idx:
            half = hidden_states.shape[1] // 2
            hidden_states[:, :half] = hidden_states[:, :half] * freeu_kwargs[b]
            res_hidden_states = fourier_filter(res_hidden_states, threshold=1, scale=freeu_kwargs[s])
    return hidden_states, res_hidden_states


def freeu_closed_form(x: torch.Tensor, scale: float) -> torch.Tensor:
    """The four-bin form of fourier_filter(x, 1, scale), fp32 [B, C, H, W]: seven sums and one multiply-add pass."""
    x = x.to(torch.float32)
    H, W = x.shape[-2:]
    th = 2.0 * math.pi * torch.arange(H, dtype=torch.float64) / H
    ph = 2.0 * math.pi * torch.arange(W, dtype=torch.float64) / W
    ch, sh = torch.cos(th).float()[:, None], torch.sin(th).float()[:, None]
    cw, sw = torch.cos(ph).float()[None, :], torch.sin(ph).float()[None, :]
    cd, sd = ch * cw - sh * sw, sh * cw + ch * sw
    fs = [torch.ones(H, W), ch.expand(H, W), sh.expand(H, W), cw.expand(H, W), sw.expand(H, W), cd, sd]
    d = torch.zeros_like(x)
    for f in fs:
        f = f.to(x.device)
        d = d + (x * f).sum((-2, -1), keepdim=True) * f
    return x + d * ((scale - 1.0) / (H * W))


def ulp16(ref: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Spacing of `dtype` (bf16: 8 significant bits, fp16: 11, subnormals below 2^-14) at the magnitude of fp32 `ref`."""
    bits, emin = (8, -126) if dtype == torch.bfloat16 else (11, -14)
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin)))
    return torch.exp2(e - (bits - 1))


def op_inputs(shape, dtype, seed=0):
    """(hidden, skip) NHWC in `dtype`: distinct data per batch item, a non-zero mean (bin (0, 0) matters), a smooth
    component (the three other bins matter)."""
    B, H, W, Ch, Cs = shape
    g = torch.Generator("cpu").manual_seed(1000 + seed)
    hid = torch.randn(B, H, W, Ch, generator=g) + 0.25
    yy = torch.arange(H, dtype=torch.float32)[None, :, None, None] / H
    xx = torch.arange(W, dtype=torch.float32)[None, None, :, None] / W
    amp = torch.randn(B, 1, 1, Cs, generator=g)
    skip = torch.randn(B, H, W, Cs, generator=g) + 0.5 + amp * torch.cos(2 * math.pi * (yy + 0.3 * xx)) + \
        0.5 * torch.sin(2 * math.pi * xx) * torch.arange(1, B + 1, dtype=torch.float32)[:, None, None, None]
    return hid.to(dtype), skip.to(dtype)


def close_gate(out: torch.Tensor, ref: torch.Tensor):
    """(cosine, max abs error, passes) under the gate tests/test_golden.py applies to this architecture."""
    out, ref = out.float().cpu(), ref.float()
    cos = torch.nn.functional.cosine_similarity(out.flatten(), ref.flatten(), dim=0).item()
    err = (out - ref).abs().max().item()
    return cos, err, bool(cos >= 0.999 and err <= 3e-2 * max(1.0, ref.abs().max().item()))


def net_inputs():
    """Inputs of the network fixture (regenerated, not stored): 64x64 latents, so up block 0 runs at 8x8 and up block 1 at
    16x16; batch 2; BrushNet residuals = 0.1 randn of the fork UNet's shapes (8 down, 1 mid, 11 up at this architecture)."""
    g = torch.Generator("cpu").manual_seed(4242)
    inp = dict(x9=torch.randn(2, 9, 64, 64, generator=g), x4=torch.randn(2, 4, 64, 64, generator=g),
               ehs=torch.randn(2, 77, 768, generator=g), t=torch.tensor(681))
    c = (320, 320, 640, 640)
    down = [(c[0], 64)]
    for i, ci in enumerate(c):
        down.append((ci, 64 >> i))
        if i != len(c) - 1:
            down.append((ci, 64 >> (i + 1)))
    up = []
    for i, ci in enumerate(reversed(c)):
        s = 8 << i
        up += [(ci, s), (ci, s)]
        if i != len(c) - 1:
            up.append((ci, 2 * s))
    mk = lambda lst: [0.1 * torch.randn(2, ch, s, s, generator=g) for ch, s in lst]      # noqa: E731
    inp["down"], inp["mid"], inp["up"] = mk(down), mk([(c[-1], 8)])[0], mk(up)
    return inp
