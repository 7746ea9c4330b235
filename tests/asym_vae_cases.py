"""AsymmetricAutoencoderKL restated in plain torch.nn.functional, from the published form (diffusers 0.27
`models/autoencoders/autoencoder_asym_kl.py`; `vae.py`: Encoder, MaskConditionEncoder, MaskConditionDecoder; Zhu et al.,
arXiv:2306.04632).  The specification the HIP path is tested against: it imports nothing from the product and the product
imports nothing from it; it runs in whatever dtype the state dict and the inputs have (fp32 and float64 are used).

    cfg = dict(in_channels, out_channels, latent_channels, down, layers_down, up, layers_up, groups)

State-dict keys are the library's.  GroupNorm eps is 1e-6 everywhere.
"""
import math

import torch
import torch.nn.functional as F

EPS = 1e-6

TINY = dict(in_channels=3, out_channels=3, latent_channels=4, down=(64, 128), layers_down=1, up=(64, 128, 256, 256),
            layers_up=1, groups=32)
X15 = dict(in_channels=3, out_channels=3, latent_channels=4, down=(128, 256, 512, 512), layers_down=2,
           up=(192, 384, 768, 768), layers_up=3, groups=32)
X2 = dict(in_channels=3, out_channels=3, latent_channels=4, down=(128, 256, 512, 512), layers_down=2,
          up=(256, 512, 1024, 1024), layers_up=5, groups=32)
# the condition encoder's weights as published for x-1-5
X15_CONDITION_WEIGHTS = [(192, 3, 3, 3), (384, 192, 3, 3), (768, 384, 4, 4), (768, 768, 4, 4), (768, 768, 4, 4)]


def condition_encoder_channels(out_ch: int, res_ch: int, stride: int = 16):
    """MaskConditionEncoder.__init__(in_ch, out_ch = up[0], res_ch = up[-1], stride = 16): the out channels of its convs, as its
    `while stride > 1` loop produces them."""
    channels = []
    while stride > 1:
        stride = stride // 2
        in_ch_ = out_ch * 2
        if out_ch > res_ch:
            out_ch = res_ch
        if stride == 1:
            in_ch_ = res_ch
        channels.append((in_ch_, out_ch))
        out_ch *= 2
    outs = [o for _, o in channels]
    outs.append(channels[-1][0])
    return outs


def condition_encoder_weight_shapes(cfg):
    outs = condition_encoder_channels(cfg["up"][0], cfg["up"][-1])
    shapes, cin = [], cfg["out_channels"]
    for l, c in enumerate(outs):
        k = 3 if l < 2 else 4
        shapes.append((c, cin, k, k))
        cin = c
    return shapes


def nearest_mask(mask: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """F.interpolate(mask, size=(h, w), mode="nearest"): source index floor(i * H / h)."""
    H, W = mask.shape[-2:]
    iy = torch.tensor([math.floor(i * H / h) for i in range(h)], dtype=torch.long, device=mask.device)
    ix = torch.tensor([math.floor(i * W / w) for i in range(w)], dtype=torch.long, device=mask.device)
    return mask.index_select(-2, iy).index_select(-1, ix)


def _gn(sd, name, x, groups):
    return F.group_norm(x, groups, sd[name + ".weight"], sd[name + ".bias"], EPS)


def _conv(sd, name, x, stride=1, padding=1):
    return F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], stride=stride, padding=padding)


def resnet(sd, pre, x, groups):
    h = _conv(sd, pre + ".conv1", F.silu(_gn(sd, pre + ".norm1", x, groups)))
    h = _conv(sd, pre + ".conv2", F.silu(_gn(sd, pre + ".norm2", h, groups)))
    if pre + ".conv_shortcut.weight" in sd:
        x = _conv(sd, pre + ".conv_shortcut", x, padding=0)
    return x + h


def attention(sd, pre, x, groups):
    """Attention(heads = 1, dim_head = C, residual_connection = True, norm_num_groups) over the H W tokens."""
    B, C, H, W = x.shape
    t = _gn(sd, pre + ".group_norm", x, groups).reshape(B, C, H * W).transpose(1, 2)
    lin = lambda n: F.linear(t, sd[f"{pre}.{n}.weight"].reshape(C, C), sd[f"{pre}.{n}.bias"])      # noqa: E731
    q, k, v = lin("to_q"), lin("to_k"), lin("to_v")
    p = torch.softmax(q @ k.transpose(1, 2) * C ** -0.5, dim=-1)
    o = F.linear(p @ v, sd[f"{pre}.to_out.0.weight"].reshape(C, C), sd[f"{pre}.to_out.0.bias"])
    return x + o.transpose(1, 2).reshape(B, C, H, W)


def mid_block(sd, side, x, groups):
    x = resnet(sd, f"{side}.mid_block.resnets.0", x, groups)
    x = attention(sd, f"{side}.mid_block.attentions.0", x, groups)
    return resnet(sd, f"{side}.mid_block.resnets.1", x, groups)


def encode_moments(sd, cfg, x):
    """Encoder(double_z) + quant_conv -> [B, 2 latent, H / 2^(len(down) - 1), ...]."""
    g = cfg["groups"]
    x = _conv(sd, "encoder.conv_in", x)
    for i in range(len(cfg["down"])):
        for j in range(cfg["layers_down"]):
            x = resnet(sd, f"encoder.down_blocks.{i}.resnets.{j}", x, g)
        if i != len(cfg["down"]) - 1:                        # Downsample2D(padding = 0): pad right / bottom, stride 2
            x = _conv(sd, f"encoder.down_blocks.{i}.downsamplers.0.conv", F.pad(x, (0, 1, 0, 1)), stride=2, padding=0)
    x = mid_block(sd, "encoder", x, g)
    x = _conv(sd, "encoder.conv_out", F.silu(_gn(sd, "encoder.conv_norm_out", x, g)))
    return _conv(sd, "quant_conv", x, padding=0)


def condition_encoder(sd, cfg, masked_image):
    """MaskConditionEncoder.forward: every layer's output is stored BEFORE the ReLU, keyed by its shape."""
    out, x = {}, masked_image
    for l in range(len(condition_encoder_channels(cfg["up"][0], cfg["up"][-1]))):
        x = _conv(sd, f"decoder.condition_encoder.layers.{l}", x, stride=1 if l < 2 else 2)
        out[tuple(x.shape)] = x
        x = F.relu(x)
    return out


def decode(sd, cfg, z, image=None, mask=None):
    """post_quant_conv + MaskConditionDecoder.forward(z, image, mask)."""
    g = cfg["groups"]
    x = _conv(sd, "post_quant_conv", z, padding=0)
    x = _conv(sd, "decoder.conv_in", x)
    x = mid_block(sd, "decoder", x, g)
    cond = image is not None and mask is not None
    if cond:
        im_x = condition_encoder(sd, cfg, (1 - mask) * image)
    n = len(cfg["up"])
    for i in range(n):
        if cond:
            m = nearest_mask(mask, x.shape[-2], x.shape[-1])
            x = x * m + im_x[tuple(x.shape)] * (1 - m)
        for j in range(cfg["layers_up"] + 1):
            x = resnet(sd, f"decoder.up_blocks.{i}.resnets.{j}", x, g)
        if i != n - 1:
            x = _conv(sd, f"decoder.up_blocks.{i}.upsamplers.0.conv", F.interpolate(x, scale_factor=2.0, mode="nearest"))
    if cond:
        x = x * mask + im_x[tuple(x.shape)] * (1 - mask)
    return _conv(sd, "decoder.conv_out", F.silu(_gn(sd, "decoder.conv_norm_out", x, g)))


def rounded_weights(sd, dtype16, to=torch.float32):
    """Matrix weights as the HIP path stores them (rounded to its 16-bit format), vectors in full precision."""
    return {k: (v.to(dtype16).to(to) if v.dim() >= 2 else v.to(to)) for k, v in sd.items()}


def two_masks(B, H, W, fractional=False, seed=0):
    """One mask plane per batch item, different between items: a box per item (1 = repaint); `fractional`: soft values."""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(B, 1, H, W)
    for b in range(B):
        y0, x0 = (3 + 5 * b) % (H // 2), (2 + 7 * b) % (W // 2)
        m[b, :, y0:y0 + H // 2, x0:x0 + W // 3 + b] = 1.0
    if fractional:
        m = (m * 0.75 + 0.25 * torch.rand(B, 1, H, W, generator=g)).clamp(0, 1)
    return m
