"""AutoencoderTiny (TAESD) restated in plain torch.nn.functional, from the published form (diffusers
`models/autoencoders/autoencoder_tiny.py`; `vae.py`: EncoderTiny, DecoderTiny, AutoencoderTinyBlock).  The specification the HIP
path is tested against: it imports nothing from the product and the product imports nothing from it.  It runs in the dtype of
the state dict and the inputs (float64 in the tests).

    Block(x) = relu(conv4(relu(conv2(relu(conv0(x))))) + x)           3x3, pad 1, bias; keys conv.0|2|4.{weight,bias}
    encoder.layers: conv in -> 64 | n_0 Blocks | per further stage: conv stride 2 (no bias), n_i Blocks | conv 64 -> latent
    decoder.layers: conv latent -> 64 | ReLU | per stage: n_i Blocks, (all but the last) Upsample(nearest 2x), conv (no bias) |
                    conv 64 -> out
    encode(x) = encoder((x + 1) / 2)        decode(z) = 2 decoder(3 tanh(z / 3)) - 1

Every function takes `r`, applied to every tensor the launch plans STORE in the 16-bit format (the packed input, the output of
every conv but the last, the ReLU's output): the identity gives the pure model, `rounder(dtype)` the rounded variant.  The last
conv of either side is stored in fp32 and is not rounded.
"""
import torch
import torch.nn.functional as F

DEFAULT = dict(in_channels=3, out_channels=3, latent_channels=4, enc_blocks=(1, 3, 3, 3), dec_blocks=(3, 3, 3, 1))
# other block counts (taesdxl's are the defaults too; these exercise the counting): two stages, one and two blocks
SMALL = dict(in_channels=3, out_channels=3, latent_channels=4, enc_blocks=(1, 2), dec_blocks=(2, 1))
LATENT_MAGNITUDE, LATENT_SHIFT = 3, 0.5

# (B, H, W) probes of pp_conv3x3_c64, every mode (tests/test_taesd_kernels_gpu.py)
CONV_SHAPES = [(1, 8, 8), (2, 9, 13), (1, 1, 1), (1, 2, 70), (3, 17, 33)]
# a 320 x 320 item in mode 0: 10 x 40 = 400 tiles of 8 x 32 = 256 pixels -> with at most 256 workgroups (one per CU) the
# first 144 of them walk two tiles
CONV_BIG = (1, 320, 320)
DECODE_SHAPES = [(8, 12), (5, 7)]          # latents h x w
ENCODE_SHAPES = [(64, 96), (24, 40)]       # images H x W


def ident(t):
    return t


def rounder(dtype):
    return lambda t: t.to(dtype).to(t.dtype)


def layers(side, cfg):
    """(kind, index) of every entry of `<side>.layers`; kind in in | relu | block | down | up | conv_up | out."""
    out = ["in"]
    if side == "encoder":
        for i, n in enumerate(cfg["enc_blocks"]):
            out += (["down"] if i else []) + ["block"] * n
    else:
        out.append("relu")
        nb = cfg["dec_blocks"]
        for i, n in enumerate(nb):
            out += ["block"] * n + (["up", "conv_up"] if i != len(nb) - 1 else [])
    out.append("out")
    return list(zip(out, range(len(out))))


def spec(cfg):
    sp = {}
    for side, cin, cout in (("encoder", cfg["in_channels"], cfg["latent_channels"]),
                            ("decoder", cfg["latent_channels"], cfg["out_channels"])):
        for kind, i in layers(side, cfg):
            pre = f"{side}.layers.{i}"
            if kind == "in":
                sp[pre + ".weight"], sp[pre + ".bias"] = (64, cin, 3, 3), (64,)
            elif kind == "out":
                sp[pre + ".weight"], sp[pre + ".bias"] = (cout, 64, 3, 3), (cout,)
            elif kind == "block":
                for c in (0, 2, 4):
                    sp[f"{pre}.conv.{c}.weight"], sp[f"{pre}.conv.{c}.bias"] = (64, 64, 3, 3), (64,)
            elif kind in ("down", "conv_up"):
                sp[pre + ".weight"] = (64, 64, 3, 3)
    return sp


def rounded_weights(sd, dtype):
    """The parameters as the HIP path stores them, in float64: filters rounded to `dtype`, biases to fp32."""
    return {k: (v.float().to(dtype) if v.dim() == 4 else v.float()).double() for k, v in sd.items()}


def as_double(sd):
    return {k: v.double() for k, v in sd.items()}


def conv(sd, pre, x, stride=1, up=False):
    if up:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return F.conv2d(x, sd[pre + ".weight"], sd.get(pre + ".bias"), stride=stride, padding=1)


def block(sd, pre, x, r=ident):
    h = r(F.relu(conv(sd, pre + ".conv.0", x)))
    h = r(F.relu(conv(sd, pre + ".conv.2", h)))
    return r(F.relu(conv(sd, pre + ".conv.4", h) + x))


def run_layers(sd, side, cfg, x, r=ident):
    for kind, i in layers(side, cfg):
        pre = f"{side}.layers.{i}"
        if kind == "in":
            x = r(conv(sd, pre, x))
        elif kind == "relu":
            x = r(F.relu(x))
        elif kind == "block":
            x = block(sd, pre, x, r)
        elif kind == "down":
            x = r(conv(sd, pre, x, stride=2))
        elif kind == "conv_up":
            x = r(conv(sd, pre, x, up=True))
        elif kind == "out":
            x = conv(sd, pre, x)
    return x


def encode(sd, cfg, x, r=ident):
    return run_layers(sd, "encoder", cfg, r((x + 1) / 2), r)


def decode(sd, cfg, z, r=ident):
    return 2 * run_layers(sd, "decoder", cfg, r(3 * torch.tanh(z / 3)), r) - 1


def scale_latents(x):
    return (x / (2 * LATENT_MAGNITUDE) + LATENT_SHIFT).clamp(0, 1)


def unscale_latents(x):
    return (x - LATENT_SHIFT) * (2 * LATENT_MAGNITUDE)


def quantise(lat):
    """forward()'s round trip of the latents through a uint8 image."""
    return unscale_latents((scale_latents(lat) * 255).round().to(torch.uint8).to(lat.dtype) / 255.0)


def forward(sd, cfg, x, r=ident):
    return decode(sd, cfg, quantise(encode(sd, cfg, x, r)), r)


def pairwise_flags():
    """(bias, res, relu) rows covering every pair of values of every two flags."""
    return [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)]
