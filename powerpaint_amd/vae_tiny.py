"""AutoencoderTiny (TAESD; diffusers `models/autoencoders/autoencoder_tiny.py`, `vae.py`: EncoderTiny / DecoderTiny /
AutoencoderTinyBlock) compiled to HIP launch plans: a 64-channel conv net without norms or attention on the SD latent space,
the fast stand-in for AutoencoderKL on either side of the denoising loop and for previews inside it.

    Block(x) = relu(conv4(relu(conv2(relu(conv0(x))))) + x)          3x3, pad 1, with bias; keys conv.0|2|4.{weight,bias}
    encoder.layers:  0 conv in -> 64 | n_0 Blocks | per further stage: conv 64 -> 64 stride 2 (no bias), n_i Blocks | conv 64 -> latent
    decoder.layers:  0 conv latent -> 64 | 1 ReLU | per stage: n_i Blocks, then (all but the last) Upsample(nearest 2x) and
                     conv 64 -> 64 (no bias) | conv 64 -> out (bias)
    encode(x) = encoder((x + 1) / 2)                  decode(z) = 2 decoder(3 tanh(z / 3)) - 1

Launches (include/pp_hip.h), one per line of the lists above plus the boundary map:
  * `pp_taesd_pack`: (x + 1) / 2 or 3 tanh(z / 3), fp32 NCHW -> the 8-channel NHWC tensor; it WRITES the pad channels, so no
    plan relies on the arena's zero fill;
  * conv in (3 | 4 -> 64): `pp_conv3x3_direct`; the decoder's ReLU behind it: `pp_relu`;
  * every 64 -> 64 conv: `pp_conv3x3_c64` -- mode 0 with ReLU (and the residual in a Block's third conv), mode 1 for the
    stride-2 convs, mode 2 for Upsample + conv as ONE launch;
  * conv out (64 -> 3 | 4): `pp_conv3x3_smallcout` on weights padded to 4 outputs, fp32 NCHW out.
The decoder's `2 y - 1` is folded into its last conv at pack time (w' = 2 w is exact in either 16-bit format, b' = 2 b - 1 in
fp32).  The encoder's `(x + 1) / 2` cannot be folded the same way: the zero padding of conv in lives in the scaled domain.

Taps.  Every launch records (name, Act | _Image) of its output in `Builder.taps`, in plan order: "pack", then the state-dict
prefix of the conv (`decoder.layers.2.conv.0`, `decoder.layers.6`, ...; `decoder.layers.1` for the ReLU).  Nothing is released,
so every tap keeps its bytes until the plan ends.
"""
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib as L
from .engine import Act, Arena, Builder, ParamPack, _conv_direct, _conv_igemm
from .vae import PlanRuntime, _Image, _pad_to

WIDTH = 64      # the only channel count pp_conv3x3_c64 is built for


class TinyVAENet:
    """Architecture + parameters of one AutoencoderTiny; `build_decode` / `build_encode` append launch plans."""

    def __init__(self, in_channels: int = 3, out_channels: int = 3, latent_channels: int = 4,
                 num_encoder_blocks=(1, 3, 3, 3), num_decoder_blocks=(3, 3, 3, 1), dtype: torch.dtype = torch.bfloat16):
        self.cin, self.cout, self.lat = in_channels, out_channels, latent_channels
        self.enc_blocks, self.dec_blocks = tuple(num_encoder_blocks), tuple(num_decoder_blocks)
        self.dtype = dtype
        L.dtype_code(dtype)
        if not 0 < in_channels <= 8 or not 0 < out_channels <= 4:
            raise L.PPError(f"AutoencoderTiny: in_channels <= 8 and out_channels <= 4 supported, got {in_channels}, {out_channels}")
        if not 0 < latent_channels <= 4:
            raise L.PPError(f"AutoencoderTiny: latent_channels <= 4 supported, got latent_channels={latent_channels}")
        for name, nb in (("num_encoder_blocks", self.enc_blocks), ("num_decoder_blocks", self.dec_blocks)):
            if not nb or any(not isinstance(n, int) or n <= 0 for n in nb):
                raise L.PPError(f"AutoencoderTiny: {name} must be a tuple of positive ints, got {name}={nb}")
        self.params: Optional[ParamPack] = None
        self.P: Dict[str, int] = {}

    # ---------------------------------------------------------------- structure
    def _layers(self, side: str) -> List[Tuple[str, str]]:
        """(kind, state-dict prefix) of every entry of `<side>.layers`: kind in {in, relu, block, down, up, conv_up, out}
        ("up" is the parameterless Upsample, "conv_up" the conv behind it)."""
        out: List[Tuple[str, str]] = []

        def add(kind):
            out.append((kind, f"{side}.layers.{len(out)}"))

        add("in")
        if side == "encoder":
            for i, n in enumerate(self.enc_blocks):
                if i:
                    add("down")
                for _ in range(n):
                    add("block")
        else:
            add("relu")
            for i, n in enumerate(self.dec_blocks):
                for _ in range(n):
                    add("block")
                if i != len(self.dec_blocks) - 1:
                    add("up")
                    add("conv_up")
        add("out")
        return out

    def state_dict_spec(self) -> Dict[str, Tuple[int, ...]]:
        sp: Dict[str, Tuple[int, ...]] = {}
        for side, cin, cout in (("encoder", self.cin, self.lat), ("decoder", self.lat, self.cout)):
            for kind, pre in self._layers(side):
                if kind == "in":
                    sp[pre + ".weight"], sp[pre + ".bias"] = (WIDTH, cin, 3, 3), (WIDTH,)
                elif kind == "out":
                    sp[pre + ".weight"], sp[pre + ".bias"] = (cout, WIDTH, 3, 3), (cout,)
                elif kind == "block":
                    for c in (0, 2, 4):
                        sp[f"{pre}.conv.{c}.weight"], sp[f"{pre}.conv.{c}.bias"] = (WIDTH, WIDTH, 3, 3), (WIDTH,)
                elif kind in ("down", "conv_up"):
                    sp[pre + ".weight"] = (WIDTH, WIDTH, 3, 3)
        return sp

    def synthetic_state_dict(self, device="cpu", seed: int = 0) -> Dict[str, torch.Tensor]:
        """Random-init weights (no checkpoints offline): He-scaled normal filters (the net has no norms: ReLU halves the second
        moment, gain 2 keeps the activations' scale through ~40 convs), small biases."""
        g = torch.Generator(device=device).manual_seed(seed)
        sd = {}
        for k, shp in self.state_dict_spec().items():
            if len(shp) == 1:
                sd[k] = 0.05 * torch.randn(shp, generator=g, device=device)
            else:
                fan_in = shp[1] * shp[2] * shp[3]
                gain = 1.0 if ".conv.4." in k else 2.0       # (the residual branch adds to the skip: keep the sum bounded)
                sd[k] = torch.randn(shp, generator=g, device=device) * (gain / fan_in) ** 0.5
        return sd

    # ---------------------------------------------------------------- parameters
    def load_state_dict(self, sd: Dict[str, torch.Tensor], device):
        missing = [k for k in self.state_dict_spec() if k not in sd]
        if missing:
            raise L.PPError(f"AutoencoderTiny state dict misses {len(missing)} keys, e.g. {missing[:3]}")
        pk = ParamPack()
        h16, f32 = self.dtype, torch.float32

        def W(k):
            return sd[k].float()

        for side in ("encoder", "decoder"):
            for kind, pre in self._layers(side):
                if kind == "in":                             # [Cout,Cin,3,3] -> [3,3,8,Cout]
                    pk.add(pre + ".weight", _pad_to(_conv_direct(W(pre + ".weight")), 2, 8), h16)
                    pk.add(pre + ".bias", W(pre + ".bias"), f32)
                elif kind == "out":
                    w, b = W(pre + ".weight"), W(pre + ".bias")
                    if side == "decoder":                    # 2 y - 1 of the image, folded
                        w, b = 2.0 * w, 2.0 * b - 1.0
                    pk.add(pre + ".weight", _conv_igemm(_pad_to(w, 0, 4)), h16)
                    pk.add(pre + ".bias", _pad_to(b, 0, 4), f32)
                elif kind == "block":
                    for c in (0, 2, 4):
                        pk.add(f"{pre}.conv.{c}.weight", _conv_igemm(W(f"{pre}.conv.{c}.weight")), h16)
                        pk.add(f"{pre}.conv.{c}.bias", W(f"{pre}.conv.{c}.bias"), f32)
                elif kind in ("down", "conv_up"):
                    pk.add(pre + ".weight", _conv_igemm(W(pre + ".weight")), h16)
        pk.to_device(device)
        self.params, self.P = pk, pk.ptr
        return self

    # ---------------------------------------------------------------- plan pieces
    def _c64(self, pb: Builder, x: Act, name: str, mode: int, relu: bool, bias: bool, res: Optional[Act] = None) -> Act:
        ho, wo = ((x.H, x.W), ((x.H - 1) // 2 + 1, (x.W - 1) // 2 + 1), (2 * x.H, 2 * x.W))[mode]
        out = pb.new_act(x.B, ho, wo, WIDTH)
        pb.plan.add("conv3x3_c64", pb.lib.pp_conv3x3_c64, x.ptr, x.B, x.H, x.W, self.P[name + ".weight"],
                    self.P[name + ".bias"] if bias else None, res.ptr if res is not None else None, mode, int(relu),
                    out.ptr, pb.dt)
        pb.plan.count("conv3x3_c64", 2.0 * out.rows * WIDTH * 9 * WIDTH)
        pb.taps.append((name, out))
        return out

    def _block(self, pb: Builder, pre: str, x: Act) -> Act:
        h = self._c64(pb, x, pre + ".conv.0", 0, True, True)
        h = self._c64(pb, h, pre + ".conv.2", 0, True, True)
        return self._c64(pb, h, pre + ".conv.4", 0, True, True, res=x)

    def _pack(self, pb: Builder, src: int, B: int, c: int, H: int, W: int, mode: int) -> Act:
        x = pb.new_act(B, H, W, 8)
        pb.plan.add("taesd_pack", pb.lib.pp_taesd_pack, src, L.PP_DT_F32, B, c, H, W, mode, x.ptr, pb.dt)
        pb.taps.append(("pack", x))
        return x

    def _run_layers(self, pb: Builder, side: str, x: Act, out_nchw: int):
        for kind, pre in self._layers(side):
            if kind == "in":
                out = pb.new_act(x.B, x.H, x.W, WIDTH)
                pb.plan.add("conv3x3_direct", pb.lib.pp_conv3x3_direct, x.ptr, x.B, x.H, x.W, x.C, self.P[pre + ".weight"],
                            self.P[pre + ".bias"], WIDTH, 1, 0, None, out.ptr, pb.dt)
                pb.taps.append((pre, out))
                x = out
            elif kind == "relu":
                out = pb.new_act(x.B, x.H, x.W, x.C)
                pb.plan.add("relu", pb.lib.pp_relu, x.ptr, out.ptr, x.rows * x.C, pb.dt)
                pb.taps.append((pre, out))
                x = out
            elif kind == "block":
                x = self._block(pb, pre, x)
            elif kind == "down":
                x = self._c64(pb, x, pre, 1, False, False)
            elif kind == "conv_up":                          # with the Upsample in front of it
                x = self._c64(pb, x, pre, 2, False, False)
            elif kind == "out":
                pb.plan.add("conv_out", pb.lib.pp_conv3x3_smallcout, x.ptr, x.B, x.H, x.W, x.C, self.P[pre + ".weight"],
                            self.P[pre + ".bias"], 4, out_nchw, pb.dt)
                pb.taps.append((pre, _Image(out_nchw, x.B, 4, x.H, x.W)))
        return (x.B, 4, x.H, x.W)

    # ---------------------------------------------------------------- plans
    def build_decode(self, pb: Builder, src: int, B: int, h: int, w: int, out_nchw: int):
        """src: fp32 NCHW latents [B,lat,h,w] -> fp32 NCHW image [B,4,s h,s w] at `out_nchw` (channels >= out_channels are
        padding).  Returns the image's shape."""
        return self._run_layers(pb, "decoder", self._pack(pb, src, B, self.lat, h, w, 1), out_nchw)

    def build_encode(self, pb: Builder, src: int, B: int, H: int, W: int, out_nchw: int):
        """src: fp32 NCHW image [B,cin,H,W] in [-1, 1] -> fp32 NCHW latents [B,4,h,w] at `out_nchw` (channels >=
        latent_channels are padding).  Returns the latents' shape."""
        return self._run_layers(pb, "encoder", self._pack(pb, src, B, self.cin, H, W, 0), out_nchw)

    def out_hw(self, direction: str, H: int, W: int) -> Tuple[int, int]:
        if direction == "decode":
            s = 2 ** (len(self.dec_blocks) - 1)
            return s * H, s * W
        for _ in range(len(self.enc_blocks) - 1):
            H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        return H, W


class TinyVAERuntime(PlanRuntime):
    """One direction, "decode" or "encode", of one TinyVAENet."""

    def _build(self, arena: Arena, B: int, H: int, W: int):
        net = self.net
        pb = Builder(arena, dtype=net.dtype)
        c = net.lat if self.direction == "decode" else net.cin
        ho, wo = net.out_hw(self.direction, H, W)
        lay = {"src": arena.alloc(B * c * H * W * 4), "src_shape": (B, c, H, W), "out": arena.alloc(B * 4 * ho * wo * 4)}
        build = net.build_decode if self.direction == "decode" else net.build_encode
        lay["shape"] = build(pb, lay["src"], B, H, W, lay["out"])
        lay["taps"] = pb.taps
        return lay, pb.plan

    def run(self, x: torch.Tensor) -> torch.Tensor:
        """decode: latents [B,lat,h,w] -> fp32 [B,4,s h,s w]; encode: image [B,cin,H,W] -> fp32 latents [B,4,h,w].  Both are
        views of arena memory, valid until the next run."""
        B, Cc, H, W = x.shape
        self.ensure(B, H, W)
        stream = torch.cuda.current_stream().cuda_stream
        self.arena.view(self.lay["src"], self.lay["src_shape"], torch.float32).copy_(x)
        self.plan.run(stream)
        return self.arena.view(self.lay["out"], self.lay["shape"], torch.float32)
