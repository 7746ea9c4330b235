"""AsymmetricAutoencoderKL (diffusers 0.27 `models/autoencoders/autoencoder_asym_kl.py`; `vae.py`: MaskConditionEncoder /
MaskConditionDecoder -- the asymmetric VQGAN of Zhu et al., arXiv:2306.04632) compiled to HIP launch plans.  The two
image-conditioned pipelines of the reference branch on it when they decode (pipeline_PowerPaint.py:1043-1051,
pipeline_PowerPaint_ControlNet.py:1317-1325).

The encoder is the SD-1.5 one (its own `down_block_out_channels` / `layers_per_down_block`); the decoder is wider / deeper
(`up_block_out_channels` / `layers_per_up_block`) and, given the original image and the mask, blends features of the image
back in outside the mask:

    cond = MaskConditionEncoder((1 - mask) * image)       five convs, every output kept BEFORE its ReLU
    in front of every up block, and behind the last:      sample = sample * m + cond[shape of sample] * (1 - m),
                                                          m = nearest(mask -> sample's h x w)

What is new against `vae.VAENet` (whose pieces -- resnet, mid block, the narrow ends -- this class reuses unchanged):
  * layers 2..4 of the condition encoder, 4x4 stride-2 pad-1 convs: `pp_conv4x4s2`, an MFMA implicit GEMM over the 16 taps
    (K = 16 Cin); the ReLU in front of each lives in its operand loader, so the pre-ReLU tensor is the only copy.  Layer 1 is a
    3x3 conv of the stock GEMM whose loader has no activation: ONE `pp_relu` launch writes its input (layer 0 -> layer 1);
  * `pp_masked_image_pack`: (1 - mask) * image, fp32 NCHW -> the 8-channel NHWC image `pp_conv3x3_direct` reads (layer 0);
  * `pp_mask_blend`: the blend, in place, which also sums the GroupNorm statistics of what it stored for the norm behind it
    (`pp_groupnorm_apply_acc`: no statistics launch).  The UNCONDITIONED plan takes the statistics of those five norms on the
    same route (`pp_mask_blend` with no condition tensor: it only sums), so a mask of ones reproduces it bit for bit.
"""
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib as L
from .engine import Act, Arena, Builder, ParamPack, Plan, _align, _conv_igemm
from .vae import EPS, _LEGACY, VAENet, _Image, _pad_to, _rot, _conv_direct

BLOCK_DOWN, BLOCK_UP = "DownEncoderBlock2D", "UpDecoderBlock2D"


def condition_channels(up: Tuple[int, ...]) -> List[int]:
    """Out channels of the five MaskConditionEncoder convs for `up_block_out_channels` = up."""
    b0, bl = up[0], up[-1]
    return [b0, 2 * b0, min(4 * b0, bl), bl, bl]


def conv4x4_igemm(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 4, 4] -> [Cout, 16 Cin], column (4 ky + kx) Cin + c: the layout pp_conv4x4s2 contracts."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


class AsymVAENet(VAENet):
    """Architecture + parameters of one AsymmetricAutoencoderKL; `build_decode` (with or without `img8` / `mask`) / `build_encode` append plans."""

    def __init__(self, in_channels: int = 3, out_channels: int = 3, latent_channels: int = 4,
                 down_block_out_channels=(128, 256, 512, 512), layers_per_down_block: int = 2,
                 up_block_out_channels=(192, 384, 768, 768), layers_per_up_block: int = 3, norm_num_groups: int = 32,
                 dtype: torch.dtype = torch.bfloat16):
        self.cin, self.cout, self.lat = in_channels, out_channels, latent_channels
        self.down, self.Ld = tuple(down_block_out_channels), layers_per_down_block
        self.up, self.Lu = tuple(up_block_out_channels), layers_per_up_block
        self.groups = norm_num_groups
        self.dtype = dtype
        L.dtype_code(dtype)
        if in_channels > 8 or out_channels > 4 or 2 * latent_channels > 8:
            raise L.PPError("AsymmetricAutoencoderKL: in_channels <= 8, out_channels <= 4, latent_channels <= 4 supported")
        if norm_num_groups > 32:
            raise L.PPError("AsymmetricAutoencoderKL: norm_num_groups <= 32 supported")
        for name, boc in (("down_block_out_channels", self.down), ("up_block_out_channels", self.up)):
            if not boc or any(c % 64 or c % norm_num_groups for c in boc):
                raise L.PPError(f"AsymmetricAutoencoderKL: {name} must be multiples of 64 (MFMA K steps) and of "
                                f"norm_num_groups, got {boc}")
        self.cond_ch = condition_channels(self.up)
        self.params: Optional[ParamPack] = None
        self.P: Dict[str, int] = {}

    def condition_mismatch(self) -> Optional[str]:
        """Why a CONDITIONED decode cannot run on this decoder (None: it can).  The sample in front of up block i must have the
        shape of one condition-encoder output -- diffusers looks it up by shape and dies with a KeyError in forward."""
        up = self.up
        if len(up) != 4:
            return f"up_block_out_channels {up}: the stride-16 condition encoder serves exactly four up blocks"
        rev = list(reversed(up))
        want = [rev[0], rev[0], rev[1], rev[2], rev[3]]                 # sample channels in front of blocks 0..3, behind the last
        have = list(reversed(self.cond_ch))                            # layers 4, 3, 2, 1, 0: H/8, H/4, H/2, H, H
        if want != have:
            return (f"up_block_out_channels {up}: the samples in front of the up blocks have {want} channels, the condition "
                    f"encoder's outputs {have} (needs up[1] == 2 up[0] and up[2] == min(4 up[0], up[3]))")
        return None

    # ---------------------------------------------------------------- structure
    def _resnets(self) -> List[Tuple[str, int, int]]:
        out, d = [], self.down
        for i, c in enumerate(d):
            for j in range(self.Ld):
                out.append((f"encoder.down_blocks.{i}.resnets.{j}", d[max(i - 1, 0)] if j == 0 else c, c))
        out += [(f"encoder.mid_block.resnets.{j}", d[-1], d[-1]) for j in range(2)]
        rev = list(reversed(self.up))
        out += [(f"decoder.mid_block.resnets.{j}", rev[0], rev[0]) for j in range(2)]
        for i, c in enumerate(rev):
            for j in range(self.Lu + 1):
                out.append((f"decoder.up_blocks.{i}.resnets.{j}", rev[max(i - 1, 0)] if j == 0 else c, c))
        return out

    def _samplers(self) -> List[Tuple[str, int]]:
        rev = list(reversed(self.up))
        return [(f"encoder.down_blocks.{i}.downsamplers.0.conv", self.down[i]) for i in range(len(self.down) - 1)] + \
               [(f"decoder.up_blocks.{i}.upsamplers.0.conv", rev[i]) for i in range(len(rev) - 1)]

    def _side(self, side: str) -> Tuple[int, ...]:
        return self.down if side == "encoder" else self.up

    def _cond_layers(self) -> List[Tuple[str, int, int, int]]:
        """(name, cin, cout, kernel) of the condition encoder's convs."""
        cin, out = self.cout, []
        for l, c in enumerate(self.cond_ch):
            out.append((f"decoder.condition_encoder.layers.{l}", cin, c, 3 if l < 2 else 4))
            cin = c
        return out

    def state_dict_spec(self) -> Dict[str, Tuple[int, ...]]:
        sp: Dict[str, Tuple[int, ...]] = {}

        def conv(name, cout, cin, k):
            sp[name + ".weight"], sp[name + ".bias"] = (cout, cin, k, k), (cout,)

        def vec(name, c):
            sp[name + ".weight"], sp[name + ".bias"] = (c,), (c,)

        conv("encoder.conv_in", self.down[0], self.cin, 3)
        conv("decoder.conv_in", self.up[-1], self.lat, 3)
        for pre, cin, cout in self._resnets():
            vec(pre + ".norm1", cin)
            conv(pre + ".conv1", cout, cin, 3)
            vec(pre + ".norm2", cout)
            conv(pre + ".conv2", cout, cout, 3)
            if cin != cout:
                conv(pre + ".conv_shortcut", cout, cin, 1)
        for pre, c in self._samplers():
            conv(pre, c, c, 3)
        for side in ("encoder", "decoder"):
            a, c = f"{side}.mid_block.attentions.0", self._side(side)[-1]
            vec(a + ".group_norm", c)
            for n in ("to_q", "to_k", "to_v", "to_out.0"):
                sp[f"{a}.{n}.weight"], sp[f"{a}.{n}.bias"] = (c, c), (c,)
        for name, cin, cout, k in self._cond_layers():
            conv(name, cout, cin, k)
        vec("encoder.conv_norm_out", self.down[-1])
        conv("encoder.conv_out", 2 * self.lat, self.down[-1], 3)
        vec("decoder.conv_norm_out", self.up[0])
        conv("decoder.conv_out", self.cout, self.up[0], 3)
        conv("quant_conv", 2 * self.lat, 2 * self.lat, 1)
        conv("post_quant_conv", self.lat, self.lat, 1)
        return sp

    # ---------------------------------------------------------------- parameters
    def load_state_dict(self, sd: Dict[str, torch.Tensor], device):
        sd = dict(sd)
        for k in list(sd):                                # pre-0.15 diffusers attention names
            for old, new in _LEGACY.items():
                if f".attentions.0.{old}." in k:
                    sd[k.replace(f".{old}.", f".{new}.")] = sd.pop(k)
        missing = [k for k in self.state_dict_spec() if k not in sd]
        if missing:
            raise L.PPError(f"AsymmetricAutoencoderKL state dict misses {len(missing)} keys, e.g. {missing[:3]}")
        pk = ParamPack()
        h16, f32 = self.dtype, torch.float32

        def W(k):
            return sd[k].float()

        def direct(w, cin_pad, cout_pad):                 # [Cout,Cin,3,3] -> [3,3,cin_pad,cout_pad]
            return _pad_to(_pad_to(_conv_direct(w), 2, cin_pad), 3, cout_pad)

        def centre(w, n):                                 # 1x1 as the centre tap of a 3x3, padded to n x n
            full = torch.zeros(w.shape[0], w.shape[1], 3, 3)
            full[:, :, 1, 1] = w[:, :, 0, 0]
            return direct(full, n, n)

        def vec(k):
            pk.add(k, W(k), f32)

        for pre, cin, cout in self._resnets():
            rot = _rot if pre.startswith("encoder") else (lambda t: t)      # the encoder runs rotated (vae.py)
            for nrm in ("norm1", "norm2"):
                vec(f"{pre}.{nrm}.weight")
                vec(f"{pre}.{nrm}.bias")
            for cv in ("conv1", "conv2"):
                pk.add(f"{pre}.{cv}.weight", _conv_igemm(rot(W(f"{pre}.{cv}.weight"))), h16)
                vec(f"{pre}.{cv}.bias")
            if cin != cout:
                pk.add(f"{pre}.conv_shortcut.weight", W(f"{pre}.conv_shortcut.weight").reshape(cout, cin), h16)
                vec(f"{pre}.conv_shortcut.bias")
        for pre, c in self._samplers():
            rot = _rot if pre.startswith("encoder") else (lambda t: t)
            pk.add(pre + ".weight", _conv_igemm(rot(W(pre + ".weight"))), h16)
            vec(pre + ".bias")
        for side in ("encoder", "decoder"):
            a, c = f"{side}.mid_block.attentions.0", self._side(side)[-1]
            vec(a + ".group_norm.weight")
            vec(a + ".group_norm.bias")
            for n in ("to_q", "to_k", "to_v", "to_out.0"):
                pk.add(f"{a}.{n}.weight", W(f"{a}.{n}.weight").reshape(c, c), h16)
                vec(f"{a}.{n}.bias")
            vec(f"{side}.conv_norm_out.weight")
            vec(f"{side}.conv_norm_out.bias")
        # the condition encoder: layer 0 on the direct kernel (3 -> 8 padded channels in), layer 1 on the GEMM, 2..4 on pp_conv4x4s2
        for l, (name, cin, cout, k) in enumerate(self._cond_layers()):
            w = W(name + ".weight")
            pk.add(name + ".weight", direct(w, 8, cout) if l == 0 else _conv_igemm(w) if l == 1 else conv4x4_igemm(w), h16)
            vec(name + ".bias")
        # the narrow ends, channel-padded
        pk.add("encoder.conv_in.weight", direct(_rot(W("encoder.conv_in.weight")), 8, self.down[0]), h16)
        vec("encoder.conv_in.bias")
        pk.add("encoder.conv_out.weight", direct(_rot(W("encoder.conv_out.weight")), self.down[-1], 8), h16)
        pk.add("encoder.conv_out.bias", _pad_to(W("encoder.conv_out.bias"), 0, 8), f32)
        pk.add("quant_conv.weight", centre(W("quant_conv.weight"), 8), h16)
        pk.add("quant_conv.bias", _pad_to(W("quant_conv.bias"), 0, 8), f32)
        pk.add("post_quant_conv.weight", centre(W("post_quant_conv.weight"), 8), h16)
        pk.add("post_quant_conv.bias", _pad_to(W("post_quant_conv.bias"), 0, 8), f32)
        pk.add("decoder.conv_in.weight", direct(W("decoder.conv_in.weight"), 8, self.up[-1]), h16)
        vec("decoder.conv_in.bias")
        pk.add("decoder.conv_out.weight", _conv_igemm(_pad_to(W("decoder.conv_out.weight"), 0, 4)), h16)
        pk.add("decoder.conv_out.bias", _pad_to(W("decoder.conv_out.bias"), 0, 4), f32)
        pk.to_device(device)
        self.params, self.P = pk, pk.ptr
        return self

    # ---------------------------------------------------------------- plan pieces
    def _norm_acc(self, pb: Builder, x: Act, name: str, silu: bool, acc: int) -> Act:
        """GroupNorm(+SiLU) from statistics a pp_mask_blend launch summed."""
        out = pb.new_act(x.B, x.H, x.W, x.C)
        pb.plan.add("groupnorm_apply", pb.lib.pp_groupnorm_apply_acc, x.ptr, x.C, None, 0, x.B, x.H * x.W, self.groups, EPS,
                    self.P[name + ".weight"], self.P[name + ".bias"], acc, int(silu), out.ptr, pb.dt)
        return out

    def _resnet_acc(self, pb: Builder, pre: str, x: Act, cout: int, acc: int) -> Act:
        """VAENet._resnet with norm1's statistics taken from `acc`."""
        P = self.P
        out = pb.new_act(x.B, x.H, x.W, cout)
        m = pb.mark()
        h = self._norm_acc(pb, x, f"{pre}.norm1", True, acc)
        h = pb.conv3x3(h, P[f"{pre}.conv1.weight"], cout, P[f"{pre}.conv1.bias"])
        h = pb.groupnorm(h, P[f"{pre}.norm2.weight"], P[f"{pre}.norm2.bias"], EPS, True, groups=self.groups)
        if x.C != cout:
            sc = pb.linear(x.ptr, x.rows, x.C, P[f"{pre}.conv_shortcut.weight"], cout, P[f"{pre}.conv_shortcut.bias"],
                           name="conv1x1")
        else:
            sc = x.ptr
        pb.conv3x3(h, P[f"{pre}.conv2.weight"], cout, P[f"{pre}.conv2.bias"], res1=sc, out=out)
        pb.release(m)
        pb.taps.append((pre, out))
        return out

    def _conv4x4(self, pb: Builder, x: Act, name: str, cout: int) -> Act:
        ho, wo = (x.H - 2) // 2 + 1, (x.W - 2) // 2 + 1
        out = pb.new_act(x.B, ho, wo, cout)
        pb.plan.add("conv4x4s2", pb.lib.pp_conv4x4s2, x.ptr, x.B, x.H, x.W, x.C, self.P[name + ".weight"],
                    self.P[name + ".bias"], cout, 1, out.ptr, pb.dt)
        pb.plan.count("conv4x4s2", 2.0 * out.rows * cout * 16 * x.C)       # all sixteen taps, nothing skipped
        pb.taps.append((name, out))
        return out

    def build_condition(self, pb: Builder, img8: Act) -> List[Act]:
        """img8: (1 - mask) * image padded to 8 channels [B,H,W,8] -> the five pre-ReLU outputs, layer 0 first."""
        P, ch = self.P, self.cond_ch
        pre = "decoder.condition_encoder.layers."
        l0 = self._direct(pb, img8, pre + "0", ch[0])
        l1 = pb.new_act(l0.B, l0.H, l0.W, ch[1])
        m = pb.mark()
        r0 = pb.new_act(l0.B, l0.H, l0.W, l0.C)
        pb.plan.add("relu", pb.lib.pp_relu, l0.ptr, r0.ptr, l0.rows * l0.C, pb.dt)
        pb.conv3x3(r0, P[pre + "1.weight"], ch[1], P[pre + "1.bias"], out=l1)
        pb.release(m)
        pb.taps.append((pre + "1", l1))
        l2 = self._conv4x4(pb, l1, pre + "2", ch[2])
        l3 = self._conv4x4(pb, l2, pre + "3", ch[3])
        l4 = self._conv4x4(pb, l3, pre + "4", ch[4])
        return [l0, l1, l2, l3, l4]

    # ---------------------------------------------------------------- plans
    def build_decode(self, pb: Builder, z: Act, out_nchw: int, img8: Optional[Act] = None, mask: int = 0,
                     mask_hw: Tuple[int, int] = (0, 0)):
        """z: latents padded to 8 channels [B,h,w,8] -> fp32 NCHW image [B,4,8h,8w] at `out_nchw` (channel 3 is 0).
        img8 / mask (device pointer of the fp32 [B][8h][8w] mask planes): the conditioned decode; without them nothing is
        blended and the condition encoder does not run."""
        P = self.P
        cond = img8 is not None
        rev = list(reversed(self.up))
        nb = len(rev) + 1                                             # blends: one per up block, one behind the last
        acc_bytes = z.B * self.groups * 2 * 8
        acc0 = pb.alloc(nb * acc_bytes)
        pb.plan.add("zero_u64", pb.lib.pp_zero_u64, acc0, nb * acc_bytes // 8)
        feats: List[Optional[Act]] = [None] * nb
        if cond:
            why = self.condition_mismatch()
            if why:
                raise L.PPError("AsymmetricAutoencoderKL: " + why)
            feats = list(reversed(self.build_condition(pb, img8)))     # in the order the blends read them
        x = self._direct(pb, z, "post_quant_conv", 8)
        x = self._direct(pb, x, "decoder.conv_in", self.up[-1])
        x = self._mid(pb, "decoder", x)

        def blend(x: Act, i: int) -> int:
            acc, c = acc0 + i * acc_bytes, feats[i]
            if cond and (c.B, c.H, c.W, c.C) != (x.B, x.H, x.W, x.C):
                raise L.PPError(f"AsymmetricAutoencoderKL: no condition-encoder output of shape {(x.B, x.C, x.H, x.W)}")
            pb.plan.add("mask_blend", pb.lib.pp_mask_blend, x.ptr, c.ptr if cond else None, mask or None,
                        x.ptr if cond else None, x.B, x.H, x.W, x.C, mask_hw[0], mask_hw[1], acc, self.groups, pb.dt)
            pb.taps.append((f"decoder.mask_blend.{i}", x, acc))      # in place: the tensor is the tap in front of it
            return acc

        for i, c in enumerate(rev):
            acc = blend(x, i)
            for j in range(self.Lu + 1):
                pre = f"decoder.up_blocks.{i}.resnets.{j}"
                x = self._resnet_acc(pb, pre, x, c, acc) if j == 0 else self._resnet(pb, pre, x, c)
            if i != len(rev) - 1:
                pre = f"decoder.up_blocks.{i}.upsamplers.0.conv"
                x = pb.conv3x3(x, P[pre + ".weight"], c, P[pre + ".bias"], up=True)
                pb.taps.append((pre, x))
        acc = blend(x, nb - 1)
        x = self._norm_acc(pb, x, "decoder.conv_norm_out", True, acc)
        pb.taps.append(("decoder.conv_norm_out", x))
        pb.plan.add("conv_out", pb.lib.pp_conv3x3_smallcout, x.ptr, x.B, x.H, x.W, x.C, P["decoder.conv_out.weight"],
                    P["decoder.conv_out.bias"], 4, out_nchw, pb.dt)
        pb.taps.append(("decoder.conv_out", _Image(out_nchw, x.B, 4, x.H, x.W)))
        return (x.B, 4, x.H, x.W)

    def build_encode(self, pb: Builder, img: Act) -> Act:
        """img: the 180-degree-rotated image padded to 8 channels [B,H,W,8] -> rotated moments [B,H/8,W/8,8]."""
        P, d = self.P, self.down
        x = self._direct(pb, img, "encoder.conv_in", d[0])
        for i, c in enumerate(d):
            for j in range(self.Ld):
                x = self._resnet(pb, f"encoder.down_blocks.{i}.resnets.{j}", x, c)
            if i != len(d) - 1:
                if x.H % 2 or x.W % 2:
                    raise L.PPError("AsymmetricAutoencoderKL.encode: image sides must be multiples of 2^(down blocks - 1)")
                pre = f"encoder.down_blocks.{i}.downsamplers.0.conv"
                x = pb.conv3x3(x, P[pre + ".weight"], c, P[pre + ".bias"], stride=2)
                pb.taps.append((pre, x))
        x = self._mid(pb, "encoder", x)
        x = pb.groupnorm(x, P["encoder.conv_norm_out.weight"], P["encoder.conv_norm_out.bias"], EPS, True,
                         groups=self.groups)
        pb.taps.append(("encoder.conv_norm_out", x))
        x = self._direct(pb, x, "encoder.conv_out", 8)
        return self._direct(pb, x, "quant_conv", 8)


class AsymVAERuntime:
    """Device state (arena + launch plan) of one direction of one AsymVAENet for one input shape.  direction: "encode",
    "decode" (unconditioned) or "decode_cond"."""

    def __init__(self, net: AsymVAENet, device, direction: str):
        self.net, self.device, self.direction = net, torch.device(device), direction
        self.key = None
        self.plan: Optional[Plan] = None
        self.arena: Optional[Arena] = None
        self.builds = 0                  # plans built so far (a new `image` / `mask` of a known shape builds nothing)

    def _build(self, arena: Arena, B: int, H: int, W: int):
        pb = Builder(arena, dtype=self.net.dtype)
        lay = {"x_in": Act(arena.alloc(B * H * W * 8 * 2), B, H, W, 8)}
        if self.direction == "encode":
            lay["moments"] = self.net.build_encode(pb, lay["x_in"])
            lay["taps"] = pb.taps
            return lay, pb.plan
        lay["img"] = arena.alloc(B * 4 * (8 * H) * (8 * W) * 4)
        if self.direction == "decode_cond":
            lay["img8"] = Act(arena.alloc(B * 64 * H * W * 8 * 2), B, 8 * H, 8 * W, 8)
            lay["mask"] = arena.alloc(B * 64 * H * W * 4)
            lay["shape"] = self.net.build_decode(pb, lay["x_in"], lay["img"], lay["img8"], lay["mask"], (8 * H, 8 * W))
        else:
            lay["shape"] = self.net.build_decode(pb, lay["x_in"], lay["img"])
        lay["taps"] = pb.taps
        return lay, pb.plan

    def ensure(self, B: int, H: int, W: int):
        if (B, H, W) == self.key:
            return
        dry = Arena()
        self._build(dry, B, H, W)
        self.arena = Arena(_align(dry.peak, 4096), self.device)      # zero-filled: the pad channels of x_in stay 0
        self.lay, self.plan = self._build(self.arena, B, H, W)
        self.key = (B, H, W)
        self.builds += 1

    def run(self, x: torch.Tensor, image: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """decode: latents [B,lat,h,w] (+ image [B,c,8h,8w], mask [B,1,8h,8w] for "decode_cond") -> fp32 [B,4,8h,8w] (a view of
        arena memory, valid until the next run); encode: ROTATED image [B,cin,H,W] -> rotated fp32 moments [B,8,H/8,W/8]."""
        B, Cc, H, W = x.shape
        self.ensure(B, H, W)
        stream = torch.cuda.current_stream().cuda_stream
        x = x.to(self.device)
        if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            x = x.float()
        x = x.contiguous()
        dt = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[x.dtype]
        code = L.dtype_code(self.net.dtype)
        xin = self.lay["x_in"]
        L.check(L.lib().pp_nchw_to_nhwc(x.data_ptr(), dt, B, Cc, H * W, 0, xin.ptr, 8, 0, code, stream), "pp_nchw_to_nhwc")
        if self.direction == "decode_cond":
            image = image.to(device=self.device, dtype=torch.float32).expand(B, image.shape[1], 8 * H, 8 * W).contiguous()
            mview = self.arena.view(self.lay["mask"], (B, 1, 8 * H, 8 * W), torch.float32)
            mview.copy_(mask.to(device=self.device, dtype=torch.float32).expand(B, 1, 8 * H, 8 * W))
            L.check(L.lib().pp_masked_image_pack(image.data_ptr(), self.lay["mask"], B, image.shape[1], 8 * H, 8 * W,
                                                 self.lay["img8"].ptr, code, stream), "pp_masked_image_pack")
        self.plan.run(stream)
        if self.direction != "encode":
            return self.arena.view(self.lay["img"], self.lay["shape"], torch.float32)
        m = self.lay["moments"]
        out = torch.empty(m.B, 8, m.H, m.W, dtype=torch.float32, device=self.device)
        L.check(L.lib().pp_nhwc_to_nchw(m.ptr, m.B, 8, m.H * m.W, out.data_ptr(), 0, code, stream), "pp_nhwc_to_nchw")
        return out
