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

`vae.VAENet` is the two-sided network already (structure lists, state-dict spec, packing, the encode plan, the decode plan's
walk); this subclass gives it the condition encoder (`_extra_convs`, `build_condition`) and the blends (`build_decode` hands
them to the base's walk as `stats`, `_norm` reads what they summed).  What is new in launches:
  * layers 2..4 of the condition encoder, 4x4 stride-2 pad-1 convs: `pp_conv4x4s2`, an MFMA implicit GEMM over the 16 taps
    (K = 16 Cin); the ReLU in front of each lives in its operand loader, so the pre-ReLU tensor is the only copy.  Layer 1 is a
    3x3 conv of the stock GEMM whose loader has no activation: ONE `pp_relu` launch writes its input (layer 0 -> layer 1);
  * `pp_masked_image_pack`: (1 - mask) * image, fp32 NCHW -> the 8-channel NHWC image `pp_conv3x3_direct` reads (layer 0);
  * `pp_mask_blend`: the blend, in place, which also sums the GroupNorm statistics of what it stored for the norm behind it
    (`pp_groupnorm_apply_acc`: no statistics launch).  The UNCONDITIONED plan takes the statistics of those five norms on the
    same route (`pp_mask_blend` with no condition tensor: it only sums), so a mask of ones reproduces it bit for bit.
"""
from typing import List, Optional, Tuple

import torch

from . import _lib as L
from .engine import Act, Builder, _conv_direct, _conv_igemm
from .vae import EPS, VAENet, VAERuntime, _pad_to

BLOCK_DOWN, BLOCK_UP = "DownEncoderBlock2D", "UpDecoderBlock2D"


def condition_channels(up: Tuple[int, ...]) -> List[int]:
    """Out channels of the five MaskConditionEncoder convs for `up_block_out_channels` = up."""
    b0, bl = up[0], up[-1]
    return [b0, 2 * b0, min(4 * b0, bl), bl, bl]


def conv4x4_igemm(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 4, 4] -> [Cout, 16 Cin], column (4 ky + kx) Cin + c: the layout pp_conv4x4s2 contracts."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


class AsymVAENet(VAENet):
    """Architecture + parameters of one AsymmetricAutoencoderKL: VAENet with the two sides set apart, the condition encoder
    and a `build_decode` that blends (with `img8` / `mask`) or only sums the blends' statistics (without)."""
    NAME = "AsymmetricAutoencoderKL"

    def __init__(self, in_channels: int = 3, out_channels: int = 3, latent_channels: int = 4,
                 down_block_out_channels=(128, 256, 512, 512), layers_per_down_block: int = 2,
                 up_block_out_channels=(192, 384, 768, 768), layers_per_up_block: int = 3, norm_num_groups: int = 32,
                 dtype: torch.dtype = torch.bfloat16):
        self._setup(in_channels, out_channels, latent_channels, down_block_out_channels, layers_per_down_block,
                    up_block_out_channels, layers_per_up_block, norm_num_groups, dtype)
        if norm_num_groups > 32:
            raise L.PPError("AsymmetricAutoencoderKL: norm_num_groups <= 32 supported")
        for name, boc in (("down_block_out_channels", self.down), ("up_block_out_channels", self.up)):
            if not boc or any(c % 64 or c % norm_num_groups for c in boc):
                raise L.PPError(f"AsymmetricAutoencoderKL: {name} must be multiples of 64 (MFMA K steps) and of "
                                f"norm_num_groups, got {boc}")
        self.cond_ch = condition_channels(self.up)

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
    def _cond_layers(self) -> List[Tuple[str, int, int, int]]:
        """(name, cin, cout, kernel) of the condition encoder's convs."""
        cin, out = self.cout, []
        for l, c in enumerate(self.cond_ch):
            out.append((f"decoder.condition_encoder.layers.{l}", cin, c, 3 if l < 2 else 4))
            cin = c
        return out

    def _extra_convs(self):
        """The condition encoder: layer 0 on the direct kernel (3 -> 8 padded channels in), layer 1 on the GEMM, 2..4 on
        pp_conv4x4s2."""
        pack = [lambda w: _pad_to(_conv_direct(w), 2, 8), _conv_igemm] + [conv4x4_igemm] * 3      # [Cout,Cin,3,3] -> [3,3,8,Cout]
        return [(name, (cout, cin, k, k), pack[l]) for l, (name, cin, cout, k) in enumerate(self._cond_layers())]

    # ---------------------------------------------------------------- plan pieces
    def _norm(self, pb: Builder, x: Act, name: str, silu: bool, acc: Optional[int] = None) -> Act:
        """With `acc`: GroupNorm(+SiLU) from statistics a pp_mask_blend launch summed (no statistics launch)."""
        if acc is None:
            return super()._norm(pb, x, name, silu)
        out = pb.new_act(x.B, x.H, x.W, x.C)
        pb.plan.add("groupnorm_apply", pb.lib.pp_groupnorm_apply_acc, x.ptr, x.C, None, 0, x.B, x.H * x.W, self.groups, EPS,
                    self.P[name + ".weight"], self.P[name + ".bias"], acc, int(silu), out.ptr, pb.dt)
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
        cond = img8 is not None
        nb = len(self.up) + 1                                         # blends: one per up block, one behind the last
        acc_bytes = z.B * self.groups * 2 * 8
        acc0 = pb.alloc(nb * acc_bytes)
        pb.plan.add("zero_u64", pb.lib.pp_zero_u64, acc0, nb * acc_bytes // 8)
        feats: List[Optional[Act]] = [None] * nb
        if cond:
            why = self.condition_mismatch()
            if why:
                raise L.PPError("AsymmetricAutoencoderKL: " + why)
            feats = list(reversed(self.build_condition(pb, img8)))     # in the order the blends read them

        def blend(x: Act, i: int) -> int:
            acc, c = acc0 + i * acc_bytes, feats[i]
            if cond and (c.B, c.H, c.W, c.C) != (x.B, x.H, x.W, x.C):
                raise L.PPError(f"AsymmetricAutoencoderKL: no condition-encoder output of shape {(x.B, x.C, x.H, x.W)}")
            pb.plan.add("mask_blend", pb.lib.pp_mask_blend, x.ptr, c.ptr if cond else None, mask or None,
                        x.ptr if cond else None, x.B, x.H, x.W, x.C, mask_hw[0], mask_hw[1], acc, self.groups, pb.dt)
            pb.taps.append((f"decoder.mask_blend.{i}", x, acc))      # in place: the tensor is the tap in front of it
            return acc

        return super().build_decode(pb, z, out_nchw, blend)


class AsymVAERuntime(VAERuntime):
    """One direction of one AsymVAENet: "encode", "decode" (unconditioned) or "decode_cond"."""

    def _build_decode(self, pb: Builder, lay: dict, B: int, H: int, W: int):
        if self.direction != "decode_cond":
            return super()._build_decode(pb, lay, B, H, W)
        lay["img8"] = Act(pb.arena.alloc(B * 64 * H * W * 8 * 2), B, 8 * H, 8 * W, 8)
        lay["mask"] = pb.arena.alloc(B * 64 * H * W * 4)
        return self.net.build_decode(pb, lay["x_in"], lay["img"], lay["img8"], lay["mask"], (8 * H, 8 * W))

    def run(self, x: torch.Tensor, image: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """VAERuntime.run; "decode_cond" first stages image [B | 1,c,8h,8w] and mask [B | 1,1,8h,8w] for the plan."""
        if self.direction == "decode_cond":
            B, _, H, W = x.shape
            self.ensure(B, H, W)
            stream = torch.cuda.current_stream().cuda_stream
            image = image.to(device=self.device, dtype=torch.float32).expand(B, image.shape[1], 8 * H, 8 * W).contiguous()
            mview = self.arena.view(self.lay["mask"], (B, 1, 8 * H, 8 * W), torch.float32)
            mview.copy_(mask.to(device=self.device, dtype=torch.float32).expand(B, 1, 8 * H, 8 * W))
            L.check(L.lib().pp_masked_image_pack(image.data_ptr(), self.lay["mask"], B, image.shape[1], 8 * H, 8 * W,
                                                 self.lay["img8"].ptr, L.dtype_code(self.net.dtype), stream),
                    "pp_masked_image_pack")
        return super().run(x)
