"""AutoencoderKL (the SD-1.5 VAE) compiled to HIP launch plans -- SURVEY.md §8f-1, the step either side of the loop:
    /root/reference/powerpaint/pipelines/pipeline_PowerPaint.py:657-669   vae.encode(image).latent_dist.sample(generator)
    /root/reference/powerpaint/pipelines/pipeline_PowerPaint.py:1051      vae.decode(latents / scaling_factor)[0]
The class is diffusers' (autoencoder_kl.py, vae.py: Encoder / Decoder / UNetMidBlock2D / DownEncoderBlock2D /
UpDecoderBlock2D); the state-dict key names below are diffusers' so `diffusion_pytorch_model.safetensors` of the
checkpoint's `vae/` folder loads unchanged (the pre-0.15 attention names query / key / value / proj_attn are mapped).

Everything runs on the kernels of the UNet path (include/pp_hip.h):
  * 3x3 convs with 64-multiple channel counts: the MFMA implicit GEMM (`pp_gemm_bf16`, PP_X_CONV3X3), nearest x2
    upsampling and stride 2 fused into its loader; GroupNorm(+SiLU): `pp_groupnorm_stats/apply` (eps 1e-6);
  * the 3 / 4 / 8-channel ends (conv_in, conv_out, quant_conv, post_quant_conv): `pp_conv3x3_direct` /
    `pp_conv3x3_smallcout` on tensors padded to 8 (4) channels -- a 1x1 conv is a 3x3 whose only non-zero tap is the
    centre;
  * the mid-block attention (ONE head of dim 512 over H*W tokens, outside `pp_attention_fwd`'s head dims): per image
    S = Q K^T as a GEMM with fp32 output, `pp_softmax_rows`, O = P V as a GEMM against V^T (`pp_transpose_v`).

Encoder trick: Downsample2D(padding=0) pads right / bottom only (F.pad((0,1,0,1)) + stride-2 conv).  With the image
rotated by 180 degrees that is exactly a symmetric pad-1 stride-2 conv with 180-degree-rotated filters (for even
sizes), and every other layer commutes with the rotation once its 3x3 filters are rotated too.  So the encoder runs
"upside down" on the stock conv kernel -- rotated input, all encoder filters rotated at pack time, moments rotated
back -- instead of growing a new padding mode in the hot GEMM loader.  tests/test_vae.py checks the identity on CPU.

Arena zero fill.  The runtimes (`PlanRuntime.ensure`, shared with vae_asym.py and vae_tiny.py, whose plans rely on nothing:
pp_taesd_pack writes the pad channels) allocate their arena zero-filled, and ONE buffer relies on it: the pad channels of `x_in`
(channels [latent_channels, 8) of the latents, [in_channels, 8) of the image), which pp_nchw_to_nhwc never writes and
pp_conv3x3_direct multiplies by the zero-padded rows of its weights.  Everything else a plan reads it has written before:
the GroupNorm and split-K workspaces, K with its pad rows (S's pad columns, the only values computed from rows the K GEMM
did not write, are never read: the softmax runs over n columns), the pad columns of P (pp_softmax_rows writes zeros) and of
V^T (pp_transpose_v writes zeros), the four channels of the image buffer (conv_out's weights and bias are padded to 4 with
zeros).  vae_asym.py adds nothing to the list: pp_masked_image_pack writes all 8 channels of `img8`, the runtime copies the
whole mask planes, pp_zero_u64 clears the blend accumulators.  tests/test_vae_blocks_gpu.py runs every plan on an arena filled
with NaNs outside its input buffers and requires the same bits.

Taps.  Every build function records (name, Act) of each block output in `Builder.taps`, in plan order, under the state-dict
prefix of the block (`decoder.mask_blend.<i>` with the accumulator pointer as a third entry for the blends; the decoder's image
as an `_Image`); the runtimes keep the list of their build on the real arena as `lay["taps"]`.  No mark / release is taken at
the top level of a build function, so every tap keeps its bytes until the plan ends.
"""
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import torch

from . import _lib as L
from .engine import Act, Arena, Builder, ParamPack, Plan, _align, _conv_direct, _conv_igemm

EPS = 1e-6
_LEGACY = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}


def _pad_to(t: torch.Tensor, dim: int, n: int) -> torch.Tensor:
    if t.shape[dim] == n:
        return t
    shp = list(t.shape)
    shp[dim] = n - t.shape[dim]
    return torch.cat([t, t.new_zeros(shp)], dim)


def _rot(w: torch.Tensor) -> torch.Tensor:
    return w.flip(2, 3)


class _Image(NamedTuple):
    """The decoder's output buffer as a tap: fp32 NCHW [B][C][H][W] (every other tap is an NHWC Act of the 16-bit format)."""
    ptr: int
    B: int
    C: int
    H: int
    W: int

    @property
    def nbytes(self) -> int:
        return self.B * self.C * self.H * self.W * 4


class VAENet:
    """Architecture + parameters of one AutoencoderKL: an encoder of widths `down` with `Ld` resnets per block, a decoder of
    widths `up` with `Lu` + 1, stored as `dtype`; `build_decode` / `build_encode` append launch plans.  AutoencoderKL itself is
    the symmetric bf16 case; vae_asym.AsymVAENet sets the two sides apart and adds the mask-conditioned decode."""
    NAME = "AutoencoderKL"

    def __init__(self, in_channels: int = 3, out_channels: int = 3, latent_channels: int = 4,
                 block_out_channels=(128, 256, 512, 512), layers_per_block: int = 2, norm_num_groups: int = 32):
        self._setup(in_channels, out_channels, latent_channels, block_out_channels, layers_per_block, block_out_channels,
                    layers_per_block, norm_num_groups, torch.bfloat16)
        if any(c % 64 or c % norm_num_groups for c in self.up):
            raise L.PPError("AutoencoderKL: block_out_channels must be multiples of 64 (MFMA K steps) and of the groups")

    def _setup(self, in_channels, out_channels, latent_channels, down, layers_down, up, layers_up, groups, dtype):
        """The fields of either constructor, and the one check they share (the 8 / 4-channel ends)."""
        self.cin, self.cout, self.lat = in_channels, out_channels, latent_channels
        self.down, self.Ld = tuple(down), layers_down
        self.up, self.Lu = tuple(up), layers_up
        self.groups = groups
        self.dtype = dtype
        L.dtype_code(dtype)
        if in_channels > 8 or out_channels > 4 or 2 * latent_channels > 8:
            raise L.PPError(f"{self.NAME}: in_channels <= 8, out_channels <= 4, latent_channels <= 4 supported")
        self.params: Optional[ParamPack] = None
        self.P: Dict[str, int] = {}

    # ---------------------------------------------------------------- structure
    def _resnets(self) -> List[Tuple[str, int, int]]:
        """(prefix, cin, cout) of every ResnetBlock2D, encoder then decoder, in diffusers order."""
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

    def _extra_convs(self) -> List[Tuple[str, Tuple[int, ...], Callable]]:
        """(name, weight shape, fp32 weight -> packed matrix) of the convs a subclass adds to the state dict.  They sit in the
        spec and in the pack behind the attentions and in front of the narrow ends (the pack order fixes every offset)."""
        return []

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
        for side, c in (("encoder", self.down[-1]), ("decoder", self.up[-1])):
            a = f"{side}.mid_block.attentions.0"
            vec(a + ".group_norm", c)
            for n in ("to_q", "to_k", "to_v", "to_out.0"):
                sp[f"{a}.{n}.weight"], sp[f"{a}.{n}.bias"] = (c, c), (c,)
        for name, shape, _ in self._extra_convs():
            sp[name + ".weight"], sp[name + ".bias"] = shape, shape[:1]
        vec("encoder.conv_norm_out", self.down[-1])
        conv("encoder.conv_out", 2 * self.lat, self.down[-1], 3)
        vec("decoder.conv_norm_out", self.up[0])
        conv("decoder.conv_out", self.cout, self.up[0], 3)
        conv("quant_conv", 2 * self.lat, 2 * self.lat, 1)
        conv("post_quant_conv", self.lat, self.lat, 1)
        return sp

    def synthetic_state_dict(self, device="cpu", seed: int = 0) -> Dict[str, torch.Tensor]:
        """Random-init weights (no checkpoints offline): fan-in scaled normal matrices, (1 + noise, noise) norm affine,
        small biases -- nothing left at a value that would hide a wiring mistake."""
        g = torch.Generator(device=device).manual_seed(seed)
        sd = {}
        for k, shp in self.state_dict_spec().items():
            if len(shp) == 1:
                base = 1.0 if (k.endswith(".weight") and ("norm" in k)) else 0.0
                sd[k] = base + 0.05 * torch.randn(shp, generator=g, device=device)
            else:
                fan_in = 1
                for d in shp[1:]:
                    fan_in *= d
                sd[k] = torch.randn(shp, generator=g, device=device) * (1.0 / fan_in) ** 0.5
        return sd

    # ---------------------------------------------------------------- parameters
    def load_state_dict(self, sd: Dict[str, torch.Tensor], device):
        sd = dict(sd)
        for k in list(sd):                                # pre-0.15 diffusers attention names; 1x1-conv shaped linears
            for old, new in _LEGACY.items():
                if f".attentions.0.{old}." in k:
                    sd[k.replace(f".{old}.", f".{new}.")] = sd.pop(k)
        missing = [k for k in self.state_dict_spec() if k not in sd]
        if missing:
            raise L.PPError(f"{self.NAME} state dict misses {len(missing)} keys, e.g. {missing[:3]}")
        pk = ParamPack()
        h16, f32 = self.dtype, torch.float32

        def W(k):
            return sd[k].float()

        def direct(w, cin_pad, cout_pad):                 # [Cout,Cin,3,3] -> [3,3,cin_pad,cout_pad]
            return _pad_to(_pad_to(_conv_direct(w), 2, cin_pad), 3, cout_pad)

        def centre(w, n):                                 # 1x1 [Cout,Cin,1,1] as the centre tap of a 3x3, padded to n x n
            full = torch.zeros(w.shape[0], w.shape[1], 3, 3)
            full[:, :, 1, 1] = w[:, :, 0, 0]
            return direct(full, n, n)

        def vec(k):
            pk.add(k, W(k), f32)

        for pre, cin, cout in self._resnets():
            rot = _rot if pre.startswith("encoder") else (lambda t: t)      # the encoder runs rotated (module docstring)
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
        for side, c in (("encoder", self.down[-1]), ("decoder", self.up[-1])):
            a = f"{side}.mid_block.attentions.0"
            vec(a + ".group_norm.weight")
            vec(a + ".group_norm.bias")
            for n in ("to_q", "to_k", "to_v", "to_out.0"):
                pk.add(f"{a}.{n}.weight", W(f"{a}.{n}.weight").reshape(c, c), h16)
                vec(f"{a}.{n}.bias")
            vec(f"{side}.conv_norm_out.weight")
            vec(f"{side}.conv_norm_out.bias")
        for name, _, pack in self._extra_convs():
            pk.add(name + ".weight", pack(W(name + ".weight")), h16)
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
    def _direct(self, pb: Builder, x: Act, name: str, cout: int) -> Act:
        out = pb.new_act(x.B, x.H, x.W, cout)
        pb.plan.add("conv3x3_direct", pb.lib.pp_conv3x3_direct, x.ptr, x.B, x.H, x.W, x.C, self.P[name + ".weight"],
                    self.P[name + ".bias"], cout, 1, 0, None, out.ptr, pb.dt)
        pb.taps.append((name, out))
        return out

    def _norm(self, pb: Builder, x: Act, name: str, silu: bool, acc: Optional[int] = None) -> Act:
        """GroupNorm(+SiLU) `name` of x.  acc: an accumulator that already holds x's statistics; only the plans of vae_asym.py,
        which overrides this, have one."""
        assert acc is None
        return pb.groupnorm(x, self.P[name + ".weight"], self.P[name + ".bias"], EPS, silu, groups=self.groups)

    def _resnet(self, pb: Builder, pre: str, x: Act, cout: int, acc: Optional[int] = None) -> Act:
        """acc: norm1 takes its statistics from there (`_norm`)."""
        P = self.P
        out = pb.new_act(x.B, x.H, x.W, cout)
        m = pb.mark()
        h = self._norm(pb, x, f"{pre}.norm1", True, acc)
        h = pb.conv3x3(h, P[f"{pre}.conv1.weight"], cout, P[f"{pre}.conv1.bias"])
        h = self._norm(pb, h, f"{pre}.norm2", True)
        if x.C != cout:
            sc = pb.linear(x.ptr, x.rows, x.C, P[f"{pre}.conv_shortcut.weight"], cout, P[f"{pre}.conv_shortcut.bias"],
                           name="conv1x1")
        else:
            sc = x.ptr
        pb.conv3x3(h, P[f"{pre}.conv2.weight"], cout, P[f"{pre}.conv2.bias"], res1=sc, out=out)
        pb.release(m)
        pb.taps.append((pre, out))
        return out

    def _attention(self, pb: Builder, pre: str, x: Act) -> Act:
        """Single-head attention over the H*W tokens with residual (diffusers Attention(residual_connection=True))."""
        P = self.P
        Cc, n, B = x.C, x.H * x.W, x.B
        # The keys are padded to the GEMMs' K step, npad = n rounded up to 64: S = Q K^T is [n][npad] (its pad columns multiply
        # whatever rows follow K -- the next image's keys, or the pad rows allocated behind the last -- and are never read:
        # the softmax runs over n columns), P is [n][npad] with pad columns the softmax WRITES as zeros (the arena is reused),
        # V^T is [C][npad] with pad columns pp_transpose_v zeroes.  n % 64 == 0: npad = n, the plan that always was.
        npad = _align(n, 64)
        out = pb.new_act(B, x.H, x.W, Cc)
        m = pb.mark()
        h = self._norm(pb, x, f"{pre}.group_norm", False)
        q = pb.linear(h.ptr, x.rows, Cc, P[f"{pre}.to_q.weight"], Cc, P[f"{pre}.to_q.bias"], name="linear")
        k = pb.linear(h.ptr, x.rows, Cc, P[f"{pre}.to_k.weight"], Cc, P[f"{pre}.to_k.bias"],
                      out=pb.alloc((x.rows + npad - n) * Cc * 2), name="linear")
        v = pb.linear(h.ptr, x.rows, Cc, P[f"{pre}.to_v.weight"], Cc, P[f"{pre}.to_v.bias"], name="linear")
        vt = pb.alloc(B * Cc * npad * 2)
        pb.plan.add("transpose_v", pb.lib.pp_transpose_v, v, Cc, B, n, Cc, vt, npad)
        o = pb.alloc(x.rows * Cc * 2)
        s = pb.alloc(n * npad * 4)
        p = pb.alloc(n * npad * 2)
        for b in range(B):
            tok = b * n * Cc * 2
            pb.linear(q + tok, n, Cc, k + tok, npad, out=s, ldo=npad, out_f32=True, name="attn_qk")
            pb.plan.add("softmax_rows", pb.lib.pp_softmax_rows, s, npad, n, n, float(Cc) ** -0.5, p, npad, pb.dt)
            pb.linear(p, n, npad, vt + b * Cc * npad * 2, Cc, out=o + tok, ldo=Cc, name="attn_pv")
        pb.linear(o, x.rows, Cc, P[f"{pre}.to_out.0.weight"], Cc, P[f"{pre}.to_out.0.bias"], res1=x.ptr, out=out.ptr,
                  name="linear")
        pb.release(m)
        pb.taps.append((pre, out))
        return out

    def _mid(self, pb: Builder, side: str, x: Act) -> Act:
        x = self._resnet(pb, f"{side}.mid_block.resnets.0", x, x.C)
        x = self._attention(pb, f"{side}.mid_block.attentions.0", x)
        return self._resnet(pb, f"{side}.mid_block.resnets.1", x, x.C)

    # ---------------------------------------------------------------- plans
    def build_decode(self, pb: Builder, z: Act, out_nchw: int, stats: Optional[Callable[[Act, int], int]] = None):
        """z: latents padded to 8 channels [B,h,w,8] -> fp32 NCHW image [B,4,8h,8w] at `out_nchw` (channel 3 is 0).
        stats(x, i): called on the sample in front of up block i, and behind the last one; returns the accumulator its first
        norm takes the statistics from (vae_asym.py: the blends).  Without it every norm launches its own."""
        P = self.P
        x = self._direct(pb, z, "post_quant_conv", 8)
        x = self._direct(pb, x, "decoder.conv_in", self.up[-1])
        x = self._mid(pb, "decoder", x)
        rev = list(reversed(self.up))
        for i, c in enumerate(rev):
            acc = stats(x, i) if stats else None
            for j in range(self.Lu + 1):
                x = self._resnet(pb, f"decoder.up_blocks.{i}.resnets.{j}", x, c, acc if j == 0 else None)
            if i != len(rev) - 1:
                pre = f"decoder.up_blocks.{i}.upsamplers.0.conv"
                x = pb.conv3x3(x, P[pre + ".weight"], c, P[pre + ".bias"], up=True)
                pb.taps.append((pre, x))
        x = self._norm(pb, x, "decoder.conv_norm_out", True, stats(x, len(rev)) if stats else None)
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
                    raise L.PPError(f"{self.NAME}.encode: image sides must be multiples of 2^(down blocks - 1)")
                pre = f"encoder.down_blocks.{i}.downsamplers.0.conv"
                x = pb.conv3x3(x, P[pre + ".weight"], c, P[pre + ".bias"], stride=2)
                pb.taps.append((pre, x))
        x = self._mid(pb, "encoder", x)
        x = self._norm(pb, x, "encoder.conv_norm_out", True)
        pb.taps.append(("encoder.conv_norm_out", x))
        x = self._direct(pb, x, "encoder.conv_out", 8)
        return self._direct(pb, x, "quant_conv", 8)


class PlanRuntime:
    """Device state (arena + launch plan) of one direction of one VAE network for one input shape (B, H, W).  A subclass gives
    `_build(arena, B, H, W) -> (lay, plan)`: `lay` names the buffers it allocated, "taps" among them."""

    def __init__(self, net, device, direction: str):
        self.net, self.device, self.direction = net, torch.device(device), direction
        self.key = None
        self.plan: Optional[Plan] = None
        self.arena: Optional[Arena] = None
        self.lay: Optional[dict] = None
        self.builds = 0                  # plans built so far (new values in buffers of a known shape build nothing)

    def ensure(self, B: int, H: int, W: int):
        if (B, H, W) == self.key:
            return
        dry = Arena()
        self._build(dry, B, H, W)
        self.arena = Arena(_align(dry.peak, 4096), self.device)      # zero-filled: the pad channels of x_in stay 0
        self.lay, self.plan = self._build(self.arena, B, H, W)
        self.key = (B, H, W)
        self.builds += 1


class VAERuntime(PlanRuntime):
    """One direction, "decode" or "encode", of one VAENet."""

    def _build(self, arena: Arena, B: int, H: int, W: int):
        pb = Builder(arena, dtype=self.net.dtype)
        lay = {"x_in": Act(arena.alloc(B * H * W * 8 * 2), B, H, W, 8)}
        if self.direction == "encode":
            lay["moments"] = self.net.build_encode(pb, lay["x_in"])
        else:
            lay["img"] = arena.alloc(B * 4 * (8 * H) * (8 * W) * 4)
            lay["shape"] = self._build_decode(pb, lay, B, H, W)
        lay["taps"] = pb.taps
        return lay, pb.plan

    def _build_decode(self, pb: Builder, lay: dict, B: int, H: int, W: int):
        return self.net.build_decode(pb, lay["x_in"], lay["img"])

    def run(self, x: torch.Tensor) -> torch.Tensor:
        """decode: latents [B,lat,h,w] -> fp32 [B,4,8h,8w] (a view of arena memory, valid until the next run);
        encode: ROTATED image [B,cin,H,W] -> rotated fp32 moments [B,8,H/8,W/8]."""
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
        self.plan.run(stream)
        if self.direction != "encode":
            return self.arena.view(self.lay["img"], self.lay["shape"], torch.float32)
        m = self.lay["moments"]
        out = torch.empty(m.B, 8, m.H, m.W, dtype=torch.float32, device=self.device)
        L.check(L.lib().pp_nhwc_to_nchw(m.ptr, m.B, 8, m.H * m.W, out.data_ptr(), 0, code, stream), "pp_nhwc_to_nchw")
        return out
