"""Shared by the VAE block tests (not a test file): the case list, teacher-forced float64 references, derived per-block error
bounds and a torch restatement of every block of the two VAE plans (powerpaint_amd/vae.py, vae_asym.py) with named defects.
Nothing here touches the HIP library; everything runs on the host in float64 (references, bounds) or float32 (emulation).

TAPS.  The plans record every block output (`rt.lay["taps"]`).  Tap k is checked against the block evaluated in float64 on the
HIP path's OWN BITS of its inputs (the previous tap; for a blend also the condition tap and the mask), with the weights as the
path stores them (matrices rounded to the 16-bit format, vectors fp32), converted block by block (`block_weights`).  The blocks
themselves are those of tests/asym_vae_cases.py (`resnet`, `attention`, `_conv`: the state-dict names of AutoencoderKL and of
AsymmetricAutoencoderKL are the same, so one restatement serves both); the stage walk below, which needs every intermediate
value for the bound, must reproduce their result (`CROSS_RTOL`, checked on every resnet and attention).  Encoder taps live in
the 180-degree-rotated frame of the plan: the REFERENCE is rotated (`flip(2, 3)` of the block on the flipped input, the
downsampler as Downsample2D's F.pad((0, 1, 0, 1)) + stride 2), never the taps.

BOUNDS (first order, per element, nothing fitted to a GPU result).  u = unit roundoff of the 16-bit format (2^-8 bf16, 2^-11
fp16), u32 = 2^-24.  A block is a chain of stages whose outputs the plan stores.  The gate of a tap is
        gate = own(last stage, at the reference's values) + (1 + u) carried(E_in)
  own terms, each the existing kernel gate, worst case:
    GroupNorm(+SiLU), statistics launch     norm_cases.gate_groupnorm with norm_cases.stats_eps(hw, C, groups)
    GroupNorm(+SiLU), accumulator           norm_cases.gate_groupnorm with `blend_acc_eps`: the accumulators pp_mask_blend sums are
                                            those of tests/test_asym_vae_kernels_gpu.py::_check_acc -- a thread adds 8 values in
                                            fp32 (7 u32 of sum|v| resp. Q), every partial is converted once (half a quantum,
                                            2^-25 resp. 2^-21) and there are 32 ceil(hw / 256) partials per channel, cg channels per
                                            group; norm_cases.acc_eps() is its one-partial, exact-sum special case
    conv / GEMM                             gemm_cases: u |ref| + (K + splits + 5) u32 A, A the absolute sum of everything added
                                            into the element (|x||w| products over the values the kernel may see, |x| + the
                                            running bound; |bias|; |res1|), splits = 8, the largest split-K the library chooses
                                            (gemm_cases.SPLITS)
    softmax                                 small_cases' pp_softmax_rows gate: u p + p (2^(2 D) - 1) + (n_S + 4) u32 p + half a
                                            subnormal, D = 2 u32 (|x| + |M|) in the exp2 domain, n_S = 3 (ceil(n / 256) + 16) + 3;
                                            here D also carries 3 u32 |x|: the reference scales by C^-1/2 in float64, the kernel
                                            by fp32(scale) * fp32(log2 e) rounded to fp32 (three roundings)
    pp_mask_blend                           test_asym_vae_kernels_gpu.py: E32 = ((1 + u32)^3 - 1)(|s m| + |c (1 - m)|), stored:
                                            E32 + u (|e| + E32) + 2^-25
    every stored 16-bit tensor              one rounding: u |ref| (+ 2^-25 in fp16: subnormals), norm_cases._finish
  the running bound E = (L, V) of a stored intermediate tensor, per element:
    L   the worst-case part, carried LINEARLY: the fp32-level terms of the norms and of the softmax (their gates less u |ref|)
    V   the sum of the SQUARED bounds of the rounding errors, carried IN QUADRATURE: one 16-bit rounding, (u ref)^2, per store
        and the n_r = K + splits + 5 fp32 roundings of a conv / GEMM accumulation, n_r (u32 A)^2
    and it stands for  L + LAMBDA sqrt(V):  rounding errors are modelled as independent, zero-mean and bounded (the model of
    Higham & Mary, "A new approach to probabilistic rounding error analysis", SIAM J. Sci. Comput. 41, 2019), and by
    Hoeffding's inequality a weighted sum of such errors exceeds LAMBDA sqrt(sum of squared weighted bounds) with probability
    <= 2 exp(-LAMBDA^2 / 2): 2.5e-14 per element at LAMBDA = 8, below 1e-5 over every element this suite checks.
    WHY NOT LINEAR THROUGHOUT: carried through |W| in the worst case, the 16-bit roundings of a resnet's first three stages
    alone reach the size of its output at K = 9 * 512 (each |W| pass multiplies a relative bound by about sqrt(K)), and
    conv_shortcut_bias_dropped, shortcut_reads_normed_input and the attention defects pass under such a gate
    (tests/test_vae_probes.py showed it): a bound under which a listed defect passes is too loose.  Single-stage taps (the
    narrow convs, the samplers, the condition encoder, the blends, conv_norm_out) carry nothing: their gates are the kernel
    gates, worst case.
  carried terms (first order):
    conv / GEMM                             L through |W|, V through W^2 (an up / down sampler's resampling included)
    GroupNorm                               its Jacobian, d x_hat_i = (dx_i - mean(dx)) / sigma - x_hat_i mean(x_hat dx) / sigma:
                                            L: |gamma| / sigma (L_i + mean_group(L) + |x_hat_i| rms_group(L)), from
                                            |mean(x_hat dx)| <= rms(x_hat) rms(dx) <= rms(dx);
                                            V: 3 (gamma / sigma)^2 (V_i + sum_group(V) / n^2 + x_hat_i^2 sum_group(x_hat^2 V) / n^2)
                                            ((a + b + c)^2 <= 3 (a^2 + b^2 + c^2))
    SiLU                                    its Lipschitz constant 1.1 (norm_cases: slope <= 1.1); ReLU: 1
    Q K^T, P V                              the product rule: L_q |k| + |q| L_k;  V_q k^2 + q^2 V_k
    softmax                                 dp_i = p_i (ds_i - sum_j p_j ds_j), ds the logit bound times the scale:
                                            L: p (L_i + sum p L);  V: 2 p^2 (V_i + sum p^2 V)
    residual add                            unchanged (the residual is a tap: exact bits; a stored conv_shortcut adds its own E)
The decoder's image (`decoder.conv_out`) is fp32: no 16-bit rounding; its channel 3 must be exactly 0.  Pad channels of the
narrow tensors (post_quant_conv: 4 of 8) carry reference 0 and gate 0: they must be exact zeros.

EMULATION (`emu_*`).  Each block in torch float32 (fp32 accumulation in the library's order, which the gates allow for: any
order) with a rounding to the 16-bit format wherever the plan stores a tensor; GroupNorm statistics are taken in float64 and
applied in fp32 (the kernels fold them in fixed point / fp64).  In the probe tests (tests/test_vae_probes.py) the emulation
takes the place of the GPU in the teacher-forced chain.  `DEFECTS` are carried by name; each is a plausible one-line mistake
in vae.py / vae_asym.py; `DEFECT_AT` names the kind of block it sits in.  cond_layer_order_reversed: the outputs of the
condition encoder have five different shapes, so a plan that hands them over in the wrong order is refused when it is built;
what can go wrong silently is the order of the two layers whose weights have the same shape (3 and 4): they trade weights.
"""
import math
from collections import namedtuple
from functools import lru_cache

import torch
import torch.nn.functional as F

import asym_vae_cases as AV
import norm_cases as NC

U32 = NC.U32
EPS = AV.EPS
MAX_SPLITS = 8                        # gemm_cases.SPLITS[-1]
LAMBDA = 8.0                          # Hoeffding: a sum of independent zero-mean terms |e_i| <= b_i exceeds LAMBDA sqrt(sum b_i^2)
#                                       with probability <= 2 exp(-LAMBDA^2 / 2) = 2.5e-14 per element
CROSS_RTOL = 1e-9                     # stage walk against asym_vae_cases' blocks, float64 both

KL = dict(in_channels=3, out_channels=3, latent_channels=4, down=(128, 256, 512, 512), layers_down=2, up=(128, 256, 512, 512),
          layers_up=2, groups=32)
ASYM = AV.X15
CFG = {"kl": KL, "asym": ASYM}
FMT = {"bf16": torch.bfloat16, "fp16": torch.float16}

DEFECTS = ("encoder_filter_not_rotated", "centre_tap_at_corner", "shortcut_reads_normed_input", "conv_shortcut_bias_dropped",
           "attention_residual_dropped", "softmax_scale_from_padded_keys", "second_image_reads_first_images_keys",
           "pad_keys_enter_softmax", "up_nearest_shifted_by_one", "down_pads_left_top", "logvar_mean_channels_swapped",
           "blend_statistics_of_unblended_sample", "blend_mask_not_resized_per_level", "cond_layer_order_reversed",
           "conv_out_pad_channel_nonzero")
# defect -> (kind of step it sits in, predicate on the step that carries it)
DEFECT_AT = {
    "encoder_filter_not_rotated": ("resnet", lambda s: s.name == "encoder.down_blocks.0.resnets.0"),
    "centre_tap_at_corner": ("direct", lambda s: s.opt["k"] == 1),
    "shortcut_reads_normed_input": ("resnet", lambda s: True),
    "conv_shortcut_bias_dropped": ("resnet", lambda s: s.opt["cin"] != s.opt["cout"]),
    "attention_residual_dropped": ("attention", lambda s: True),
    "softmax_scale_from_padded_keys": ("attention", lambda s: True),
    "second_image_reads_first_images_keys": ("attention", lambda s: True),
    "pad_keys_enter_softmax": ("attention", lambda s: True),
    "up_nearest_shifted_by_one": ("up", lambda s: True),
    "down_pads_left_top": ("down", lambda s: True),
    "logvar_mean_channels_swapped": ("direct", lambda s: s.name == "quant_conv"),
    "blend_statistics_of_unblended_sample": ("resnet_acc", lambda s: True),
    "blend_mask_not_resized_per_level": ("blend", lambda s: s.opt["level"] < 4),
    "cond_layer_order_reversed": ("cond4", lambda s: s.opt["layer"] >= 3),
    "conv_out_pad_channel_nonzero": ("conv_out", lambda s: True),
}

Case = namedtuple("Case", "id model direction fmt B H W cond")      # H, W: the latents (decode) or the image (encode)
Step = namedtuple("Step", "name kind src opt")


def _cases():
    out = []
    for B, H, W in ((2, 5, 6), (2, 8, 8), (3, 8, 9)):        # n = 30 (64 padded keys), 64 (none), 72 (128) tokens
        out.append(Case(f"kl-decode-{B}x{H}x{W}-bf16", "kl", "decode", "bf16", B, H, W, False))
    for H, W in ((40, 48), (64, 64)):
        out.append(Case(f"kl-encode-2x{H}x{W}-bf16", "kl", "encode", "bf16", 2, H, W, False))
    for fmt in ("bf16", "fp16"):
        out.append(Case(f"asym-decode-cond-2x4x6-{fmt}", "asym", "decode", fmt, 2, 4, 6, True))
        out.append(Case(f"asym-decode-2x4x6-{fmt}", "asym", "decode", fmt, 2, 4, 6, False))
        out.append(Case(f"asym-encode-2x32x48-{fmt}", "asym", "encode", fmt, 2, 32, 48, False))
    return out


CASES = _cases()


def thin(cfg):
    """The same widths with one layer per block (tests/test_vae_probes.py runs the defects there)."""
    return dict(cfg, layers_down=1, layers_up=1)


def unit(dtype) -> float:
    return NC.unit_roundoff(dtype)


# ------------------------------------------------------------------------------------------------ weights, inputs, steps
def make_net(model: str, cfg, dtype=torch.bfloat16):
    from powerpaint_amd.vae import VAENet
    from powerpaint_amd.vae_asym import AsymVAENet
    if model == "kl":
        assert dtype == torch.bfloat16 and cfg["down"] == cfg["up"] and cfg["layers_down"] == cfg["layers_up"]
        return VAENet(cfg["in_channels"], cfg["out_channels"], cfg["latent_channels"], cfg["up"], cfg["layers_up"], cfg["groups"])
    return AsymVAENet(cfg["in_channels"], cfg["out_channels"], cfg["latent_channels"], cfg["down"], cfg["layers_down"], cfg["up"],
                      cfg["layers_up"], cfg["groups"], dtype=dtype)


@lru_cache(maxsize=None)
def state_dict(model: str, layers=None):
    """synthetic_state_dict of the configuration (`layers`: one number for both sides, the thin form), built once."""
    cfg = CFG[model] if layers is None else dict(CFG[model], layers_down=layers, layers_up=layers)
    return make_net(model, cfg).synthetic_state_dict(seed=21 if model == "kl" else 22)


def block_weights(sd, prefix: str, dtype, to=torch.float64):
    """The block's weights as the HIP path stores them, in `to`, under their full names."""
    return AV.rounded_weights({k: v for k, v in sd.items() if k.startswith(prefix + ".")}, dtype, to=to)


def inputs(c: Case, same_items: bool = False):
    """dict z | img (+ image, mask): fp32, what the product entry point is given.  same_items: every batch item equal."""
    g = torch.Generator().manual_seed(1000 + c.B * 100 + c.H * 10 + c.W)
    rep = lambda t: t[:1].expand_as(t).contiguous() if same_items else t      # noqa: E731
    if c.direction == "encode":
        return dict(img=rep(torch.rand(c.B, 3, c.H, c.W, generator=g) * 2 - 1))
    d = dict(z=rep(torch.randn(c.B, 4, c.H, c.W, generator=g) * 3.0))
    if c.cond:
        d["image"] = rep(torch.rand(c.B, 3, 8 * c.H, 8 * c.W, generator=g) * 2 - 1)
        d["mask"] = rep(AV.two_masks(c.B, 8 * c.H, 8 * c.W, fractional=True))
    return d


def steps(cfg, direction: str, cond: bool = False, asym: bool = False):
    """The plan's block outputs in plan order (the tap names), each with its kind and the tap it reads."""
    S, lat = [], cfg["latent_channels"]

    def add(name, kind, src, **opt):
        S.append(Step(name, kind, src, opt))
        return name

    def mid(side, x, c):
        x = add(f"{side}.mid_block.resnets.0", "resnet", x, cin=c, cout=c)
        x = add(f"{side}.mid_block.attentions.0", "attention", x, c=c)
        return add(f"{side}.mid_block.resnets.1", "resnet", x, cin=c, cout=c)

    if direction == "encode":
        d = cfg["down"]
        x = add("encoder.conv_in", "direct", "x_in", k=3, cin=cfg["in_channels"], cout=d[0])
        for i, c in enumerate(d):
            for j in range(cfg["layers_down"]):
                x = add(f"encoder.down_blocks.{i}.resnets.{j}", "resnet", x, cin=d[max(i - 1, 0)] if j == 0 else c, cout=c)
            if i != len(d) - 1:
                x = add(f"encoder.down_blocks.{i}.downsamplers.0.conv", "down", x, c=c)
        x = mid("encoder", x, d[-1])
        x = add("encoder.conv_norm_out", "norm", x, c=d[-1])
        x = add("encoder.conv_out", "direct", x, k=3, cin=d[-1], cout=2 * lat)
        add("quant_conv", "direct", x, k=1, cin=2 * lat, cout=2 * lat)
        return S
    up = cfg["up"]
    rev = list(reversed(up))
    if cond:
        pre, ch = "decoder.condition_encoder.layers.", AV.condition_encoder_channels(up[0], up[-1])
        x = add(pre + "0", "direct", "img8", k=3, cin=cfg["out_channels"], cout=ch[0])
        x = add(pre + "1", "cond1", x, cin=ch[0], cout=ch[1])
        for l in (2, 3, 4):
            x = add(pre + str(l), "cond4", x, layer=l, cin=ch[l - 1], cout=ch[l])
    x = add("post_quant_conv", "direct", "x_in", k=1, cin=lat, cout=lat)
    x = add("decoder.conv_in", "direct", x, k=3, cin=lat, cout=up[-1])
    x = mid("decoder", x, up[-1])

    def blend(x, i):
        return add(f"decoder.mask_blend.{i}", "blend", x, level=i, cond=f"decoder.condition_encoder.layers.{4 - i}" if cond else None)

    for i, c in enumerate(rev):
        if asym:
            x = blend(x, i)
        for j in range(cfg["layers_up"] + 1):
            x = add(f"decoder.up_blocks.{i}.resnets.{j}", "resnet_acc" if asym and j == 0 else "resnet", x,
                    cin=rev[max(i - 1, 0)] if j == 0 else c, cout=c)
        if i != len(rev) - 1:
            x = add(f"decoder.up_blocks.{i}.upsamplers.0.conv", "up", x, c=c)
    if asym:
        x = blend(x, len(rev))
    x = add("decoder.conv_norm_out", "norm_acc" if asym else "norm", x, c=up[0])
    add("decoder.conv_out", "conv_out", x, cin=up[0], cout=cfg["out_channels"])
    return S


# ------------------------------------------------------------------------------------------------ stages: (ref, gate, E)
class Ctx:
    """dtype: the 16-bit format; bound=False: references only (the free-running oracle), every gate and E is None."""

    def __init__(self, dtype, groups: int = 32, bound: bool = True):
        self.dtype, self.groups, self.bound, self.u = dtype, groups, bound, unit(dtype)
        self.sub = 2.0 ** -25 if dtype == torch.float16 else 0.0

    def tot(self, E):
        """the running bound as one number per element: L + LAMBDA sqrt(V)"""
        return E[0] + LAMBDA * torch.sqrt(E[1])

    def gate(self, own, Ec):
        """own: the stage's worst-case gate at the reference's values; Ec: what it carried in (None: exact inputs)"""
        return own if Ec is None else own + (1.0 + self.u) * self.tot(Ec)

    def out(self, ref, own32, n_acc_A2, Ec):
        """E of a stored 16-bit tensor: own32 (worst-case fp32-level terms, linear), n_acc_A2 (the squares of the fp32
        accumulation's roundings), one 16-bit rounding, and what was carried in"""
        L = own32 + self.sub + (0.0 if Ec is None else Ec[0])
        V = n_acc_A2 + (self.u * ref) ** 2 + (0.0 if Ec is None else Ec[1])
        return L + torch.zeros_like(ref), V + torch.zeros_like(ref)


def blend_acc_eps(hw: int, cg: int):
    """(eS, eQ, aS, aQ) of the accumulators pp_mask_blend sums (the model of test_asym_vae_kernels_gpu.py::_check_acc)"""
    parts = (hw + 255) // 256 * 32
    return 7 * U32, 7 * U32, parts * cg * 2.0 ** -25, parts * cg * 2.0 ** -21


def s_conv(cx: Ctx, x, E, w, b, stride=1, padding=1, up=False, relu=False, res=None, Eres=None, store16=True):
    """x NCHW float64 with running bound E = (L, V) (None: exact bits) -> (conv (+ res), its gate, E of the stored output)"""
    if relu:
        x = F.relu(x)
    if up:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
        E = None if E is None else tuple(F.interpolate(t, scale_factor=2.0, mode="nearest") for t in E)
    ref = F.conv2d(x, w, b, stride=stride, padding=padding)
    if res is not None:
        ref = ref + res
    if not cx.bound:
        return ref, None, None
    wa, B = w.abs(), x.shape[0]
    kw = dict(stride=stride, padding=padding)
    if E is None:
        A, Ec = F.conv2d(x.abs(), wa, b.abs(), **kw), None
    else:
        both = F.conv2d(torch.cat([x.abs() + cx.tot(E), E[0]]), wa, None, **kw)
        A, Ec = both[:B] + b.abs()[None, :, None, None], (both[B:], F.conv2d(E[1], w * w, None, **kw))
    if res is not None:
        A = A + res.abs()
        if Eres is not None:                  # the stored shortcut: its bound rides the fp32 add unchanged
            A = A + cx.tot(Eres)
            Ec = Eres if Ec is None else (Ec[0] + Eres[0], Ec[1] + Eres[1])
    n_r = w[0].numel() + MAX_SPLITS + 5
    own = n_r * U32 * A + ((cx.u * ref.abs() + cx.sub) if store16 else 0.0)
    return ref, cx.gate(own, Ec), cx.out(ref, 0.0, n_r * (U32 * A) ** 2, Ec)


def s_linear(cx: Ctx, a, E, w, b, res=None):
    """a [.., n, K] tokens with bound E -> (a w^T + b (+ res) stored in 16 bits, gate, E)"""
    ref = a @ w.t() + b
    if res is not None:
        ref = ref + res
    if not cx.bound:
        return ref, None, None
    wt = w.t()
    A = (a.abs() + (0.0 if E is None else cx.tot(E))) @ wt.abs() + b.abs() + (0.0 if res is None else res.abs())
    Ec = None if E is None else (E[0] @ wt.abs(), E[1] @ (wt * wt))
    n_r = w.shape[1] + MAX_SPLITS + 5
    return ref, cx.gate(n_r * U32 * A + cx.u * ref.abs() + cx.sub, Ec), cx.out(ref, 0.0, n_r * (U32 * A) ** 2, Ec)


def _tok(x):
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B, H * W, C)


def _img(t, H, W):
    B, _, C = t.shape
    return t.reshape(B, H, W, C).permute(0, 3, 1, 2)


def s_gn(cx: Ctx, x, E, gamma, beta, silu: bool, terms):
    """GroupNorm(+SiLU) stored in 16 bits: x NCHW float64 with running bound E -> (ref, gate, E of the output)"""
    B, C, H, W = x.shape
    xt = _tok(x)
    if not cx.bound:
        return _img(NC.ref_groupnorm(xt, None, cx.groups, gamma, beta, EPS, silu), H, W), None, None
    ref, own = NC.gate_groupnorm(xt, None, cx.groups, gamma, beta, EPS, silu, cx.dtype, terms)
    Ec = None
    if E is not None:
        cg, n = C // cx.groups, H * W * (C // cx.groups)
        _, _, _, mean, var = NC._pop(xt, cx.groups)
        pc = lambda t: NC._per_channel(t, cg)      # noqa: E731
        grp = lambda t: t.reshape(B, H * W, cx.groups, cg)      # noqa: E731
        sigma = pc(torch.sqrt(var + EPS))
        xhat = (xt - pc(mean)) / sigma
        Lt, Vt = _tok(E[0]), _tok(E[1])
        k = (1.1 if silu else 1.0) * gamma.abs() / sigma
        Lc = k * (Lt + pc(grp(Lt).mean((1, 3))) + xhat.abs() * pc(torch.sqrt(grp(Lt * Lt).mean((1, 3)))))
        # three terms of one sum: (a + b + c)^2 <= 3 (a^2 + b^2 + c^2); mean(dx) has sum(V) / n^2, mean(x_hat dx) sum(x_hat^2 V) / n^2
        Vc = 3.0 * k * k * (Vt + pc(grp(Vt).sum((1, 3))) / n ** 2 + xhat ** 2 * pc(grp(xhat ** 2 * Vt).sum((1, 3))) / n ** 2)
        Ec = (Lc, Vc)
    Eo = cx.out(ref, own - cx.u * ref.abs() - cx.sub, 0.0, Ec)
    img = lambda t: _img(t, H, W)      # noqa: E731
    return img(ref), img(cx.gate(own, Ec)), (img(Eo[0]), img(Eo[1]))


# ------------------------------------------------------------------------------------------------ blocks: (ref, gate)
def gate_direct(cx, w, st, x):
    """pp_conv3x3_direct on channel-padded tensors: x has >= cin channels; the output is padded to 8 where cout < 8"""
    o = st.opt
    ref, g, _ = s_conv(cx, x[:, :o["cin"]], None, w[st.name + ".weight"], w[st.name + ".bias"], padding=o["k"] // 2)
    pad = (8 - o["cout"]) if o["cout"] < 8 else 0
    if pad:
        ref, g = F.pad(ref, (0, 0, 0, 0, 0, pad)), (None if g is None else F.pad(g, (0, 0, 0, 0, 0, pad)))
    return ref, g


def gate_resnet(cx, w, st, x, acc_terms=None):
    pre, (B, C, H, W) = st.name, x.shape
    t1 = acc_terms or NC.stats_eps(H * W, C, cx.groups)
    h, _, E = s_gn(cx, x, None, w[pre + ".norm1.weight"], w[pre + ".norm1.bias"], True, t1)
    h, _, E = s_conv(cx, h, E, w[pre + ".conv1.weight"], w[pre + ".conv1.bias"])
    h, _, E = s_gn(cx, h, E, w[pre + ".norm2.weight"], w[pre + ".norm2.bias"], True, NC.stats_eps(H * W, h.shape[1], cx.groups))
    sc, Esc = x, None
    if pre + ".conv_shortcut.weight" in w:
        sc, _, Esc = s_conv(cx, x, None, w[pre + ".conv_shortcut.weight"], w[pre + ".conv_shortcut.bias"], padding=0)
    ref, g, _ = s_conv(cx, h, E, w[pre + ".conv2.weight"], w[pre + ".conv2.bias"], res=sc, Eres=Esc)
    if not cx.bound:
        return ref, None
    want = AV.resnet(w, pre, x, cx.groups)
    assert torch.allclose(ref, want, rtol=CROSS_RTOL, atol=CROSS_RTOL * float(want.abs().max())), pre
    return want, g


def softmax_own(cx, logits, scale: float, n: int):
    """(p, own gate) of pp_softmax_rows on float64 logits [.., n] (small_cases.build_softmax + the scale's three roundings)"""
    x2 = logits * (scale * math.log2(math.e))
    M = x2.max(-1, keepdim=True).values
    p = torch.softmax(logits * scale, -1)
    D = U32 * (5.0 * x2.abs() + 2.0 * M.abs())
    n_s = 3 * (-(-n // 256) + 16) + 3
    sub = 2.0 ** -25 if cx.dtype == torch.float16 else 2.0 ** -134
    return p, cx.u * p + p * (torch.exp2(2 * D) - 1) + (n_s + 4) * U32 * p + sub


def gate_attention(cx, w, st, x):
    pre, (B, C, H, W) = st.name, x.shape
    n, scale = H * W, C ** -0.5
    npad = -(-n // 64) * 64
    h, _, E = s_gn(cx, x, None, w[pre + ".group_norm.weight"], w[pre + ".group_norm.bias"], False, NC.stats_eps(n, C, cx.groups))
    t, Et = _tok(h), (None if E is None else (_tok(E[0]), _tok(E[1])))
    lin = lambda nm, a, Ea, res=None: s_linear(cx, a, Ea, w[f"{pre}.{nm}.weight"].reshape(C, C), w[f"{pre}.{nm}.bias"], res)   # noqa: E731
    (q, _, Eq), (k, _, Ek), (v, _, Ev) = lin("to_q", t, Et), lin("to_k", t, Et), lin("to_v", t, Et)
    s = q @ k.transpose(1, 2)
    if not cx.bound:
        o = torch.softmax(s * scale, -1) @ v
        return _img(lin("to_out.0", o, None, _tok(x))[0], H, W), None
    T = lambda m: m.transpose(1, 2)      # noqa: E731
    A_s = (q.abs() + cx.tot(Eq)) @ T(k.abs() + cx.tot(Ek))
    n_s = C + MAX_SPLITS + 5
    Ls = Eq[0] @ T(k.abs()) + q.abs() @ T(Ek[0])
    Vs = Eq[1] @ T(k * k) + (q * q) @ T(Ek[1]) + n_s * (U32 * A_s) ** 2                  # S is fp32: no 16-bit rounding
    p, own = softmax_own(cx, s, scale, n)
    Lsl, Vsl = Ls * scale, Vs * scale * scale
    Lp = (own - cx.u * p) + p * (Lsl + (p * Lsl).sum(-1, keepdim=True))
    Vp = (cx.u * p) ** 2 + 2.0 * p * p * (Vsl + (p * p * Vsl).sum(-1, keepdim=True))     # (a - b)^2 <= 2 (a^2 + b^2)
    o = p @ v
    A_o = (p + cx.tot((Lp, Vp))) @ (v.abs() + cx.tot(Ev))
    n_o = npad + MAX_SPLITS + 5
    Eo = (Lp @ v.abs() + p @ Ev[0] + cx.sub, Vp @ (v * v) + (p * p) @ Ev[1] + n_o * (U32 * A_o) ** 2 + (cx.u * o) ** 2)
    ref, g, _ = lin("to_out.0", o, Eo, _tok(x))
    want = AV.attention(w, pre, x, cx.groups)
    ref = _img(ref, H, W)
    assert torch.allclose(ref, want, rtol=CROSS_RTOL, atol=CROSS_RTOL * float(want.abs().max())), pre
    return want, _img(g, H, W)


def gate_sampler(cx, w, st, x):
    if st.kind == "up":
        return s_conv(cx, x, None, w[st.name + ".weight"], w[st.name + ".bias"], up=True)[:2]
    return s_conv(cx, F.pad(x, (0, 1, 0, 1)), None, w[st.name + ".weight"], w[st.name + ".bias"], stride=2, padding=0)[:2]


def gate_cond(cx, w, st, x):
    """layers 1..4 of the condition encoder: ReLU of the stored pre-ReLU tap, then the 3x3 (layer 1) or 4x4 stride-2 conv"""
    s4 = st.kind == "cond4"
    return s_conv(cx, x, None, w[st.name + ".weight"], w[st.name + ".bias"], stride=2 if s4 else 1, relu=True)[:2]


def gate_blend(cx, st, x, cond, mask):
    """pp_mask_blend in place: x the sample in front of the blend; cond None: the plan only sums statistics, x is unchanged"""
    if cond is None:
        return x, (torch.zeros_like(x) if cx.bound else None)
    m = AV.nearest_mask(mask, x.shape[-2], x.shape[-1])
    a, b = x * m, cond * (1.0 - m)
    e = a + b
    if not cx.bound:
        return e, None
    e32 = ((1 + U32) ** 3 - 1) * (a.abs() + b.abs())
    return e, e32 + cx.u * (e.abs() + e32) + 2.0 ** -25


def gate_norm(cx, w, st, x, acc: bool):
    B, C, H, W = x.shape
    terms = blend_acc_eps(H * W, C // cx.groups) if acc else NC.stats_eps(H * W, C, cx.groups)
    return s_gn(cx, x, None, w[st.name + ".weight"], w[st.name + ".bias"], True, terms)[:2]


def gate_conv_out(cx, w, st, x):
    """pp_conv3x3_smallcout: fp32 NCHW, 4 channels, channel 3 exactly 0"""
    ref, g, _ = s_conv(cx, x, None, w[st.name + ".weight"], w[st.name + ".bias"], store16=False)
    return F.pad(ref, (0, 0, 0, 0, 0, 4 - ref.shape[1])), (None if g is None else F.pad(g, (0, 0, 0, 0, 0, 4 - g.shape[1])))


def gate_step(cx: Ctx, sd, st: Step, taps, extra):
    """(ref, gate) of tap st.name from the bits of its inputs.  taps: name -> NCHW float64; extra: x_in, img8 (NCHW float64,
    8 channels), mask ([B, 1, H, W] float64), pre_blend (name of a blend -> the sample in front of it)."""
    w = block_weights(sd, st.name, cx.dtype) if st.kind != "blend" else None
    x = extra["pre_blend"][st.name] if st.kind == "blend" else (extra[st.src] if st.src in ("x_in", "img8") else taps[st.src])
    enc = st.name.startswith(("encoder.", "quant_conv"))
    if enc:
        x = x.flip(2, 3)
    if st.kind == "direct":
        r = gate_direct(cx, w, st, x)
    elif st.kind == "resnet":
        r = gate_resnet(cx, w, st, x)
    elif st.kind == "resnet_acc":
        r = gate_resnet(cx, w, st, x, blend_acc_eps(x.shape[2] * x.shape[3], x.shape[1] // cx.groups))
    elif st.kind == "attention":
        r = gate_attention(cx, w, st, x)
    elif st.kind in ("up", "down"):
        r = gate_sampler(cx, w, st, x)
    elif st.kind in ("cond1", "cond4"):
        r = gate_cond(cx, w, st, x)
    elif st.kind == "blend":
        r = gate_blend(cx, st, x, taps[st.opt["cond"]] if st.opt["cond"] else None, extra.get("mask"))
    elif st.kind in ("norm", "norm_acc"):
        r = gate_norm(cx, w, st, x, st.kind == "norm_acc")
    else:
        r = gate_conv_out(cx, w, st, x)
    return (r[0].flip(2, 3), None if r[1] is None else r[1].flip(2, 3)) if enc else r


def _unravel(i: int, shape):
    idx = []
    for n in reversed(shape):
        idx.append(i % n)
        i //= n
    return tuple(reversed(idx))


def where_worst(out, ref, gate):
    """(worst |out - ref| / gate, (b, c, y, x) of it)"""
    err = (out.double() - ref).abs()
    if not bool(torch.isfinite(err).all()):
        return math.inf, _unravel(int((~torch.isfinite(err)).flatten().nonzero()[0]), err.shape)
    r = torch.where(gate > 0, err / gate.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    i = int(r.flatten().argmax())
    return float(r.flatten()[i]), _unravel(i, r.shape)


def check_chain(c: Case, cfg, sd, taps, extra, only=None):
    """Every tap of the chain against its teacher-forced reference -> [(name, kind, worst ratio, where)]"""
    cx = Ctx(FMT[c.fmt], cfg["groups"])
    out = []
    for st in steps(cfg, c.direction, c.cond, c.model == "asym"):
        if only is not None and st.name not in only:
            continue
        ref, gate = gate_step(cx, sd, st, taps, extra)
        assert tuple(ref.shape) == tuple(taps[st.name].shape), (st.name, tuple(ref.shape), tuple(taps[st.name].shape))
        out.append((st.name, st.kind) + where_worst(taps[st.name], ref, gate))
    return out


def free_run(c: Case, cfg, sd, extra):
    """The whole chain in float64 from the input bits, every block on the reference's own output: the end-to-end oracle.
    -> the image [B, 3, H, W] or the moments [B, 8, h, w] (unrotated)."""
    cx = Ctx(FMT[c.fmt], cfg["groups"], bound=False)
    taps, pre = {}, {}
    for st in steps(cfg, c.direction, c.cond, c.model == "asym"):
        if st.kind == "blend":
            pre[st.name] = taps[st.src]
        taps[st.name] = gate_step(cx, sd, st, taps, dict(extra, pre_blend=pre))[0]
    return taps["decoder.conv_out"][:, :3] if c.direction == "decode" else taps["quant_conv"].flip(2, 3)


# ------------------------------------------------------------------------------------------------ emulation
def r16(t, dtype):
    return t.to(dtype).float()


def e_gn(x, gamma, beta, silu, dtype, groups, stats_of=None):
    """statistics (of `stats_of`, default x) in float64, scale / shift in fp32, one rounding"""
    B, C, H, W = x.shape
    sx = (x if stats_of is None else stats_of).double().reshape(B, groups, -1)
    mean, var = sx.mean(-1), sx.var(-1, unbiased=False)
    rstd = (1.0 / torch.sqrt(var + EPS)).float().repeat_interleave(C // groups, 1)[:, :, None, None]
    mean = mean.float().repeat_interleave(C // groups, 1)[:, :, None, None]
    sc = rstd * gamma.float()[None, :, None, None]
    y = x.float() * sc + (beta.float()[None, :, None, None] - mean * sc)
    return r16(F.silu(y) if silu else y, dtype)


def e_conv(x, w, b, dtype, store16=True, **kw):
    y = F.conv2d(x.float(), w.float(), None if b is None else b.float(), **kw)
    return r16(y, dtype) if store16 else y


def emu_direct(w, st, x, dtype, defect=None, rot=False):
    o = st.opt
    wt, b = w[st.name + ".weight"], w[st.name + ".bias"]
    if o["k"] == 1:                                            # a 1x1 conv is a 3x3 whose only non-zero tap is the centre
        full = torch.zeros(wt.shape[0], wt.shape[1], 3, 3)
        at = 0 if defect == "centre_tap_at_corner" else 1
        full[:, :, at, at] = wt[:, :, 0, 0]
        wt = full
    elif rot:
        wt = wt.flip(2, 3)
    y = e_conv(x[:, :o["cin"]], wt, b, dtype, padding=1)
    if defect == "logvar_mean_channels_swapped":
        y = torch.cat([y[:, o["cout"] // 2:], y[:, :o["cout"] // 2]], 1)
    return F.pad(y, (0, 0, 0, 0, 0, 8 - o["cout"])) if o["cout"] < 8 else y


def emu_resnet(w, st, x, dtype, groups, defect=None, rot=False, stats_of=None):
    pre = st.name
    R = (lambda t: t.flip(2, 3)) if rot else (lambda t: t)
    h1 = e_gn(x, w[pre + ".norm1.weight"], w[pre + ".norm1.bias"], True, dtype, groups, stats_of=stats_of)
    w1 = w[pre + ".conv1.weight"]
    h = e_conv(h1, w1 if defect == "encoder_filter_not_rotated" else R(w1), w[pre + ".conv1.bias"], dtype, padding=1)
    h = e_gn(h, w[pre + ".norm2.weight"], w[pre + ".norm2.bias"], True, dtype, groups)
    src = h1 if defect == "shortcut_reads_normed_input" else x.float()
    if pre + ".conv_shortcut.weight" in w:
        bsc = None if defect == "conv_shortcut_bias_dropped" else w[pre + ".conv_shortcut.bias"]
        src = e_conv(src, w[pre + ".conv_shortcut.weight"], bsc, dtype)
    return r16(F.conv2d(h, R(w[pre + ".conv2.weight"]).float(), w[pre + ".conv2.bias"].float(), padding=1) + src, dtype)


def emu_attention(w, st, x, dtype, groups, defect=None):
    """The per-image loop of VAENet._attention: K is one buffer of B n + (npad - n) rows, image b's npad key rows start at row
    b n; S has npad columns, the softmax reads n of them and writes P's pad columns as zeros."""
    pre, (B, C, H, W) = st.name, x.shape
    n = H * W
    npad = -(-n // 64) * 64
    h = _tok(e_gn(x, w[pre + ".group_norm.weight"], w[pre + ".group_norm.bias"], False, dtype, groups))
    lin = lambda nm, a: a @ w[f"{pre}.{nm}.weight"].reshape(C, C).float().t() + w[f"{pre}.{nm}.bias"].float()      # noqa: E731
    q, k, v = r16(lin("to_q", h), dtype), r16(lin("to_k", h), dtype), r16(lin("to_v", h), dtype)
    krows = torch.cat([k.reshape(B * n, C), torch.zeros(npad - n, C)])
    scale = float(npad if defect == "softmax_scale_from_padded_keys" else C) ** -0.5
    o = torch.empty_like(q)
    for b in range(B):
        kb = 0 if defect == "second_image_reads_first_images_keys" else b
        s = q[b] @ krows[kb * n: kb * n + npad].t()
        cols = npad if defect == "pad_keys_enter_softmax" else n
        p = r16(torch.softmax(s[:, :cols] * scale, -1), dtype)[:, :n]
        o[b] = r16(p @ v[b], dtype)
    out = lin("to_out.0", o)
    return _img(r16(out if defect == "attention_residual_dropped" else out + _tok(x.float()), dtype), H, W)


def emu_sampler(w, st, x, dtype, defect=None):
    wt, b = w[st.name + ".weight"], w[st.name + ".bias"]
    if st.kind == "up":
        B, C, H, W = x.shape
        sh = 1 if defect == "up_nearest_shifted_by_one" else 0
        iy = ((torch.arange(2 * H) + sh) // 2).clamp_max(H - 1)
        ix = ((torch.arange(2 * W) + sh) // 2).clamp_max(W - 1)
        return e_conv(x.float()[:, :, iy][:, :, :, ix], wt, b, dtype, padding=1)
    # the plan's frame: rotated image, rotated filter, symmetric padding (its last row / column of padding is never read)
    if defect == "down_pads_left_top":
        return e_conv(F.pad(x.float(), (0, 1, 0, 1)), wt.flip(2, 3), b, dtype, stride=2)
    return e_conv(x, wt.flip(2, 3), b, dtype, stride=2, padding=1)


def emu_cond(w, st, x, dtype):
    return e_conv(F.relu(x.float()), w[st.name + ".weight"], w[st.name + ".bias"], dtype, stride=2 if st.kind == "cond4" else 1, padding=1)


def emu_blend(st, x, cond, mask, dtype, defect=None):
    if cond is None:
        return x.float()
    h, wd = x.shape[-2:]
    m = mask[..., :h, :wd] if defect == "blend_mask_not_resized_per_level" else AV.nearest_mask(mask, h, wd)
    m = m.float()
    return r16(torch.addcmul(cond.float() * (1.0 - m), x.float(), m), dtype)


def emu_step(sd, st: Step, taps, extra, dtype, groups, defect=None):
    """The emulation's tap st.name from the emulation's own earlier taps (its frame: encoder rotated), float32 values."""
    w = block_weights(sd, st.name, dtype, to=torch.float32) if st.kind != "blend" else None
    x = extra["pre_blend"][st.name] if st.kind == "blend" else (extra[st.src] if st.src in ("x_in", "img8") else taps[st.src])
    rot = st.name.startswith("encoder.")
    if st.kind == "direct":
        return emu_direct(w, st, x, dtype, defect, rot)
    if st.kind in ("resnet", "resnet_acc"):
        so = None
        if defect == "blend_statistics_of_unblended_sample":
            so = extra["pre_blend"][st.src]
        return emu_resnet(w, st, x, dtype, groups, defect, rot, stats_of=so)
    if st.kind == "attention":
        return emu_attention(w, st, x, dtype, groups, defect)
    if st.kind in ("up", "down"):
        return emu_sampler(w, st, x, dtype, defect)
    if st.kind in ("cond1", "cond4"):
        if defect == "cond_layer_order_reversed":                  # layers 3 and 4 (equal shapes) trade weights
            other = st.name[:-1] + str(7 - st.opt["layer"])
            wo = block_weights(sd, other, dtype, to=torch.float32)
            w = {k.replace(other, st.name): v for k, v in wo.items()}
        return emu_cond(w, st, x, dtype)
    if st.kind == "blend":
        return emu_blend(st, x, taps[st.opt["cond"]] if st.opt["cond"] else None, extra.get("mask"), dtype, defect)
    if st.kind in ("norm", "norm_acc"):
        return e_gn(x, w[st.name + ".weight"], w[st.name + ".bias"], True, dtype, groups)
    y = e_conv(x, w[st.name + ".weight"], w[st.name + ".bias"], dtype, store16=False, padding=1)
    y = F.pad(y, (0, 0, 0, 0, 0, 4 - y.shape[1]))
    if defect == "conv_out_pad_channel_nonzero":
        y[:, 3] = y[:, 2]
    return y


def emu_inputs(c: Case, inp):
    """What the runtime puts in front of the plan: x_in (8 channels, the encoder's image rotated), img8 = (1 - mask) * image in
    fp32 rounded once, the fp32 mask planes."""
    dtype = FMT[c.fmt]
    if c.direction == "encode":
        return dict(x_in=F.pad(r16(inp["img"].flip(2, 3), dtype), (0, 0, 0, 0, 0, 5)))
    ex = dict(x_in=F.pad(r16(inp["z"], dtype), (0, 0, 0, 0, 0, 4)))
    if c.cond:
        ex["mask"] = inp["mask"].float()
        ex["img8"] = F.pad(r16((1.0 - ex["mask"]) * inp["image"].float(), dtype), (0, 0, 0, 0, 0, 5))
    return ex


def emulate(c: Case, cfg, sd, inp):
    """The faithful chain -> (taps: name -> float32 NCHW, extra with pre_blend filled)"""
    dtype = FMT[c.fmt]
    extra = dict(emu_inputs(c, inp), pre_blend={})
    taps = {}
    for st in steps(cfg, c.direction, c.cond, c.model == "asym"):
        if st.kind == "blend":
            extra["pre_blend"][st.name] = taps[st.src]
        taps[st.name] = emu_step(sd, st, taps, extra, dtype, cfg["groups"])
    return taps, extra


def as64(taps, extra):
    d = lambda t: t.double() if torch.is_tensor(t) else t      # noqa: E731
    return {k: d(v) for k, v in taps.items()}, {k: ({a: d(b) for a, b in v.items()} if isinstance(v, dict) else d(v)) for k, v in extra.items()}


# ------------------------------------------------------------------------------------------------ the tap layout (CPU)
def expected_tap_names(net, direction: str, cond: bool = False):
    """The tap names in plan order, from the net's own structure lists (`_resnets`, `_samplers`, `_cond_layers`)."""
    side = "encoder" if direction == "encode" else "decoder"
    res = [pre for pre, _, _ in net._resnets() if pre.startswith(side)]
    smp = [pre for pre, _ in net._samplers() if pre.startswith(side)]
    asym = hasattr(net, "_cond_layers")
    mid = [f"{side}.mid_block.resnets.0", f"{side}.mid_block.attentions.0", f"{side}.mid_block.resnets.1"]
    blocks = sorted({int(pre.split(".")[2]) for pre in res if "_blocks." in pre})
    body = []
    for i in blocks:
        if asym and direction == "decode":
            body.append(f"decoder.mask_blend.{i}")
        body += [pre for pre in res if pre.split(".")[1:3] == [("down" if side == "encoder" else "up") + "_blocks", str(i)]]
        body += [pre for pre in smp if pre.split(".")[2] == str(i)]
    if direction == "encode":
        return ["encoder.conv_in"] + body + mid + ["encoder.conv_norm_out", "encoder.conv_out", "quant_conv"]
    head = [name for name, _, _, _ in net._cond_layers()] if cond else []
    tail = [f"decoder.mask_blend.{len(blocks)}"] if asym else []
    return head + ["post_quant_conv", "decoder.conv_in"] + mid + body + tail + ["decoder.conv_norm_out", "decoder.conv_out"]


def dry_build(rt, B: int, H: int, W: int):
    """rt._build on a dry arena whose `alloc` is logged -> (lay, plan, [(ptr, nbytes)] in allocation order)"""
    from powerpaint_amd.engine import Arena
    arena, log = Arena(), []
    alloc = arena.alloc

    def logged(nbytes):
        ptr = alloc(nbytes)
        log.append((ptr, nbytes))
        return ptr

    arena.alloc = logged
    lay, plan = rt._build(arena, B, H, W)
    return lay, plan, log


def tap_layout_violations(taps, log):
    """Every tap must keep its bytes to the end of the plan: no other tap's range and no allocation made after its own may
    overlap it.  A mask_blend tap works in place: it IS the tap in front of it (same Act), and is checked as that one."""
    bad, spans = [], []
    for i, t in enumerate(taps):
        name, act = t[0], t[1]
        if ".mask_blend." in name:
            if i == 0 or act is not taps[i - 1][1] or len(t) != 3 or not t[2]:
                bad.append((name, "not the tap in front of it / no accumulator"))
            continue
        own = [j for j, (p, n) in enumerate(log) if p == act.ptr and n == act.nbytes]
        if not own:
            bad.append((name, "no allocation of its own"))
            continue
        lo, hi = act.ptr, act.ptr + act.nbytes
        bad += [(name, f"allocation {j} overlaps") for j in range(own[-1] + 1, len(log)) if log[j][0] < hi and lo < log[j][0] + log[j][1]]
        bad += [(name, f"overlaps tap {o}") for o, a, b in spans if a < hi and lo < b]
        spans.append((name, lo, hi))
    return bad
