"""Shared by the SD network block tests (not a test file): the case list, the wiring of the three networks by name, teacher-forced
float64 references, derived per-segment error bounds and a torch restatement of the segments of the step plans
(powerpaint_amd/engine.py, SDNet.build_step) with named defects.  Nothing here launches a kernel; the library is loaded only for
the dry builds (its `*_supported` queries run on a machine without a GPU).

TAPS.  build_step records (`rt.lay["taps"]`) every block output -- temb_all, conv_in (and `conv_in.add_sample`, the second
conv_in of a UNet that takes BrushNet residuals), every `*.resnets.j`, `*.attentions.j`, `*.downsamplers.0`, `*.upsamplers.0`,
`mid_block.*`, the `skip_add.k` sums of a UNet that takes ControlNet residuals, every zero conv of a side network, the UNet's
`eps` -- and, with the plan call that completes it, the tensors inside the blocks: `<resnet>.conv1`, and of a transformer what the
chosen form stores of `.proj_in`, `.attn1`, `.attn1_out`, `.attn2`.

WHAT IS GATED HERE.  Every segment of the plan: tap k against the segment evaluated in float64 on the HIP path's
OWN BITS of its inputs, with the weights as the path stores them (matrices rounded to the 16-bit format, vectors fp32; the
sub-pixel upsampling conv: the folded sums of the rounded weights, rounded once more, upconv_cases.fold).  The inputs of a
segment are chosen BY NAME from the wiring of the reference networks (`steps`: unet_2d_condition.py:1040-1363,
BrushNet_CA.py:690-952 of the reference, the diffusers ControlNet as oracle/sd_modules.py restates it), never by following the
plan's pointers: a block fed the wrong tensor shows as a wrong output.  Segments:
    temb            t -> temb_all: the sinusoid, linear_1 + SiLU, linear_2, then SiLU -> every resnet's time_emb_proj, rows
                    concatenated in SDNet._resnet_specs order (the layout conv1's `rowvec` reads)
    conv_in         x_in (+ the ControlNet conditioning embedding | + add_down[0]) -> conv_in
    res_a           x (, skip), temb_all -> <resnet>.conv1
    res_b           <resnet>.conv1, x (, skip, res2) -> <resnet>
    down | up       the samplers (+ res2); up resizes to the size of the skip tensor the next block pops
    add             skip + ControlNet residual (pp_add: the float64 sum rounded once, gate 0: bit equality)
    zero            a side network's zero conv, times the conditioning scale
    eps             conv_norm_out + SiLU + conv_out, fp32 NCHW
    t_in            x -> <transformer>.proj_in: GroupNorm (eps 1e-6, no SiLU) -> proj_in
    t_out1          (.proj_in, .attn1) -> .attn1_out: attn1.to_out + bias + the residual (absent where the form is BLOCK_PRE)
    t_ff            (.attn2, x, res2) -> <transformer>: folded norm3 -> GEGLU -> [g | hs] x the composed FF2 . proj_out matrix +
                    its composed bias + the transformer's input (+ res2).  Its weights are the PACKED ones, read by name from
                    the network's ParamPack (ff1.weight with norm3's gamma folded in and its rows in GEGLU quads, ff1.colsum,
                    ff1.bias = W beta + b, ff2_proj_out.weight = [W_po W_ff2 | W_po] composed in fp32 and rounded once,
                    ff2_proj_out.bias = W_po b_ff2 + b_po): what the path stores is a function of several checkpoint tensors
                    there, and the float64 formula on the UNROUNDED composition must equal oracle/sd_modules.py (CROSS_RTOL)
    t_attn1         .proj_in -> .attn1: norm1 folded into the QKV GEMM (packed attn1.qkv.*), self-attention per head (gate_t_attn1)
    t_attn2         .attn1_out -> .attn2: CHAIN (gate_t_attn2: folded to_q, hoisted K / V, attention over the NCTX real keys, to_out)
                    and the folded forms BLOCK and TWO_GEMM (gate_t_attn2_folded: G and H rounded once more per prompt)
Every packed tensor these read is compared with its composition from the checkpoint tensors (`pack_violations`), and each float64
formula on the UNROUNDED composition must equal oracle/sd_modules.py (CROSS_RTOL).  Under BLOCK_PRE (C = 320 where pp_xattn_block
runs) .attn1_out is never stored: .attn2 is teacher-forced from (.proj_in, .attn1), the bound of the h the launch forms itself
carried through norm2 into the logits and along the residual (gate_t_attn2_folded, pre_in).

BOUNDS.  The model of tests/vae_cases.py, reused (its docstring has the derivation): own terms from the kernel gates, the running
bound E = (L, V) of a stored intermediate tensor, LAMBDA = 8.  What is added to it:
    GroupNorm statistics    the path is the library's choice per shape (statistics launch, or int64 accumulators filled by the
                            producers' epilogues): `gn_terms` takes, per term, the larger of norm_cases.stats_eps and of
                            norm_cases.gate_epilogue_acc's terms where the caller cannot know the form (256-row column sums:
                            eS = 256 u32, eQ = 257 u32; 16-row blocks: (ceil(hw / 16) + 3) cg adds of half a quantum, the + 3 for
                            the four parities of a sub-pixel producer)
    conv1                   |bias| and |temb row| both enter A (two adds of the epilogue: in n_r's 5)
    conv2 + shortcut        the 1x1 shortcut is a K tail of conv2 (SDNet.merge_shortcut: every width here is a multiple of 64):
                            one accumulation over K = 9 cout + cin, A over both parts and both biases, no rounding between
    identity shortcut       |x| (and |res2|) enter A
    temb                    fp32 throughout, carried linearly: small_cases' gates of pp_timestep_embedding ((3 |e| + 5) u32 |a| +
                            4 u32 |ref|) and of pp_linear_skinny ((K + 7) u32 A, SiLU in / out: 1.1 d + (7 + |v|) u32 |y|),
                            each carried through |W| of the next
    eps                     vae_cases' conv_out: GroupNorm gate carried through |W|, (K + 13) u32 A, no 16-bit rounding
    t_ff                    norm_cases.gate_folded_ln (GEGLU) on row moments that the producer's epilogue formed (gate_row_stats:
                            28 / 29 u32) and the consumer folded over the tiles (folded_ln_eps): eS = (31 + tiles) u32,
                            eQ = (34 + tiles) u32; the GEGLU value g is rounded to 16 bits once (stored, or handed to the second
                            MFMA inside pp_ff_fused): its gate less u |g| is carried linearly, (u g)^2 in quadrature, through
                            the composed matrix; the second GEMM is norm_cases.gate_ff_fused's, K = 5 C

EMULATION (`emu_*`).  Each segment in torch float32 with a rounding to the 16-bit format wherever the plan stores a tensor;
GroupNorm statistics in float64, applied in fp32 (vae_cases.e_gn).  `DEFECTS` are carried by name, each a plausible one-line
mistake in engine.py; `DEFECT_AT` names the kind of segment it sits in and which segments can carry it.
"""
import math
from collections import namedtuple
from functools import lru_cache

import torch
import torch.nn.functional as F

import asym_vae_cases as AV
import norm_cases as NC
import small_cases as SC
import upconv_cases as UC
import vae_cases as VC

U32, LAMBDA, CROSS_RTOL, MAX_SPLITS = VC.U32, VC.LAMBDA, VC.CROSS_RTOL, VC.MAX_SPLITS
BOC, HEADS, NCTX, CTX_DIM, GROUPS, EPS = (320, 640, 1280, 1280), 8, 77, 768, 32, 1e-5
CIN_PAD = 64                          # the input buffer's channels (zero-padded to one K chunk)
FMT = VC.FMT
SCALE = 0.75                          # conditioning scale of the side-network cases (1.0 would hide a scale applied twice)
TIMESTEP = 481.0

Net = namedtuple("Net", "kind cin layers wiring")        # wiring (of a UNet): plain | brushnet | controlnet
Case = namedtuple("Case", "id nets fmt B H W twin")      # nets: the side network first, then the UNet it feeds
Step = namedtuple("Step", "name kind opt")

UNET9 = Net("unet", 9, 2, "plain")
BRUSH = (Net("brushnet", 4, 1, "plain"), Net("unet", 4, 1, "brushnet"))
CTRL = (Net("controlnet", 4, 1, "plain"), Net("unet", 4, 1, "controlnet"))

CASES = [
    Case("unet9-2x16x64-bf16", (UNET9,), "bf16", 2, 16, 64, False),
    Case("unet9-2x16x16-bf16", (UNET9,), "bf16", 2, 16, 16, False),
    Case("unet9-2x16x16-bf16-twin", (UNET9,), "bf16", 2, 16, 16, True),
    Case("unet9-3x10x12-bf16", (UNET9,), "bf16", 3, 10, 12, False),
    Case("unet9-2x16x16-fp16", (UNET9,), "fp16", 2, 16, 16, False),
    Case("brushnet-2x16x16-bf16", BRUSH, "bf16", 2, 16, 16, False),
    Case("controlnet-2x16x16-bf16", CTRL, "bf16", 2, 16, 16, False),
]

# what each shape must select: transformer -> form name, and launch names that must / must not occur (the CONDITION of a case)
FORMS = {
    (16, 64): dict(forms={"down_blocks.0.attentions.0": "BLOCK_PRE", "down_blocks.1.attentions.0": "BLOCK",
                          "down_blocks.2.attentions.0": "TWO_GEMM", "mid_block.attentions.0": "CHAIN"},
                   launches=("tfront", "xattn_block", "ff_fused"), absent=("transpose_v",)),
    (16, 16): dict(forms={"down_blocks.0.attentions.0": "BLOCK_PRE", "down_blocks.1.attentions.0": "BLOCK",
                          "down_blocks.2.attentions.0": "CHAIN", "mid_block.attentions.0": "CHAIN"},
                   launches=("tfront", "xattn_block", "ff_fused", "transpose_v"), absent=()),
    (10, 12): dict(forms={"down_blocks.0.attentions.0": "CHAIN", "down_blocks.1.attentions.0": "CHAIN",
                          "down_blocks.2.attentions.0": "CHAIN", "mid_block.attentions.0": "CHAIN"},
                   launches=("transpose_v",), absent=("tfront", "xattn_block", "ff_fused")),
}

DEFECTS = ("temb_row_of_the_next_resnet", "norm2_uses_norm1_affine", "concat_statistics_of_hidden_only",
           "shortcut_tail_drops_skip_half", "conv_shortcut_bias_dropped", "res2_dropped_on_resnet", "down_conv_pads_right_bottom_only",
           "up_nearest_shifted_by_one", "up_odd_target_cropped_not_resampled", "skip0_taken_after_the_brushnet_add",
           "zero_conv_scale_applied_twice", "controlnet_cond_embedding_dropped", "conv_out_statistics_of_previous_block",
           "temb_rows_in_plan_order_of_another_network", "res2_dropped_on_transformer", "transformer_residual_is_normed_input",
           "geglu_halves_swapped", "proj_out_bias_term_of_ff2_missing", "twin_residual_not_wrapped",
           "head_dim_of_another_level_in_attn1_scale", "log2e_prescale_applied_twice", "second_item_reads_first_items_context",
           "pad_context_keys_enter_softmax", "attn2_out_bias_dropped")
INNER = ("t_in", "t_attn1", "t_out1", "t_attn2")
DEFECT_AT = {
    "temb_row_of_the_next_resnet": ("res_a", lambda s: True),
    "norm2_uses_norm1_affine": ("res_b", lambda s: s.opt["cin"] == s.opt["cout"]),
    "concat_statistics_of_hidden_only": ("res_a", lambda s: s.opt["x2"] is not None),
    "shortcut_tail_drops_skip_half": ("res_b", lambda s: s.opt["x2"] is not None),
    "conv_shortcut_bias_dropped": ("res_b", lambda s: s.opt["cin"] != s.opt["cout"]),
    "res2_dropped_on_resnet": ("res_b", lambda s: s.opt["res2"] is not None),
    "down_conv_pads_right_bottom_only": ("down", lambda s: True),
    "up_nearest_shifted_by_one": ("up", lambda s: True),
    "up_odd_target_cropped_not_resampled": ("up", lambda s: True),
    "skip0_taken_after_the_brushnet_add": ("conv_in", lambda s: s.name == "conv_in" and s.opt["brush"]),
    "zero_conv_scale_applied_twice": ("zero", lambda s: True),
    "controlnet_cond_embedding_dropped": ("conv_in", lambda s: s.opt["res2"] == "cond_emb"),
    "conv_out_statistics_of_previous_block": ("eps", lambda s: True),
    "temb_rows_in_plan_order_of_another_network": ("temb", lambda s: True),
    "res2_dropped_on_transformer": ("t_ff", lambda s: s.opt["res2"] is not None),
    "transformer_residual_is_normed_input": ("t_ff", lambda s: True),
    "geglu_halves_swapped": ("t_ff", lambda s: True),
    "proj_out_bias_term_of_ff2_missing": ("t_ff", lambda s: True),
    "twin_residual_not_wrapped": ("t_ff", lambda s: s.name == "down_blocks.0.attentions.0"),
    "head_dim_of_another_level_in_attn1_scale": ("t_attn1", lambda s: True),
    "log2e_prescale_applied_twice": ("t_attn1", lambda s: True),
    "second_item_reads_first_items_context": ("t_attn2", lambda s: True),
    "pad_context_keys_enter_softmax": ("t_attn2", lambda s: True),
    "attn2_out_bias_dropped": ("t_attn2", lambda s: True),
}


def unit(dtype) -> float:
    return NC.unit_roundoff(dtype)


def sizes(H: int, W: int):
    """(h, w) per level: Downsample2D is a 3x3 conv of stride 2 and padding 1, h -> ceil(h / 2)"""
    out = [(H, W)]
    for _ in range(len(BOC) - 1):
        out.append((-(-out[-1][0] // 2), -(-out[-1][1] // 2)))
    return out


# ------------------------------------------------------------------------------------------------ networks, weights, inputs
def make_net(n: Net, dtype=torch.bfloat16):
    from powerpaint_amd.engine import SDNet
    cc = {"brushnet": 5, "controlnet": 3}.get(n.kind, 0)
    return SDNet(n.kind, n.cin, BOC, n.layers, HEADS, CTX_DIM, GROUPS, EPS, conditioning_channels=cc, dtype=dtype)


@lru_cache(maxsize=None)
def state_dict(n: Net):
    """SDNet.synthetic_state_dict with what it leaves trivial made random: norm affines (1, 0) -> (1 + 0.3 N, 0.2 N), biases
    N(0, 0.02) -> N(0, 0.25): an affine or a bias that goes missing must move the output."""
    sd = make_net(n).synthetic_state_dict(seed={"unet": 31, "brushnet": 32, "controlnet": 33}[n.kind] + n.cin)
    g = torch.Generator().manual_seed(77)
    for k in sorted(sd):
        v = sd[k]
        if v.dim() != 1:
            continue
        is_norm = ".norm" in k or k.startswith("conv_norm_out")
        if is_norm and k.endswith(".weight"):
            sd[k] = 1.0 + 0.3 * torch.randn(v.shape, generator=g)
        elif is_norm:
            sd[k] = 0.2 * torch.randn(v.shape, generator=g)
        else:
            sd[k] = 0.25 * torch.randn(v.shape, generator=g)
    return sd


_BW = {}


def block_weights(sd, prefix: str, dtype, to=torch.float64):
    """the block's weights as the HIP path stores them (matrices rounded to the 16-bit format), converted once per block"""
    key = (id(sd), prefix, dtype, to)
    if key not in _BW:
        if len(_BW) > 64:
            _BW.clear()
        _BW[key] = AV.rounded_weights({k: v for k, v in sd.items() if k.startswith(prefix + ".")}, dtype, to=to)
    return _BW[key]


def inputs(c: Case, same_items: bool = False):
    """fp32 NCHW, what the product entry points are given: per network its input channels, the context, the ControlNet image"""
    g = torch.Generator().manual_seed(2000 + c.B * 100 + c.H * 10 + c.W)
    rep = lambda t: t[:1].expand_as(t).contiguous() if (same_items or c.twin) else t      # noqa: E731
    # the context: per-token noise on a component every token shares (3 m, m one N(0, 1) vector), as text embeddings have one:
    # q . k then carries an offset of either sign per (query, head), and where it is negative the real keys' logits lie below
    # the 0 of a zero pad row -- a pad key that enters the softmax takes visible mass there
    d = dict(ctx=torch.randn(c.B, NCTX, CTX_DIM, generator=g) + 3.0 * torch.randn(CTX_DIM, generator=g))
    if same_items:
        d["ctx"] = rep(d["ctx"])
    for n in c.nets:
        cin = n.cin + (5 if n.kind == "brushnet" else 0)
        d["x_" + n.kind] = rep(torch.randn(c.B, cin, c.H, c.W, generator=g))
        if n.kind == "controlnet":
            d["cond"] = rep(torch.rand(c.B, 3, 8 * c.H, 8 * c.W, generator=g))
    return d


# ------------------------------------------------------------------------------------------------ the wiring, by name
def resnet_order(n: Net):
    """(prefix, cin, cout) of every resnet in module order: down, mid, up (the rows of temb_all)"""
    out, oc = [], BOC[0]
    for i, c in enumerate(BOC):
        for j in range(n.layers):
            out.append((f"down_blocks.{i}.resnets.{j}", oc if j == 0 else c, c))
        oc = c
    out += [("mid_block.resnets.0", BOC[-1], BOC[-1]), ("mid_block.resnets.1", BOC[-1], BOC[-1])]
    if n.kind != "controlnet":
        rev = list(reversed(BOC))
        for i, c in enumerate(rev):
            prev, nxt = rev[max(i - 1, 0)], rev[min(i + 1, len(BOC) - 1)]
            for j in range(n.layers + 1):
                out.append((f"up_blocks.{i}.resnets.{j}", (prev if j == 0 else c) + (nxt if j == n.layers else c), c))
    return out


def temb_offsets(n: Net):
    off, o = {}, 0
    for pre, _, cout in resnet_order(n):
        off[pre] = (o, cout)
        o += cout
    return off, o


def zero_names(n: Net):
    nm = n.kind
    cnt = 1 + sum(n.layers + (1 if i != len(BOC) - 1 else 0) for i in range(len(BOC)))
    out = [f"{nm}_down_blocks.{k}" for k in range(cnt)] + [f"{nm}_mid_block"]
    if n.kind == "brushnet":
        cnt = sum(n.layers + 1 + (1 if i != len(BOC) - 1 else 0) for i in range(len(BOC)))
        out += [f"brushnet_up_blocks.{k}" for k in range(cnt)]
    return out


def steps(n: Net, H: int, W: int):
    """The segments of one network in execution order, each with the NAMES of its inputs (taps, or the network's inputs x_in,
    cond_emb, add_down.k / add_mid / add_up.k, ctrl_down.k / ctrl_mid) -- the reference's wiring."""
    S, shape = [], {}
    sz, rev, nl = sizes(H, W), list(reversed(BOC)), len(BOC)
    brush, ctrl = n.wiring == "brushnet", n.wiring == "controlnet"
    it = {"d": 0, "u": 0}

    def nxt(which):
        if not brush:
            return None
        it[which] += 1
        return f"add_{'down' if which == 'd' else 'up'}.{it[which] - 1}"

    def add(name, kind, C, hw, **opt):
        S.append(Step(name, kind, opt))
        shape[name] = (C,) + tuple(hw)
        return name

    def resnet(pre, x, x2, cout, res2):
        cin = shape[x][0] + (shape[x2][0] if x2 else 0)
        hw = shape[x][1:]
        add(pre + ".conv1", "res_a", cout, hw, pre=pre, x=x, x2=x2, cin=cin, cout=cout)
        return add(pre, "res_b", cout, hw, pre=pre, h=pre + ".conv1", x=x, x2=x2, res2=res2, cin=cin, cout=cout)

    def transformer(pre, x, res2):
        C, hw = shape[x][0], shape[x][1:]
        add(pre + ".proj_in", "t_in", C, hw, pre=pre, x=x)
        add(pre + ".attn1", "t_attn1", C, hw, pre=pre, hs=pre + ".proj_in")
        add(pre + ".attn1_out", "t_out1", C, hw, pre=pre, hs=pre + ".proj_in", a=pre + ".attn1")
        add(pre + ".attn2", "t_attn2", C, hw, pre=pre, hs=pre + ".attn1_out")
        return add(pre, "t_ff", C, hw, pre=pre, hs=pre + ".attn2", x=x, res2=res2, c=C)

    add("temb_all", "temb", temb_offsets(n)[1], (1, 1))
    x = add("conv_in", "conv_in", BOC[0], sz[0], x="x_in", res2="cond_emb" if n.kind == "controlnet" else None, brush=brush)
    skips = [x]
    if brush:
        x = add("conv_in.add_sample", "conv_in", BOC[0], sz[0], x="x_in", res2=nxt("d"))
    for i, c in enumerate(BOC):
        attn = i != nl - 1
        for j in range(n.layers):
            r2 = nxt("d")
            x = resnet(f"down_blocks.{i}.resnets.{j}", x, None, c, None if attn else r2)
            if attn:
                x = transformer(f"down_blocks.{i}.attentions.{j}", x, r2)
            skips.append(x)
        if i != nl - 1:
            x = add(f"down_blocks.{i}.downsamplers.0", "down", c, sz[i + 1], x=x, res2=nxt("d"), c=c)
            skips.append(x)
    x = resnet("mid_block.resnets.0", x, None, BOC[-1], None)
    x = transformer("mid_block.attentions.0", x, None)
    x = resnet("mid_block.resnets.1", x, None, BOC[-1], "add_mid" if brush else ("ctrl_mid" if ctrl else None))
    if n.kind == "controlnet":
        for name, f in zip(zero_names(n), skips + [x]):
            add(name, "zero", shape[f][0], shape[f][1:], x=f)
        return S
    if ctrl:
        skips = [add(f"skip_add.{k}", "add", shape[s][0], shape[s][1:], a=s, b=f"ctrl_down.{k}") for k, s in enumerate(skips)]
    down_feats, mid_feat, up_feats = list(skips), x, []
    for i, c in enumerate(rev):
        attn = i != 0
        for j in range(n.layers + 1):
            r2 = nxt("u")
            x = resnet(f"up_blocks.{i}.resnets.{j}", x, skips.pop(), c, None if attn else r2)
            if attn:
                x = transformer(f"up_blocks.{i}.attentions.{j}", x, r2)
            up_feats.append(x)
        if i != nl - 1:
            tgt = shape[skips[-1]][1:]
            x = add(f"up_blocks.{i}.upsamplers.0", "up", c, tgt, x=x, res2=nxt("u"), c=c, size=tgt)
            up_feats.append(x)
    if n.kind == "brushnet":
        for name, f in zip(zero_names(n), down_feats + [mid_feat] + up_feats):
            add(name, "zero", shape[f][0], shape[f][1:], x=f)
        return S
    prev = [s.name for s in S if s.kind in ("res_b", "t_ff")][-2]
    add("eps", "eps", 4, sz[0], x=x, prev=prev)
    return S


def residual_sources(side: Net):
    """input name of the UNet -> zero-conv tap of the side network that feeds it"""
    names = zero_names(side)
    nd = len([k for k in names if "_down_blocks." in k])
    if side.kind == "brushnet":
        m = {f"add_down.{k}": names[k] for k in range(nd)}
        m["add_mid"] = names[nd]
        m.update({f"add_up.{k}": names[nd + 1 + k] for k in range(len(names) - nd - 1)})
        return m
    return dict({f"ctrl_down.{k}": names[k] for k in range(nd)}, ctrl_mid=names[nd])


def tap_names(net, forms, wiring: str):
    """The tap names in plan order from the net's own structure lists (_resnet_specs, _attn_specs, _zero_conv_specs) and the
    form table {transformer: XAttnForm name}: a resnet records .conv1 then itself; a transformer .proj_in, .attn1, then
    .attn1_out unless its form is BLOCK_PRE, .attn2, then itself.  Not derived from `steps`: two derivations, one list."""
    res = [p for p, _, _ in net._resnet_specs()]
    att = {p for p, _ in net._attn_specs()}
    nl, out = len(net.boc), ["temb_all", "conv_in"] + (["conv_in.add_sample"] if wiring == "brushnet" else [])

    def transformer(a):
        return [a + ".proj_in", a + ".attn1"] + ([] if forms[a] == "BLOCK_PRE" else [a + ".attn1_out"]) + [a + ".attn2", a]

    def block(r):
        a = r.replace(".resnets.", ".attentions.")
        return [r + ".conv1", r] + (transformer(a) if a in att else [])

    for i in range(nl):
        for r in res:
            if r.startswith(f"down_blocks.{i}."):
                out += block(r)
        if i != nl - 1:
            out.append(f"down_blocks.{i}.downsamplers.0")
    out += ["mid_block.resnets.0.conv1", "mid_block.resnets.0"] + transformer("mid_block.attentions.0")
    out += ["mid_block.resnets.1.conv1", "mid_block.resnets.1"]
    if net.kind == "controlnet":
        return out + [p for p, _ in net._zero_conv_specs()]
    if wiring == "controlnet":
        out += [f"skip_add.{k}" for k in range(net.skip_count())]
    for i in range(nl):
        for r in res:
            if r.startswith(f"up_blocks.{i}."):
                out += block(r)
        if i != nl - 1:
            out.append(f"up_blocks.{i}.upsamplers.0")
    return out + ([p for p, _ in net._zero_conv_specs()] if net.kind == "brushnet" else ["eps"])


# ------------------------------------------------------------------------------------------------ stages: (ref, gate, E)
Ctx = VC.Ctx


def gn_terms(hw: int, C: int):
    """(eS, eQ, aS, aQ): per term the larger of the statistics launch and of the epilogue accumulators in unknown form"""
    a = NC.stats_eps(hw, C, GROUPS)
    adds = (-(-hw // 16) + 3) * (C // GROUPS)
    b = (min(256, hw) * U32, (min(256, hw) + 1) * U32, adds * 0.5 / NC.SUM_SCALE, adds * 0.5 / NC.SQ_SCALE)
    return tuple(max(p, q) for p, q in zip(a, b))


def s_gn(cx, x, E, gamma, beta, silu: bool, terms, eps: float = EPS):
    """vae_cases.s_gn with the norm's own eps (1e-5 in the resnets and conv_norm_out; vae_cases fixes the VAE's 1e-6): GroupNorm
    (+SiLU) stored in 16 bits, x NCHW float64 with running bound E -> (ref, gate, E of the output)"""
    B, C, H, W = x.shape
    xt = VC._tok(x)
    if not cx.bound:
        return VC._img(NC.ref_groupnorm(xt, None, cx.groups, gamma, beta, eps, silu), H, W), None, None
    ref, own = NC.gate_groupnorm(xt, None, cx.groups, gamma, beta, eps, silu, cx.dtype, terms)
    Ec = None
    if E is not None:
        cg, n = C // cx.groups, H * W * (C // cx.groups)
        _, _, _, mean, var = NC._pop(xt, cx.groups)
        pc = lambda t: NC._per_channel(t, cg)      # noqa: E731
        grp = lambda t: t.reshape(B, H * W, cx.groups, cg)      # noqa: E731
        sigma = pc(torch.sqrt(var + eps))
        xhat = (xt - pc(mean)) / sigma
        Lt, Vt = VC._tok(E[0]), VC._tok(E[1])
        k = (1.1 if silu else 1.0) * gamma.abs() / sigma
        Lc = k * (Lt + pc(grp(Lt).mean((1, 3))) + xhat.abs() * pc(torch.sqrt(grp(Lt * Lt).mean((1, 3)))))
        Vc = 3.0 * k * k * (Vt + pc(grp(Vt).sum((1, 3))) / n ** 2 + xhat ** 2 * pc(grp(xhat ** 2 * Vt).sum((1, 3))) / n ** 2)
        Ec = (Lc, Vc)
    Eo = cx.out(ref, own - cx.u * ref.abs() - cx.sub, 0.0, Ec)
    img = lambda t: VC._img(t, H, W)      # noqa: E731
    return img(ref), img(cx.gate(own, Ec)), (img(Eo[0]), img(Eo[1]))


def conv_terms(cx, x, E, w, **kw):
    """-> (conv without bias, A = its absolute products over the values the kernel may see, what E carries through it)"""
    val = F.conv2d(x, w, None, **kw)
    if not cx.bound:
        return val, None, None
    wa, B = w.abs(), x.shape[0]
    if E is None:
        return val, F.conv2d(x.abs(), wa, None, **kw), None
    both = F.conv2d(torch.cat([x.abs() + cx.tot(E), E[0]]), wa, None, **kw)
    return val, both[:B], (both[B:], F.conv2d(E[1], w * w, None, **kw))


def finish(cx, ref, A, K: int, Ec, store16: bool = True):
    """the GEMM / conv epilogue of vae_cases.s_conv on explicit terms: n_r = K + splits + 5 fp32 roundings of A, one store"""
    if not cx.bound:
        return ref, None, None
    n_r = K + MAX_SPLITS + 5
    own = n_r * U32 * A + ((cx.u * ref.abs() + cx.sub) if store16 else 0.0)
    return ref, cx.gate(own, Ec), cx.out(ref, 0.0, n_r * (U32 * A) ** 2, Ec)


def _v(t):
    return t[None, :, None, None]


def _cat(x, x2):
    return x if x2 is None else torch.cat([x, x2], 1)


def gate_temb(cx, sd, n: Net, t: float, dtype, order=None):
    """-> (temb_all [total] float64, gate): everything fp32, bounds carried linearly"""
    w = AV.rounded_weights({k: v for k, v in sd.items() if k.startswith("time_embedding.") or ".time_emb_proj." in k}, dtype,
                           to=torch.float64)
    half = BOC[0] // 2
    e = -math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half
    a = t * torch.exp(e)
    ts = torch.cat([torch.cos(a), torch.sin(a)])
    d = ((3 * e.abs() + 5) * U32 * a.abs()).repeat(2) + 4 * U32 * ts.abs() + 2.0 ** -149

    def lin(x, dx, wt, b):
        A = (x.abs() + dx) @ wt.abs().t() + b.abs()
        return x @ wt.t() + b, (wt.shape[1] + 7) * U32 * A + dx @ wt.abs().t()

    l1, d1 = lin(ts, d, w["time_embedding.linear_1.weight"], w["time_embedding.linear_1.bias"])
    y1 = NC.silu64(l1)
    l2, d2 = lin(y1, SC.silu_gate(d1, l1, y1), w["time_embedding.linear_2.weight"], w["time_embedding.linear_2.bias"])
    xa = NC.silu64(l2)
    dxa = 1.1 * d2 + (7 + l2.abs()) * U32 * xa.abs()
    names = order or [p for p, _, _ in resnet_order(n)]
    wt = torch.cat([w[p + ".time_emb_proj.weight"] for p in names])
    b = torch.cat([w[p + ".time_emb_proj.bias"] for p in names])
    ref, g = lin(xa, dxa, wt, b)
    return ref, (g if cx.bound else None)


def gate_conv_in(cx, w, x_in, cin0: int, res2):
    """x_in [B, 64, H, W] (pad channels: zeros) -> conv_in (+ res2)"""
    val, A, _ = conv_terms(cx, x_in[:, :cin0], None, w["weight"], padding=1)
    ref = val + _v(w["bias"]) + (0.0 if res2 is None else res2)
    if cx.bound:
        A = A + _v(w["bias"].abs()) + (0.0 if res2 is None else res2.abs())
    return finish(cx, ref, A, 9 * CIN_PAD, None)[:2]


def gate_res_a(cx, w, pre, x, x2, trow):
    xc = _cat(x, x2)
    B, C, H, W = xc.shape
    h1, _, E = s_gn(cx, xc, None, w[pre + ".norm1.weight"], w[pre + ".norm1.bias"], True, gn_terms(H * W, C))
    val, A, Ec = conv_terms(cx, h1, E, w[pre + ".conv1.weight"], padding=1)
    b = w[pre + ".conv1.bias"]
    ref = val + _v(b) + _v(trow)
    if cx.bound:
        A = A + _v(b.abs()) + _v(trow.abs())
    return finish(cx, ref, A, 9 * C, Ec)[:2]


def gate_res_b(cx, w, pre, h, x, x2, res2):
    xc = _cat(x, x2)
    B, C, H, W = h.shape
    h2, _, E = s_gn(cx, h, None, w[pre + ".norm2.weight"], w[pre + ".norm2.bias"], True, gn_terms(H * W, C))
    val, A, Ec = conv_terms(cx, h2, E, w[pre + ".conv2.weight"], padding=1)
    b, K = w[pre + ".conv2.bias"], 9 * C
    if pre + ".conv_shortcut.weight" in w:
        sval, sA, _ = conv_terms(cx, xc, None, w[pre + ".conv_shortcut.weight"])
        b, K = b + w[pre + ".conv_shortcut.bias"], K + xc.shape[1]
        ba = w[pre + ".conv2.bias"].abs() + w[pre + ".conv_shortcut.bias"].abs()
    else:
        sval, sA, ba = xc, xc.abs(), b.abs()
    ref = val + sval + _v(b) + (0.0 if res2 is None else res2)
    if cx.bound:
        A = A + sA + _v(ba) + (0.0 if res2 is None else res2.abs())
    return finish(cx, ref, A, K, Ec)[:2]


def subpix64(x, wf):
    """upconv_cases.subpix_conv in the dtype of its operands, NCHW: x [B, C, H, W], wf [4, Cout, 4 C] -> [B, Cout, 2 H, 2 W]"""
    B, C, H, W = x.shape
    cout = wf.shape[1]
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros(B, cout, 2 * H, 2 * W, dtype=x.dtype)
    for a in (0, 1):
        for b in (0, 1):
            k = wf[2 * a + b].reshape(cout, 2, 2, C).permute(0, 3, 1, 2)
            out[:, :, a::2, b::2] = F.conv2d(xp[:, :, a:a + H + 1, b:b + W + 1], k)
    return out


def folded(w16, dtype, to):
    """the sub-pixel weights as the path stores them: [Cout, C, 3, 3] of 16-bit values -> [4, Cout, 4 C], rounded once more"""
    cout, C = w16.shape[:2]
    return UC.fold(w16.permute(0, 2, 3, 1).reshape(cout, 9 * C), dtype).to(to)


def gate_sampler(cx, w, st, x, res2, dtype, subpix: bool):
    wt, b, C = w["conv.weight"], w["conv.bias"], x.shape[1]
    if st.kind == "down":
        val, A, _ = conv_terms(cx, x, None, wt, stride=2, padding=1)
    elif subpix:
        wf = folded(wt, dtype, torch.float64)
        val, A = subpix64(x, wf), (subpix64(x.abs(), wf.abs()) if cx.bound else None)
    else:
        val, A, _ = conv_terms(cx, F.interpolate(x, size=tuple(st.opt["size"]), mode="nearest"), None, wt, padding=1)
    ref = val + _v(b) + (0.0 if res2 is None else res2)
    if cx.bound:
        A = A + _v(b.abs()) + (0.0 if res2 is None else res2.abs())
    return finish(cx, ref, A, 9 * C, None)[:2]


def gate_zero(cx, w, x, scale: float):
    val, A, _ = conv_terms(cx, x, None, w["weight"])
    ref = (val + _v(w["bias"])) * scale
    if cx.bound:
        A = (A + _v(w["bias"].abs())) * abs(scale)
    return finish(cx, ref, A, x.shape[1], None)[:2]


def gate_add(cx, a, b, dtype):
    ref = (a + b).to(dtype).double()
    return ref, (torch.zeros_like(ref) if cx.bound else None)


def gate_eps(cx, w, x):
    B, C, H, W = x.shape
    h, _, E = s_gn(cx, x, None, w["conv_norm_out.weight"], w["conv_norm_out.bias"], True, gn_terms(H * W, C))
    val, A, Ec = conv_terms(cx, h, E, w["conv_out.weight"], padding=1)
    ref = val + _v(w["conv_out.bias"])
    if cx.bound:
        A = A + _v(w["conv_out.bias"].abs())
    return finish(cx, ref, A, 9 * C, Ec, store16=False)[:2]


def oracle_module(sd, pre, C: int, dtype, to):
    """oracle/sd_modules.py's Transformer2DModel in `to`, on the weights rounded to `dtype` (None: as they are)"""
    from oracle.sd_modules import Transformer2DModel
    m = Transformer2DModel(HEADS, C // HEADS, C, CTX_DIM, groups=GROUPS)
    w = {k: v for k, v in sd.items() if k.startswith(pre + ".")} if dtype is None else block_weights(sd, pre, dtype, to=torch.float32)
    m.load_state_dict({k[len(pre) + 1:]: v for k, v in w.items()})
    return m.to(to).eval()


def oracle_attn1(m, hs):
    """attn1 of the oracle module over norm1(hs), IN FRONT of its to_out (what the plan stores as .attn1); hs NCHW"""
    B, C, H, W = hs.shape
    blk = m.transformer_blocks[0]
    with torch.no_grad():
        x = blk.norm1(VC._tok(hs))
        sp = lambda t: t.view(B, H * W, HEADS, -1).transpose(1, 2)      # noqa: E731
        q, k, v = sp(blk.attn1.to_q(x)), sp(blk.attn1.to_k(x)), sp(blk.attn1.to_v(x))
        p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1]), -1)
        return VC._img((p @ v).transpose(1, 2).reshape(B, H * W, C), H, W)


def oracle_attn2(m, hs, ctx):
    """hs + attn2(norm2(hs), ctx) of the oracle module (to_out and the residual included: what the plan stores as .attn2)"""
    B, C, H, W = hs.shape
    blk = m.transformer_blocks[0]
    with torch.no_grad():
        t = VC._tok(hs)
        return VC._img(t + blk.attn2(blk.norm2(t), ctx.to(t.dtype)), H, W)


def gate_t_in(cx, w, pre, x):
    B, C, H, W = x.shape
    h, _, E = s_gn(cx, x, None, w[pre + ".norm.weight"], w[pre + ".norm.bias"], False, gn_terms(H * W, C), eps=1e-6)
    val, A, Ec = conv_terms(cx, h, E, w[pre + ".proj_in.weight"])
    b = w[pre + ".proj_in.bias"]
    if cx.bound:
        A = A + _v(b.abs())
    return finish(cx, val + _v(b), A, C, Ec)[:2]


def gate_t_out1(cx, w, pre, hs, a):
    tb = pre + ".transformer_blocks.0.attn1.to_out.0"
    val, A, _ = conv_terms(cx, a, None, w[tb + ".weight"][:, :, None, None])
    b = w[tb + ".bias"]
    if cx.bound:
        A = A + _v(b.abs()) + hs.abs()
    return finish(cx, val + _v(b) + hs, A, a.shape[1], None)[:2]


def quads(w):
    """rows [h_0 .. h_F-1 ; g_0 .. g_F-1] -> (h_0, h_1, g_0, g_1, h_2, h_3, g_2, g_3, ...): the GEGLU row order of the packed ff1
    (written here, not taken from the code under test; norm_cases.quad_perm is its inverse)"""
    F2 = w.shape[0] // 2
    i = torch.arange(F2 // 2)
    idx = torch.stack([2 * i, 2 * i + 1, F2 + 2 * i, F2 + 2 * i + 1], 1).reshape(-1)
    return w[idx]


def pack_violations(sd, packed, net_attn, dtype):
    """Every packed tensor the gated transformer segments read, against its composition from the checkpoint tensors in float64
    (SDNet.pack_host composes in fp32 from the unrounded tensors and rounds once): matrices within one 16-bit rounding plus the
    fp32 composition's K u32 of absolute products (+ 2^-25 in fp16: subnormals), vectors and column sums within fp32 accuracy.  -> [(name, worst excess)]"""
    u, bad = unit(dtype), []
    sub = 2.0 ** -25 if dtype == torch.float16 else 0.0      # fp16: weights below 2^-14 are subnormal, half a quantum

    def close(name, got, want, slack):
        r = ((got.double() - want).abs() - slack).max().item()
        if not r <= 0.0 or got.shape != want.shape:
            bad.append((name, r))

    for pre, C in net_attn:
        tb = pre + ".transformer_blocks.0"
        d = lambda k: sd[k].double()      # noqa: E731
        for name, mods, nrm, badd, il in ((tb + ".attn1.qkv", ("attn1.to_q", "attn1.to_k", "attn1.to_v"), "norm1", None, False),
                                          (tb + ".attn2.to_q", ("attn2.to_q",), "norm2", None, False),
                                          (tb + ".ff1", ("ff.net.0.proj",), "norm3", tb + ".ff.net.0.proj.bias", True)):
            W = torch.cat([d(f"{tb}.{m}.weight") for m in mods])
            g, b = d(f"{tb}.{nrm}.weight"), d(f"{tb}.{nrm}.bias")
            o = quads if il else (lambda t: t)
            wf = o(W * g[None, :])
            close(name + ".weight", packed(name + ".weight"), wf, u * wf.abs() + 2 * U32 * wf.abs() + sub)
            w16 = packed(name + ".weight").double()
            close(name + ".colsum", packed(name + ".colsum"), w16.sum(1), (C + 1) * U32 * w16.abs().sum(1))
            t = W @ b + (d(badd) if badd else 0.0)
            close(name + ".bias", packed(name + ".bias"), o(t), (C + 2) * U32 * o(W.abs() @ b.abs() + (d(badd).abs() if badd else 0.0)) + 1e-30)
        Wpo, Wf2 = d(pre + ".proj_out.weight").reshape(C, C), d(tb + ".ff.net.2.weight")
        comp, compa = torch.cat([Wpo @ Wf2, Wpo], 1), torch.cat([Wpo.abs() @ Wf2.abs(), Wpo.abs()], 1)
        close(pre + ".ff2_proj_out.weight", packed(pre + ".ff2_proj_out.weight"), comp, u * comp.abs() + (C + 1) * U32 * compa + sub)
        bc = Wpo @ d(tb + ".ff.net.2.bias") + d(pre + ".proj_out.bias")
        close(pre + ".ff2_proj_out.bias", packed(pre + ".ff2_proj_out.bias"), bc,
              (C + 2) * U32 * (Wpo.abs() @ d(tb + ".ff.net.2.bias").abs() + d(pre + ".proj_out.bias").abs()))
    return bad


def attn_core(cx, q, Eq, k, Ek, v, Ev, scale: float):
    """softmax(q k^T scale) v per head, [B, H, n, d] float64, the operands with running bounds E (None: exact bits) ->
    (o, gate of the stored o, E of it).  Own terms: attention_cases' P3 gate -- u |o| for the denominator, 1e-5 A for the fp32
    score accumulation and exp2, every probability rounded once to 16 bits (u p: carried in quadrature through v, as
    vae_cases carries the rounding of P), the output rounding; the scale is fp32(scale) fp32(log2 e): 3 u32 on the logit."""
    T = lambda m: m.transpose(-1, -2)      # noqa: E731
    s = q @ T(k)
    p = torch.softmax(s * scale, -1)
    o = p @ v
    if not cx.bound:
        return o, None, None
    z = lambda t: (torch.zeros_like(t), torch.zeros_like(t))      # noqa: E731
    Eq, Ek, Ev = Eq or z(q), Ek or z(k), Ev or z(v)
    d = q.shape[-1]
    A_s = (q.abs() + cx.tot(Eq)) @ T(k.abs() + cx.tot(Ek))
    Ls = (Eq[0] @ T(k.abs()) + q.abs() @ T(Ek[0]) + 3 * U32 * s.abs()) * scale
    Vs = (Eq[1] @ T(k * k) + (q * q) @ T(Ek[1]) + (d + MAX_SPLITS + 5) * (U32 * A_s) ** 2) * scale ** 2
    Lp = 1e-5 * p + p * (Ls + (p * Ls).sum(-1, keepdim=True))
    Vp = (cx.u * p) ** 2 + 2.0 * p * p * (Vs + (p * p * Vs).sum(-1, keepdim=True))
    va = v.abs()
    Lo = Lp @ va + p @ Ev[0] + cx.u * o.abs() + (2.0 ** -25 * va.sum(-2, keepdim=True) if cx.sub else 0.0)
    Vo = Vp @ (v * v) + (p * p) @ Ev[1]
    gate = Lo + cx.u * o.abs() + cx.sub + LAMBDA * torch.sqrt(Vo)
    return o, gate, (Lo + cx.sub, Vo + (cx.u * o) ** 2)


def _split_heads(t, B, n):
    return t.reshape(B, n, HEADS, -1).permute(0, 2, 1, 3)


def _merge_heads(t):
    B, H, n, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, n, H * d)


def _folded(cx, rows, w, cs, t, dtype, terms):
    """LayerNorm folded into a GEMM whose output is stored in 16 bits -> (ref, E): norm_cases.gate_folded_ln"""
    tiles = -(-rows.shape[1] // 160)
    if not cx.bound:
        return NC.ref_ln_linear(rows, w, t, 1e-5), None
    ref, g = NC.gate_folded_ln(rows, w, cs, t, 1e-5, tiles, dtype, terms=terms)
    # of the gate's fp32-level part, the K roundings of the accumulation (rstd K u32 A in folded_pre) are carried as every
    # GEMM's are in vae_cases, K (rstd u32 A)^2 in quadrature; the moments' terms and the rest stay linear
    K = rows.shape[1]
    rstd = 1.0 / torch.sqrt(rows.var(-1, unbiased=False, keepdim=True) + 1e-5)
    a1 = rstd * U32 * (rows.abs() @ w.abs().t())
    return ref, ((g - cx.u * ref.abs() - cx.sub - K * a1).clamp_min(0.0), (cx.u * ref) ** 2 + K * a1 * a1)


def _each_item(fn, B):
    """fn(b) -> (ref, gate) per batch item, concatenated (the n x n score matrices of one item at a time)"""
    r = [fn(b) for b in range(B)]
    return torch.cat([a for a, _ in r]), (None if r[0][1] is None else torch.cat([g for _, g in r]))


def gate_t_attn1(cx, pk, hs, dtype):
    """the stored .proj_in -> .attn1: norm1 folded into the QKV GEMM (q, k, v stored in 16 bits; pp_tfront hands q over times
    d^-1/2 log2 e, rounded once all the same), self-attention per head, the output in front of to_out.  The row moments are
    formed in the kernel (pp_tfront: norm_cases.kernel_moments_eps) or by the producer (fewer roundings): the larger terms."""
    w, cs, t = pk
    B, C, H, W = hs.shape
    n = H * W

    def item(b):
        rows = VC._tok(hs[b:b + 1]).reshape(n, C)
        ref, E = _folded(cx, rows, w, cs, t, dtype, NC.kernel_moments_eps())
        part = lambda m, i: _split_heads(m[:, i * C:(i + 1) * C], 1, n)      # noqa: E731
        Es = [None if E is None else (part(E[0], i), part(E[1], i)) for i in range(3)]
        o, g, _ = attn_core(cx, part(ref, 0), Es[0], part(ref, 1), Es[1], part(ref, 2), Es[2], (C // HEADS) ** -0.5)
        return VC._img(_merge_heads(o), H, W), (None if g is None else VC._img(_merge_heads(g), H, W))

    return _each_item(item, B)


def gate_t_attn2(cx, pk, w, pre, hs, ctx, dtype):
    """the stored .attn1_out -> .attn2 in the CHAIN form: norm2 folded into to_q (stored), K and V of the prompt hoisted into the
    setup plan (ctx W^T, stored in 16 bits: (768 + 13) u32 A and one rounding each), attention over the NCTX real keys, to_out +
    bias + the residual."""
    wq, cs, t = pk
    B, C, H, W = hs.shape
    n, tb = H * W, pre + ".transformer_blocks.0.attn2"
    wk, wv, wo, bo = w[tb + ".to_k.weight"], w[tb + ".to_v.weight"], w[tb + ".to_out.0.weight"], w[tb + ".to_out.0.bias"]
    tiles = -(-C // 160)

    def kv(c, wt):
        ref = c @ wt.t()
        if not cx.bound:
            return ref, None
        A = c.abs() @ wt.abs().t()
        return ref, (cx.sub + torch.zeros_like(ref), (CTX_DIM + MAX_SPLITS + 5) * (U32 * A) ** 2 + (cx.u * ref) ** 2)

    def item(b):
        rows = VC._tok(hs[b:b + 1]).reshape(n, C)
        q, Eq = _folded(cx, rows, wq, cs, t, dtype, ((31 + tiles) * U32, (34 + tiles) * U32, 0.0, 0.0))
        (k, Ek), (v, Ev) = kv(ctx[b], wk), kv(ctx[b], wv)
        sp = lambda m, m_n: _split_heads(m, 1, m_n)      # noqa: E731
        spE = lambda E, m_n: None if E is None else (sp(E[0], m_n), sp(E[1], m_n))      # noqa: E731
        o, _, Eo = attn_core(cx, sp(q, n), spE(Eq, n), sp(k, NCTX), spE(Ek, NCTX), sp(v, NCTX), spE(Ev, NCTX), (C // HEADS) ** -0.5)
        o = _merge_heads(o)[0]
        ref = o @ wo.t() + bo + rows
        if not cx.bound:
            return VC._img(ref[None], H, W), None
        Eo = (_merge_heads(Eo[0])[0], _merge_heads(Eo[1])[0])
        A = (o.abs() + cx.tot(Eo)) @ wo.abs().t() + bo.abs() + rows.abs()
        ref, g, _ = finish(cx, ref, A, C, (Eo[0] @ wo.abs().t(), Eo[1] @ (wo * wo).t()))
        return VC._img(ref[None], H, W), VC._img(g[None], H, W)

    return _each_item(item, B)


def ln_carry(rows, E, eps: float = 1e-5):
    """what a running bound E = (L, V) of the rows [n, C] becomes in (x - mean) / sigma: the Jacobian vae_cases carries through
    GroupNorm (d xh_i = (dx_i - mean(dx)) / sigma - xh_i mean(xh dx) / sigma), the population being the row"""
    C = rows.shape[1]
    mean = rows.mean(-1, keepdim=True)
    sigma = torch.sqrt(rows.var(-1, unbiased=False, keepdim=True) + eps)
    xh = (rows - mean) / sigma
    L, V = E
    Lc = (L + L.mean(-1, keepdim=True) + xh.abs() * torch.sqrt((L * L).mean(-1, keepdim=True))) / sigma
    Vc = 3.0 / sigma ** 2 * (V + V.sum(-1, keepdim=True) / C ** 2 + xh ** 2 * (xh ** 2 * V).sum(-1, keepdim=True) / C ** 2)
    return Lc, Vc


def gate_t_attn2_folded(cx, pk, w, pre, hs, ctx, dtype, pre_in=None):
    """the stored .attn1_out -> .attn2 in the folded forms (BLOCK, TWO_GEMM): pp_xattn_fold composes, once per prompt, from the
    STORED K and V (one 16-bit rounding each, as in the chain) G = scale Wq' K_h^T and H = V_h Wo_h, each rounded ONCE more to 16
    bits; the step computes l = LN(x) G^T + g_b (no q is ever stored), p = softmax per head over the real keys, rounded to 16
    bits, out = p H + b_o + x.  Logit terms: norm_cases.folded_pre on G (the fp32 level, linear); the roundings of G, (u G)^2
    through LN(x)^2, and of K, (u k)^2 through q^2, in quadrature.  Output terms: (u H)^2 and V's rounding through Wo^2 under p^2,
    p's own terms as in attn_core, K = 8 x 80 accumulation roundings.  No o is stored: no (u o)^2.
    pre_in = (.proj_in, .attn1), the BLOCK_PRE form: .attn1_out is not stored; the launch forms h = round16(attn1 Wo1^T + b1 +
    proj_in) itself (tblock_cases: "h = round16(x pre_w^T + pre_b + res) is parked in `out`"), takes the row moments from that h
    in the kernel (norm_cases.kernel_moments_eps) and adds it as the residual.  The reference's x is the float64 h; its bound
    E_h = (0, (u h)^2 + (C + 13) (u32 A)^2) -- one accumulation, one rounding -- is carried through the LayerNorm (ln_carry) into
    the logits, L through |G|, V through G^2, and rides the residual add."""
    wq, cs, t = pk
    if pre_in is not None:
        hs0, a1_in = pre_in
        tb1 = pre + ".transformer_blocks.0.attn1.to_out.0"
        wo1, b1 = w[tb1 + ".weight"], w[tb1 + ".bias"]
        hs = hs0
    B, C, H, W = hs.shape
    n, d, tb = H * W, C // HEADS, pre + ".transformer_blocks.0.attn2"
    wk, wv, wo, bo = w[tb + ".to_k.weight"], w[tb + ".to_v.weight"], w[tb + ".to_out.0.weight"], w[tb + ".to_out.0.bias"]
    scale, tiles = d ** -0.5, -(-C // 160)
    wqh, woh = wq.reshape(HEADS, d, C), wo.reshape(C, HEADS, d).permute(1, 0, 2)          # [H, d, C], [H, C, d]

    def item(b):
        rows, Eh = VC._tok(hs[b:b + 1]).reshape(n, C), None
        terms = ((31 + tiles) * U32, (34 + tiles) * U32, 0.0, 0.0)
        if pre_in is not None:
            ar = VC._tok(a1_in[b:b + 1]).reshape(n, C)
            h = ar @ wo1.t() + b1 + rows
            if cx.bound:
                A1 = ar.abs() @ wo1.abs().t() + b1.abs() + rows.abs()
                Eh = (cx.sub + torch.zeros_like(h), (cx.u * h) ** 2 + (C + MAX_SPLITS + 5) * (U32 * A1) ** 2)
            rows, terms = h, NC.kernel_moments_eps()
        k, v = (ctx[b] @ wk.t()).reshape(NCTX, HEADS, d).transpose(0, 1), (ctx[b] @ wv.t()).reshape(NCTX, HEADS, d).transpose(0, 1)
        G = (k @ wqh) * scale                                                             # [H, 77, C]
        gb = (k @ t.reshape(HEADS, d, 1))[..., 0] * scale                                 # [H, 77]
        Hm = v @ woh.transpose(1, 2)                                                      # [H, 77, C]
        Gm = G.reshape(HEADS * NCTX, C)
        if cx.bound:
            l, dz = NC.folded_pre(rows, Gm, Gm.sum(1), gb.reshape(-1), 1e-5, terms)
        else:
            l, dz = NC.ref_ln_linear(rows, Gm, gb.reshape(-1), 1e-5), None
        lh = l.reshape(n, HEADS, NCTX).transpose(0, 1)                                    # [H, n, 77]
        p = torch.softmax(lh, -1)
        ref = (p @ Hm).sum(0) + bo + rows
        if not cx.bound:
            return VC._img(ref[None], H, W), None
        one = torch.ones(C, dtype=torch.float64)
        xh = NC.ref_layernorm(rows, one, 0 * one, 1e-5)
        q = (xh @ wq.t() + t).reshape(n, HEADS, d).transpose(0, 1)                        # what the chain would store, unrounded
        ka = lambda c_, wt: ((CTX_DIM + MAX_SPLITS + 5) * (U32 * (c_.abs() @ wt.abs().t())) ** 2).reshape(NCTX, HEADS, d).transpose(0, 1)      # noqa: E731
        Vk, Vv = ka(ctx[b], wk) + (cx.u * k) ** 2, ka(ctx[b], wv) + (cx.u * v) ** 2      # the stored K, V: accumulation + one rounding
        rstd = 1.0 / torch.sqrt(rows.var(-1, unbiased=False, keepdim=True) + 1e-5)
        a1 = rstd * U32 * (rows.abs() @ Gm.abs().t())                                     # the logits' accumulation: in quadrature
        Ls = (dz - C * a1).clamp_min(0.0).reshape(n, HEADS, NCTX).transpose(0, 1) + 3 * U32 * lh.abs() + cx.sub * (q.abs().sum(-1, keepdim=True)) * scale + cx.sub
        Vs = ((xh * xh) @ ((cx.u * Gm) ** 2).t() + C * a1 * a1).reshape(n, HEADS, NCTX).transpose(0, 1) + \
            ((q * q) @ Vk.transpose(1, 2)) * scale ** 2
        if Eh is not None:
            Lc, Vc = ln_carry(rows, Eh)
            Ls = Ls + (Lc @ Gm.abs().t()).reshape(n, HEADS, NCTX).transpose(0, 1)
            Vs = Vs + (Vc @ (Gm * Gm).t()).reshape(n, HEADS, NCTX).transpose(0, 1)
        Lp = 1e-5 * p + p * (Ls + (p * Ls).sum(-1, keepdim=True))
        Vp = (cx.u * p) ** 2 + 2.0 * p * p * (Vs + (p * p * Vs).sum(-1, keepdim=True))
        woa = woh.abs().transpose(1, 2)                                                   # [H, d, C]
        Lh = cx.sub * woa.sum(1, keepdim=True) + cx.sub + torch.zeros_like(Hm)
        Vh = (cx.u * Hm) ** 2 + Vv @ (woa * woa) + (d + MAX_SPLITS + 5) * (U32 * (v.abs() @ woa)) ** 2
        toth = Lh + LAMBDA * torch.sqrt(Vh)
        A = ((p + Lp + LAMBDA * torch.sqrt(Vp)) @ (Hm.abs() + toth)).sum(0) + bo.abs() + rows.abs()
        Ec = ((Lp @ Hm.abs() + p @ Lh).sum(0), (Vp @ (Hm * Hm) + (p * p) @ Vh).sum(0))
        if Eh is not None:                                                                # the residual is that h
            A, Ec = A + cx.tot(Eh), (Ec[0] + Eh[0], Ec[1] + Eh[1])
        ref, g, _ = finish(cx, ref, A, HEADS * 80, Ec)
        return VC._img(ref[None], H, W), VC._img(g[None], H, W)

    return _each_item(item, B)


def attn_packed(packed, pre, which: str, to=torch.float64):
    name = f"{pre}.transformer_blocks.0.{which}"
    return tuple(packed(name + k).to(to) for k in (".weight", ".colsum", ".bias"))


def ff_packed(packed, pre, to=torch.float64):
    """(w1 [8 C, C] in GEGLU quads with gamma folded in, its column sums, its bias, w2 [C, 5 C], its bias) as the path stores them"""
    tb = pre + ".transformer_blocks.0"
    return tuple(packed(k).to(to) for k in (tb + ".ff1.weight", tb + ".ff1.colsum", tb + ".ff1.bias", pre + ".ff2_proj_out.weight",
                                            pre + ".ff2_proj_out.bias"))


def ff_composed(sd, pre):
    """the same five from the checkpoint tensors in float64, nothing rounded (SDNet.pack_host's algebra): the cross-check's side"""
    tb = pre + ".transformer_blocks.0"
    d = lambda k: sd[k].double()      # noqa: E731
    W1, g3, b3 = d(tb + ".ff.net.0.proj.weight"), d(tb + ".norm3.weight"), d(tb + ".norm3.bias")
    w1 = quads(W1 * g3[None, :])
    t = quads(W1 @ b3 + d(tb + ".ff.net.0.proj.bias"))
    Wpo, Wf2 = d(pre + ".proj_out.weight").reshape(W1.shape[1], -1), d(tb + ".ff.net.2.weight")
    return w1, w1.sum(1), t, torch.cat([Wpo @ Wf2, Wpo], 1), Wpo @ d(tb + ".ff.net.2.bias") + d(pre + ".proj_out.bias")


def gate_t_ff(cx, params, hs, x, res2, dtype):
    """hs = the stored .attn2 [B, C, H, W]; x the transformer's input; -> (ref, gate) of the transformer's output"""
    w1, cs, t, w2, b2 = params
    B, C, H, W = hs.shape
    rows, perm, tiles = VC._tok(hs).reshape(B * H * W, C), NC.quad_perm(8 * C), -(-C // 160)
    if cx.bound:
        terms = ((31 + tiles) * U32, (34 + tiles) * U32, 0.0, 0.0)
        act, g_act = NC.gate_folded_ln(rows, w1[perm], cs[perm], t[perm], 1e-5, tiles, dtype, geglu=True, terms=terms)
    else:
        z = NC.ref_ln_linear(rows, w1[perm], t[perm], 1e-5)
        act = z[:, :4 * C] * NC.gelu64(z[:, 4 * C:])
    w2a, w2b = w2[:, :4 * C], w2[:, 4 * C:]
    add = VC._tok(x).reshape(B * H * W, C) + (0.0 if res2 is None else VC._tok(res2).reshape(B * H * W, C))
    ref = act @ w2a.t() + rows @ w2b.t() + b2 + add
    img = lambda m: VC._img(m.reshape(B, H * W, C), H, W)      # noqa: E731
    if not cx.bound:
        return img(ref), None
    Eg = (g_act - cx.u * act.abs() - cx.sub, (cx.u * act) ** 2)
    A = (act.abs() + cx.tot(Eg)) @ w2a.abs().t() + rows.abs() @ w2b.abs().t() + b2.abs() + VC._tok(x).reshape(B * H * W, C).abs() + \
        (0.0 if res2 is None else VC._tok(res2).reshape(B * H * W, C).abs())
    ref, gate, _ = finish(cx, ref, A, 5 * C, (Eg[0] @ w2a.abs().t(), Eg[1] @ (w2a * w2a).t()))
    return img(ref), img(gate)


def oracle_resnet(w, pre, xc, trow):
    """oracle/sd_modules.py's ResnetBlock2D in float64: time_emb_proj replaced by the given row (weight 0, bias = the row)"""
    from oracle.sd_modules import ResnetBlock2D
    cout = w[pre + ".conv1.weight"].shape[0]
    m = ResnetBlock2D(xc.shape[1], cout, 8, GROUPS, EPS).double()
    sd = {k[len(pre) + 1:]: v for k, v in w.items() if ".time_emb_proj." not in k}
    sd["time_emb_proj.weight"], sd["time_emb_proj.bias"] = torch.zeros(cout, 8, dtype=torch.float64), trow
    m.load_state_dict(sd)
    with torch.no_grad():
        return m(xc, torch.zeros(xc.shape[0], 8, dtype=torch.float64))


class NetIO:
    """What a network's segments read besides taps: x_in [B, 64, H, W], named inputs (cond_emb, add_*, ctrl_*), ctx, t, the
    conditioning scale, which upsamplers ran in the sub-pixel form -- float64 (checks) or float32 (emulation)."""

    def __init__(self, x_in, named, ctx, t=TIMESTEP, scale=1.0, subpix=(), packed=None, twin=False, forms=None):
        self.forms = forms or {}                   # transformer -> XAttnForm name (which form of .attn2 ran)
        self.x_in, self.named, self.ctx, self.t, self.scale, self.subpix = x_in, named, ctx, t, scale, set(subpix)
        self.packed, self.twin = packed, twin      # packed: name -> the ParamPack's tensor (host); twin: the case runs the twin prefix

    def get(self, taps, name):
        if name is None:
            return None
        return self.x_in if name == "x_in" else (self.named[name] if name in self.named else taps[name])


def gate_step(cx, sd, n: Net, st: Step, taps, io: NetIO, dtype):
    """(ref, gate) of tap st.name of network n from the bits of its inputs; None for the ungated kinds when cx.bound"""
    o, g = st.opt, lambda k: io.get(taps, st.opt.get(k))      # noqa: E731
    if st.kind == "temb":
        return gate_temb(cx, sd, n, io.t, dtype)
    if st.kind == "conv_in":
        key = "conv_in_condition" if n.kind == "brushnet" else "conv_in"
        w = {k[len(key) + 1:]: v for k, v in block_weights(sd, key, dtype).items()}
        return gate_conv_in(cx, w, io.x_in, n.cin + (5 if n.kind == "brushnet" else 0), g("res2"))
    if st.kind in ("res_a", "res_b"):
        pre = o["pre"]
        w = block_weights(sd, pre, dtype)
        if st.kind == "res_a":
            off, cout = temb_offsets(n)[0][pre]
            return gate_res_a(cx, w, pre, g("x"), g("x2"), taps["temb_all"][off:off + cout])
        return gate_res_b(cx, w, pre, g("h"), g("x"), g("x2"), g("res2"))
    if st.kind in ("down", "up"):
        w = {k[len(st.name) + 1:]: v for k, v in block_weights(sd, st.name, dtype).items()}
        return gate_sampler(cx, w, st, g("x"), g("res2"), dtype, st.name in io.subpix)
    if st.kind == "zero":
        w = {k[len(st.name) + 1:]: v for k, v in block_weights(sd, st.name, dtype).items()}
        return gate_zero(cx, w, g("x"), io.scale)
    if st.kind == "add":
        return gate_add(cx, g("a"), g("b"), dtype)
    if st.kind == "eps":
        return gate_eps(cx, {k: v for p in ("conv_norm_out", "conv_out") for k, v in block_weights(sd, p, dtype).items()}, g("x"))
    pre = o["pre"]
    if st.kind == "t_in":
        return gate_t_in(cx, block_weights(sd, pre, dtype), pre, g("x"))
    if st.kind == "t_out1":
        return gate_t_out1(cx, block_weights(sd, pre, dtype), pre, g("hs"), g("a"))
    if st.kind == "t_ff":
        return gate_t_ff(cx, ff_packed(io.packed, pre), g("hs"), g("x"), g("res2"), dtype)
    if st.kind == "t_attn1":
        return gate_t_attn1(cx, attn_packed(io.packed, pre, "attn1.qkv"), g("hs"), dtype)
    form, pk, w = io.forms.get(pre, "CHAIN"), attn_packed(io.packed, pre, "attn2.to_q"), block_weights(sd, pre, dtype)
    if form == "BLOCK_PRE":      # .attn1_out is not stored: teacher-forced from (.proj_in, .attn1)
        return gate_t_attn2_folded(cx, pk, w, pre, None, io.ctx, dtype, pre_in=(taps[pre + ".proj_in"], taps[pre + ".attn1"]))
    return (gate_t_attn2 if form == "CHAIN" else gate_t_attn2_folded)(cx, pk, w, pre, g("hs"), io.ctx, dtype)


where_worst = VC.where_worst


def check_chain(n: Net, c: Case, sd, taps, io: NetIO, only=None):
    """Every gated tap of the network against its teacher-forced reference -> [(name, kind, worst ratio, where)]"""
    dtype = FMT[c.fmt]
    cx, out = Ctx(dtype, GROUPS), []
    for st in steps(n, c.H, c.W):
        if only is not None and st.name not in only:
            continue
        if st.kind == "t_out1" and st.name not in taps:      # BLOCK_PRE does not store it (tap_names holds the list to the form)
            continue
        ref, gate = gate_step(cx, sd, n, st, taps, io, dtype)
        got = taps[st.name]
        assert tuple(ref.shape) == tuple(got.shape), (st.name, tuple(ref.shape), tuple(got.shape))
        r, where = where_worst(got.reshape(1, -1) if got.dim() == 1 else got, ref.reshape(1, -1) if ref.dim() == 1 else ref,
                               gate.reshape(1, -1) if gate.dim() == 1 else gate)
        out.append((st.name, st.kind, r, where))
    return out


def free_run(n: Net, c: Case, sd, io: NetIO, cross_check: bool = True):
    """The whole network in float64 from the input bits, every segment on the reference's own outputs -> taps.  Every resnet
    is compared with oracle/sd_modules.py's ResnetBlock2D in float64 on the same input (CROSS_RTOL)."""
    dtype = FMT[c.fmt]
    cx, taps = Ctx(dtype, GROUPS, bound=False), {}
    for st in steps(n, c.H, c.W):
        taps[st.name] = gate_step(cx, sd, n, st, taps, io, dtype)[0]
        if cross_check and st.kind == "res_b":
            o, pre = st.opt, st.opt["pre"]
            off, cout = temb_offsets(n)[0][pre]
            want = oracle_resnet(block_weights(sd, pre, dtype), pre, _cat(io.get(taps, o["x"]), io.get(taps, o["x2"])),
                                 taps["temb_all"][off:off + cout])
            if o["res2"] is not None:
                want = want + io.get(taps, o["res2"])
            assert torch.allclose(taps[st.name], want, rtol=CROSS_RTOL, atol=CROSS_RTOL * float(want.abs().max())), pre
        if cross_check and st.kind in ("t_attn1", "t_attn2"):
            o, pre, got = st.opt, st.opt["pre"], taps[st.name]
            hs, C, tb = io.get(taps, o["hs"]), got.shape[1], st.opt["pre"] + ".transformer_blocks.0"
            d = lambda k: sd[k].double()      # noqa: E731
            m = oracle_module(sd, pre, C, None, torch.float64)
            if st.kind == "t_attn1":               # the formula on the unrounded fold against the oracle on the raw weights
                Wc, gm, bt = torch.cat([d(f"{tb}.attn1.to_{x}.weight") for x in "qkv"]), d(tb + ".norm1.weight"), d(tb + ".norm1.bias")
                mine, want = gate_t_attn1(cx, (Wc * gm[None, :], None, Wc @ bt), hs, dtype)[0], oracle_attn1(m, hs)
            else:
                Wc, gm, bt = d(tb + ".attn2.to_q.weight"), d(tb + ".norm2.weight"), d(tb + ".norm2.bias")
                raw = {k: v.double() for k, v in sd.items() if k.startswith(pre + ".")}
                fn = gate_t_attn2 if io.forms.get(pre, "CHAIN") == "CHAIN" else gate_t_attn2_folded
                mine, want = fn(cx, (Wc * gm[None, :], None, Wc @ bt), raw, pre, hs, io.ctx, dtype)[0], oracle_attn2(m, hs, io.ctx)
            assert torch.allclose(mine, want, rtol=CROSS_RTOL, atol=CROSS_RTOL * float(want.abs().max())), (pre, st.kind)
        if cross_check and st.kind in ("t_in", "t_out1", "t_ff"):
            o, pre, got = st.opt, st.opt["pre"], taps[st.name]
            g = lambda k: io.get(taps, o.get(k))      # noqa: E731
            C = got.shape[1]
            with torch.no_grad():
                if st.kind == "t_ff":                 # the formula on the unrounded composition against the oracle on the raw weights
                    m = oracle_module(sd, pre, C, None, torch.float64)
                    blk, t = m.transformer_blocks[0], VC._tok(g("hs"))
                    want = m.proj_out(VC._img(t + blk.ff(blk.norm3(t)), *got.shape[2:])) + g("x") + (0.0 if g("res2") is None else g("res2"))
                    got = gate_t_ff(cx, ff_composed(sd, pre), g("hs"), g("x"), g("res2"), dtype)[0]
                else:
                    m = oracle_module(sd, pre, C, dtype, torch.float64)
                    want = m.proj_in(m.norm(g("x"))) if st.kind == "t_in" else \
                        g("hs") + VC._img(m.transformer_blocks[0].attn1.to_out[0](VC._tok(g("a"))), *got.shape[2:])
            assert torch.allclose(got, want, rtol=CROSS_RTOL, atol=CROSS_RTOL * float(want.abs().max())), (pre, st.kind)
    return taps


def e2e(got, ref):
    """(cosine, max-abs / bound) under the gate of tests/test_models_gpu.py: cosine >= 0.999, max-abs <= 3e-2 max(1, max|ref|)"""
    cos = F.cosine_similarity(got.flatten(), ref.flatten(), dim=0).item()
    return cos, ((got - ref).abs().max() / (3e-2 * max(1.0, float(ref.abs().max())))).item()


def outputs_of(n: Net, taps):
    """the network's outputs among its taps: eps, or the zero convs in output order"""
    return [taps["eps"]] if n.kind == "unet" else [taps[k] for k in zero_names(n)]


# ------------------------------------------------------------------------------------------------ emulation
r16 = VC.r16


def e_gn(x, gamma, beta, silu, dtype, groups, stats_of=None, eps: float = EPS):
    """vae_cases.e_gn with the norm's own eps: statistics (of `stats_of`, default x) in float64, scale / shift in fp32, one rounding"""
    B, C, H, W = x.shape
    sx = (x if stats_of is None else stats_of).double().reshape(B, groups, -1)
    mean, var = sx.mean(-1), sx.var(-1, unbiased=False)
    rstd = (1.0 / torch.sqrt(var + eps)).float().repeat_interleave(C // groups, 1)[:, :, None, None]
    mean = mean.float().repeat_interleave(C // groups, 1)[:, :, None, None]
    sc = rstd * gamma.float()[None, :, None, None]
    y = x.float() * sc + (beta.float()[None, :, None, None] - mean * sc)
    return r16(F.silu(y) if silu else y, dtype)


def emu_temb(sd, n: Net, t: float, dtype, defect=None):
    w = AV.rounded_weights({k: v for k, v in sd.items() if k.startswith("time_embedding.") or ".time_emb_proj." in k}, dtype)
    half = BOC[0] // 2
    a = torch.tensor(t, dtype=torch.float32) * torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
    ts = torch.cat([torch.cos(a), torch.sin(a)])
    y = F.silu(F.linear(ts, w["time_embedding.linear_1.weight"], w["time_embedding.linear_1.bias"]))
    y = F.silu(F.linear(y, w["time_embedding.linear_2.weight"], w["time_embedding.linear_2.bias"]))
    names = [p for p, _, _ in resnet_order(n)]
    if defect == "temb_rows_in_plan_order_of_another_network":      # the up path's rows in front of the mid block's
        names = [p for p in names if not p.startswith("mid_block")] + [p for p in names if p.startswith("mid_block")]
    return F.linear(y, torch.cat([w[p + ".time_emb_proj.weight"] for p in names]), torch.cat([w[p + ".time_emb_proj.bias"] for p in names]))


def emu_conv_in(w, x_in, cin0, res2, dtype, defect=None, extra=None):
    y = F.conv2d(x_in[:, :cin0].float(), w["weight"].float(), w["bias"].float(), padding=1)
    if res2 is not None and defect != "controlnet_cond_embedding_dropped":
        y = y + res2.float()
    if defect == "skip0_taken_after_the_brushnet_add":
        y = y + extra.float()
    return r16(y, dtype)


def _gn_hidden_only(x, x2, gamma, beta, dtype):
    """norm1 over concat(x, x2) with accumulators that only the hidden tensor's producer filled: the sums of x2 are missing"""
    return e_gn(_cat(x, x2), gamma, beta, True, dtype, GROUPS, stats_of=_cat(x, torch.zeros_like(x2)))


def emu_res_a(w, pre, x, x2, temb_all, n: Net, dtype, defect=None):
    off, cout = temb_offsets(n)[0][pre]
    if defect == "temb_row_of_the_next_resnet":
        off = off + cout if off + 2 * cout <= temb_all.numel() else off - cout
    if defect == "concat_statistics_of_hidden_only":
        h1 = _gn_hidden_only(x, x2, w[pre + ".norm1.weight"], w[pre + ".norm1.bias"], dtype)
    else:
        h1 = e_gn(_cat(x, x2), w[pre + ".norm1.weight"], w[pre + ".norm1.bias"], True, dtype, GROUPS)
    y = F.conv2d(h1, w[pre + ".conv1.weight"].float(), w[pre + ".conv1.bias"].float(), padding=1)
    return r16(y + _v(temb_all[off:off + cout].float()), dtype)


def emu_res_b(w, pre, h, x, x2, res2, dtype, defect=None):
    nrm = "norm1" if defect == "norm2_uses_norm1_affine" else "norm2"
    h2 = e_gn(h, w[f"{pre}.{nrm}.weight"], w[f"{pre}.{nrm}.bias"], True, dtype, GROUPS)
    y = F.conv2d(h2, w[pre + ".conv2.weight"].float(), w[pre + ".conv2.bias"].float(), padding=1)
    xc = _cat(x, x2).float()
    if pre + ".conv_shortcut.weight" in w:
        ws, bs = w[pre + ".conv_shortcut.weight"].float(), w[pre + ".conv_shortcut.bias"].float()
        if defect == "shortcut_tail_drops_skip_half":
            xc, ws = x.float(), ws[:, :x.shape[1]]
        y = y + F.conv2d(xc, ws, None if defect == "conv_shortcut_bias_dropped" else bs)
    else:
        y = y + xc
    if res2 is not None and defect != "res2_dropped_on_resnet":
        y = y + res2.float()
    return r16(y, dtype)


def emu_sampler(w, st, x, res2, dtype, subpix: bool, defect=None):
    wt, b = w["conv.weight"], w["conv.bias"].float()
    if st.kind == "down":
        if defect == "down_conv_pads_right_bottom_only":
            y = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), wt.float(), b, stride=2)
        else:
            y = F.conv2d(x.float(), wt.float(), b, stride=2, padding=1)
    else:
        H, W = x.shape[-2:]
        th, tw = st.opt["size"]
        if defect is None and subpix:
            y = subpix64(x.float(), folded(wt, dtype, torch.float32)) + _v(b)
        else:
            if defect == "up_odd_target_cropped_not_resampled":
                iy, ix = torch.arange(th) // 2, torch.arange(tw) // 2
            else:
                sh = 1 if defect == "up_nearest_shifted_by_one" else 0
                iy = ((torch.arange(th) * H + sh * H) // th).clamp_max(H - 1)      # F.interpolate(nearest): floor(i * H / th)
                ix = ((torch.arange(tw) * W + sh * W) // tw).clamp_max(W - 1)
            y = F.conv2d(x.float()[:, :, iy][:, :, :, ix], wt.float(), b, padding=1)
    return r16(y if res2 is None else y + res2.float(), dtype)


def emu_step(sd, n: Net, st: Step, taps, io: NetIO, dtype, defect=None):
    """The emulation's tap st.name from the emulation's own earlier taps, float32 values"""
    o, g = st.opt, lambda k: io.get(taps, st.opt.get(k))      # noqa: E731
    bw = lambda p: block_weights(sd, p, dtype, to=torch.float32)      # noqa: E731
    strip = lambda p: {k[len(p) + 1:]: v for k, v in bw(p).items()}      # noqa: E731
    if st.kind == "temb":
        return emu_temb(sd, n, io.t, dtype, defect)
    if st.kind == "conv_in":
        extra = io.named.get("add_down.0") if defect == "skip0_taken_after_the_brushnet_add" else None
        return emu_conv_in(strip("conv_in_condition" if n.kind == "brushnet" else "conv_in"), io.x_in,
                           n.cin + (5 if n.kind == "brushnet" else 0), g("res2"), dtype, defect, extra)
    if st.kind == "res_a":
        return emu_res_a(bw(o["pre"]), o["pre"], g("x"), g("x2"), taps["temb_all"], n, dtype, defect)
    if st.kind == "res_b":
        return emu_res_b(bw(o["pre"]), o["pre"], g("h"), g("x"), g("x2"), g("res2"), dtype, defect)
    if st.kind in ("down", "up"):
        return emu_sampler(strip(st.name), st, g("x"), g("res2"), dtype, st.name in io.subpix, defect)
    if st.kind == "zero":
        w = strip(st.name)
        s = io.scale * (io.scale if defect == "zero_conv_scale_applied_twice" else 1.0)
        return r16(F.conv2d(g("x").float(), w["weight"].float(), w["bias"].float()) * s, dtype)
    if st.kind == "add":
        return r16(g("a").float() + g("b").float(), dtype)
    if st.kind == "eps":
        src = taps[o["prev"]] if defect == "conv_out_statistics_of_previous_block" else None
        h = e_gn(g("x"), sd["conv_norm_out.weight"], sd["conv_norm_out.bias"], True, dtype, GROUPS, stats_of=src)
        w = bw("conv_out")
        return F.conv2d(h, w["conv_out.weight"].float(), w["conv_out.bias"].float(), padding=1)
    pre = o["pre"]
    if st.kind == "t_in":
        w = bw(pre)
        h = e_gn(g("x"), w[pre + ".norm.weight"], w[pre + ".norm.bias"], False, dtype, GROUPS, eps=1e-6)
        return r16(F.conv2d(h, w[pre + ".proj_in.weight"], w[pre + ".proj_in.bias"]), dtype)
    if st.kind == "t_out1":
        w, tb = bw(pre), pre + ".transformer_blocks.0.attn1.to_out.0"
        return r16(F.conv2d(g("a").float(), w[tb + ".weight"][:, :, None, None], w[tb + ".bias"]) + g("hs").float(), dtype)
    if st.kind == "t_ff":
        return emu_t_ff(ff_packed(io.packed, pre, torch.float32), bw(pre), pre, g("hs"), g("x"), g("res2"), dtype, io.twin, defect)
    if st.kind == "t_attn1":
        return emu_t_attn1(attn_packed(io.packed, pre, "attn1.qkv", torch.float32), g("hs"), dtype, defect)
    fn = emu_t_attn2 if io.forms.get(pre, "CHAIN") == "CHAIN" else emu_t_attn2_folded      # (BLOCK_PRE: hs is the emulation's own .attn1_out, the rounded h)
    return fn(attn_packed(io.packed, pre, "attn2.to_q", torch.float32), bw(pre), pre, g("hs"), io.ctx, dtype, defect)


def emu_t_attn2_folded(pk, w, pre, hs, ctx, dtype, defect=None):
    """BLOCK / TWO_GEMM: G and H composed in fp32 from the stored (rounded) K and V and rounded once more, 80 key slots per head
    of which the NCTX real ones enter the softmax; p rounded to 16 bits; no q, no o stored"""
    wq, cs, t = pk
    B, C, H, W = hs.shape
    n, d, tb = H * W, C // HEADS, pre + ".transformer_blocks.0.attn2"
    wqh = wq.reshape(HEADS, d, C)
    woh = w[tb + ".to_out.0.weight"].reshape(C, HEADS, d).permute(1, 0, 2)
    c = ctx.float()
    if defect == "second_item_reads_first_items_context":
        c = c[:1].expand_as(c)
    slots = 80 if defect == "pad_context_keys_enter_softmax" else NCTX
    c = F.pad(c, (0, 0, 0, slots - NCTX))
    out = []
    for b in range(B):
        rows = VC._tok(hs[b:b + 1].float()).reshape(n, C)
        k = r16(c[b] @ w[tb + ".to_k.weight"].t(), dtype).reshape(slots, HEADS, d).transpose(0, 1)
        v = r16(c[b] @ w[tb + ".to_v.weight"].t(), dtype).reshape(slots, HEADS, d).transpose(0, 1)
        G = r16((k @ wqh) * d ** -0.5, dtype).reshape(HEADS * slots, C)
        gb = ((k @ t.reshape(HEADS, d, 1))[..., 0] * d ** -0.5).reshape(-1)
        Hm = r16(v @ woh.transpose(1, 2), dtype)
        mean = rows.double().mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(rows.double().var(-1, unbiased=False, keepdim=True) + 1e-5)
        l = rstd.float() * (rows @ G.t() - mean.float() * G.sum(1)) + gb
        p = r16(torch.softmax(l.reshape(n, HEADS, slots).transpose(0, 1), -1), dtype)
        y = (p @ Hm).sum(0) + rows
        if defect != "attn2_out_bias_dropped":
            y = y + w[tb + ".to_out.0.bias"]
        out.append(y)
    return r16(VC._img(torch.stack(out), H, W), dtype)


def _emu_folded(rows, w, cs, t, dtype):
    mean = rows.double().mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(rows.double().var(-1, unbiased=False, keepdim=True) + 1e-5)
    return r16(rstd.float() * (rows @ w.t() - mean.float() * cs) + t, dtype)


def _emu_attn(q, k, v, scale, dtype, cols=None):
    """the flash form: exp(s - max) rounded to 16 bits, numerator and denominator from the rounded values, one output rounding;
    cols: the key columns that enter the softmax (default all)"""
    s = (q @ k.transpose(-1, -2)) * scale
    e = r16(torch.exp(s - s.max(-1, keepdim=True).values), dtype)
    return r16((e @ v) / e.sum(-1, keepdim=True), dtype)


def emu_t_attn1(pk, hs, dtype, defect=None):
    w, cs, t = pk
    B, C, H, W = hs.shape
    n, d = H * W, C // HEADS
    z = _emu_folded(VC._tok(hs.float()).reshape(B * n, C), w, cs, t, dtype)
    q, k, v = (_split_heads(z[:, i * C:(i + 1) * C], B, n) for i in range(3))
    if defect == "head_dim_of_another_level_in_attn1_scale":
        d = 2 * d if d < 160 else d // 2
    scale = d ** -0.5 * (1.4426950408889634 if defect == "log2e_prescale_applied_twice" else 1.0)
    return VC._img(_merge_heads(_emu_attn(q, k, v, scale, dtype)), H, W)


def emu_t_attn2(pk, w, pre, hs, ctx, dtype, defect=None):
    """CHAIN: K / V rows of the prompt padded with zero rows to a multiple of 8 (80); the softmax reads the NCTX real ones"""
    wq, cs, t = pk
    B, C, H, W = hs.shape
    n, tb = H * W, pre + ".transformer_blocks.0.attn2"
    rows = VC._tok(hs.float()).reshape(B * n, C)
    q = _split_heads(_emu_folded(rows, wq, cs, t, dtype), B, n)
    c = ctx.float()
    if defect == "second_item_reads_first_items_context":
        c = c[:1].expand_as(c)
    pad = F.pad(c, (0, 0, 0, 80 - NCTX)) if defect == "pad_context_keys_enter_softmax" else c
    k = _split_heads(r16(pad @ w[tb + ".to_k.weight"].t(), dtype), B, pad.shape[1])
    v = _split_heads(r16(pad @ w[tb + ".to_v.weight"].t(), dtype), B, pad.shape[1])
    o = _merge_heads(_emu_attn(q, k, v, (C // HEADS) ** -0.5, dtype)).reshape(B * n, C)
    y = o @ w[tb + ".to_out.0.weight"].t() + rows
    if defect != "attn2_out_bias_dropped":
        y = y + w[tb + ".to_out.0.bias"]
    return r16(VC._img(y.reshape(B, n, C), H, W), dtype)


def emu_t_ff(params, w, pre, hs, x, res2, dtype, twin: bool, defect=None):
    """norm3's moments in float64 applied in fp32, the GEGLU value rounded once, one GEMM over [g | hs], one store"""
    w1, cs, t, w2, b2 = params
    B, C, H, W = hs.shape
    rows, perm = VC._tok(hs.float()).reshape(B * H * W, C), NC.quad_perm(8 * C)
    mean = rows.double().mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(rows.double().var(-1, unbiased=False, keepdim=True) + 1e-5)
    z = rstd.float() * (rows @ w1[perm].t() - mean.float() * cs[perm]) + t[perm]
    a, gt = (z[:, 4 * C:], z[:, :4 * C]) if defect == "geglu_halves_swapped" else (z[:, :4 * C], z[:, 4 * C:])
    act = r16(a * F.gelu(gt), dtype)
    if defect == "transformer_residual_is_normed_input":
        x = e_gn(x, w[pre + ".norm.weight"], w[pre + ".norm.bias"], False, dtype, GROUPS, eps=1e-6)
    xr = VC._tok(x.float()).reshape(B * H * W, C).clone()
    if defect == "twin_residual_not_wrapped" and twin:      # rows of the second half read past the half tensor that was stored
        xr[B * H * W // 2:] = 0.0
    if defect == "proj_out_bias_term_of_ff2_missing":
        b2 = w[pre + ".proj_out.bias"]
    y = act @ w2[:, :4 * C].t() + rows @ w2[:, 4 * C:].t() + b2 + xr
    if res2 is not None and defect != "res2_dropped_on_transformer":
        y = y + VC._tok(res2.float()).reshape(B * H * W, C)
    return r16(VC._img(y.reshape(B, H * W, C), H, W), dtype)


def emu_cond_emb(sd, cond, dtype):
    """the ControlNet conditioning embedding (the setup plan's output): conv + SiLU chain, every layer stored in 16 bits"""
    ce = "controlnet_cond_embedding"
    w = block_weights(sd, ce, dtype, to=torch.float32)
    conv = lambda nm, x, s=1: F.conv2d(x, w[f"{ce}.{nm}.weight"], w[f"{ce}.{nm}.bias"], stride=s, padding=1)      # noqa: E731
    e = r16(F.silu(conv("conv_in", r16(cond.float(), dtype))), dtype)
    for i in range(3):
        e = r16(F.silu(conv(f"blocks.{2 * i}", e)), dtype)
        e = r16(F.silu(conv(f"blocks.{2 * i + 1}", e, 2)), dtype)
    return r16(conv("conv_out", e), dtype)


def default_subpix(n: Net, H: int, W: int):
    """the upsamplers the emulation runs in the sub-pixel form: those whose target is exactly twice the source (the product's
    choice is read from the plan and asserted in the GPU file; the gates hold for either form of the weights it names)"""
    sz = sizes(H, W)
    return {f"up_blocks.{i}.upsamplers.0" for i in range(len(BOC) - 1)
            if n.kind != "controlnet" and sz[len(BOC) - 2 - i] == (2 * sz[len(BOC) - 1 - i][0], 2 * sz[len(BOC) - 1 - i][1])}


@lru_cache(maxsize=None)
def host_packed(n: Net, fmt: str):
    """name -> tensor of the network's ParamPack, packed on the host as load_state_dict packs it"""
    net = make_net(n, FMT[fmt])
    net.load_state_dict(state_dict(n), "cpu")
    return net.params.tensor


def emulate(c: Case, inp=None):
    """The faithful chain of every network of the case -> {kind: (net, sd, taps float32, NetIO float32)}"""
    dtype, inp, out, feed = FMT[c.fmt], inp or inputs(c), {}, {}
    for n in c.nets:
        sd = state_dict(n)
        x = F.pad(r16(inp["x_" + n.kind], dtype), (0, 0, 0, 0, 0, CIN_PAD - inp["x_" + n.kind].shape[1]))
        named = dict(feed)
        if n.kind == "controlnet":
            named["cond_emb"] = emu_cond_emb(sd, inp["cond"], dtype)
        io = NetIO(x, named, r16(inp["ctx"], dtype), scale=SCALE if n.kind != "unet" else 1.0, subpix=default_subpix(n, c.H, c.W),
                   packed=host_packed(n, c.fmt), twin=c.twin, forms=forms_of(dry_runtime(n, c)[0], c))
        taps = {}
        for st in steps(n, c.H, c.W):
            taps[st.name] = emu_step(sd, n, st, taps, io, dtype)
        out[n.kind] = (n, sd, taps, io)
        if n.kind != "unet":
            feed = {k: taps[v] for k, v in residual_sources(n).items()}
    return out


def io64(io: NetIO):
    d = lambda t: t.double() if torch.is_tensor(t) else t      # noqa: E731
    return NetIO(d(io.x_in), {k: d(v) for k, v in io.named.items()}, d(io.ctx), io.t, io.scale, io.subpix, io.packed, io.twin, io.forms)


# ------------------------------------------------------------------------------------------------ dry builds (CPU)
def dry_runtime(n: Net, c: Case):
    """The network compiled as NetRuntime.ensure compiles it, on a host arena and without weights (no launch is made) ->
    (rt, [(ptr, nbytes)] of the final arena in allocation order)"""
    from powerpaint_amd import engine
    from powerpaint_amd.runtime import NetRuntime
    net = make_net(n, FMT[c.fmt])
    net.load_state_dict(net.synthetic_state_dict(meta=True), "cpu", materialize=False)
    rt = NetRuntime(net, "cpu")
    wiring = ("plain",)
    if n.wiring != "plain":
        sh = rt._residual_shapes(c.B, c.H, c.W, with_up=n.wiring == "brushnet")
        wiring = (n.wiring, {k: [0] * len(v) for k, v in sh.items()})
    log, alloc = [], engine.Arena.alloc

    def logged(self, nbytes):
        ptr = alloc(self, nbytes)
        log.append((self, ptr, nbytes))
        return ptr

    engine.Arena.alloc = logged
    try:
        rt.ensure(c.B, c.H, c.W, NCTX, net.cin0, wiring, cond_hw=(8 * c.H, 8 * c.W) if n.kind == "controlnet" else None,
                  scale=SCALE if n.kind != "unet" else 1.0, twin=c.twin)
    finally:
        engine.Arena.alloc = alloc
    return rt, [(p, nb) for a, p, nb in log if a is rt.arena]


def forms_of(rt, c: Case):
    return {p: f.name for p, (f, _) in rt.net.xattn_forms(rt.lib, c.B, c.H, c.W, NCTX).items()}


def form_violations(rt, c: Case):
    """the CONDITION of a case: the forms and launches its shape must select are the ones in the plan (FORMS)"""
    want, bad = FORMS[(c.H, c.W)], []
    forms, names = forms_of(rt, c), [call[2] for call in rt.step_plan.calls]
    bad += [(p, forms.get(p), f) for p, f in want["forms"].items() if forms.get(p) != f]
    bad += [("missing launch", nm) for nm in want["launches"] if nm not in names]
    bad += [("unexpected launch", nm) for nm in want["absent"] if nm in names]
    return bad


def block_taps(taps):
    return [t for t in taps if len(t) == 2]


def inner_tap_violations(rt):
    """every tensor recorded inside a block is written by the call it names: the call is in the plan, and the tensor is the
    output of its PPGemmArgs or one of its pointer arguments"""
    bad, calls = [], rt.step_plan.calls
    for t in rt.lay["taps"]:
        if len(t) != 3:
            continue
        name, act, call = t
        if not any(call is k for k in calls):
            bad.append((name, "its call is not in the plan"))
            continue
        a = getattr(call[1][0], "_obj", None) if call[1] else None
        outs = [a.out] if a is not None and hasattr(a, "out") else [v for v in call[1] if isinstance(v, int)]
        if act.ptr not in outs:
            bad.append((name, f"{call[2]} does not write it"))
    return bad
