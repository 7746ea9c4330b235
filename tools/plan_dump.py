#!/usr/bin/env python
"""usage: tools/plan_dump.py OUT [TREE] -- every launch of the compiled plans on a CPU arena, no GPU: launch names in order, every
field of each PPGemmArgs and every scalar argument of the other launches, pointers as offsets into the arena (A+) or the
packed weights (W+), and per plan the FLOP accounting (flops, flops_skipped, flops_by_kind) and the arena's peak.
In full text: both UNets (the 4-channel one behind a BrushNet), BrushNet and ControlNet, setup and step plans, twin prefix
asked for and not, at 64x64 latents batch 8 and 16x16 batch 2; the full UNet at batch 2 at 32x32, 16x8 (twin), 8x8, 29x32 and
13x10, and in fp16 at 64x64; the plans of the three VAE runtimes (VAENet; AsymVAENet at the x-1-5 widths in bf16 and fp16 and at
the small widths of the tests; TinyVAENet at both block counts of the tests in bf16 and fp16), each as the runtime's own `_build`
compiles it on a dry arena, with the tap names in plan order, and per VAE network a sha256 of the packed parameter bytes and one
of its (name, offset) table.  As one sha256 line per case: the full UNet at batch 2 with every one and every
pair of the transformer switches taken off on the instance, at 64x64, 32x32, 29x32 and 13x10, twin asked for and not, and with
the wide cross-attention block let up to C = 1280.  Two trees whose dumps are equal byte for byte compile the same plans
(TREE: the checkout to import from, default this one): how a change to the plan compiler shows that it leaves them alone."""
import hashlib
import itertools
import os
import sys

out = sys.argv[1]
tree = sys.argv[2] if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, tree)
import torch
from powerpaint_amd import _lib as L
from powerpaint_amd.engine import SDNet
from powerpaint_amd.runtime import NetRuntime
from powerpaint_amd.vae import VAENet, VAERuntime
from powerpaint_amd.vae_asym import AsymVAENet, AsymVAERuntime
from powerpaint_amd.vae_tiny import TinyVAENet, TinyVAERuntime
from powerpaint_amd.engine import Arena
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))      # the case files (data only)
import asym_vae_cases as AV
import taesd_cases as TC

SWITCHES = ("fold_ln", "merge_ff2_proj_out", "fuse_xattn", "fuse_tfront", "fuse_xattn_pre", "fuse_ff", "ff_w8", "attn_log2",
            "fuse_xattn_wide", "fuse_xattn_2g")

RANGES = []
def norm(x):
    if not isinstance(x, int) or isinstance(x, bool):
        return x
    for tag, lo, hi in RANGES:
        if lo <= x < hi:
            return f"{tag}+{x - lo}"
    return x

def desc(plan):
    rows = []
    for fn, args, name in plan.calls:
        a = getattr(args[0], "_obj", None) if args else None
        if isinstance(a, L.PPGemmArgs):
            f = []
            for fld, typ in L.PPGemmArgs._fields_:
                v = getattr(a, fld)
                if typ is L.vp:
                    v = None if not v else norm(v)
                elif hasattr(v, "__len__"):
                    v = [norm(x) if x else 0 for x in v]
                f.append(f"{fld}={v}")
            rows.append(name + " " + " ".join(f))
        else:
            rows.append(name + " " + " ".join(str(norm(x)) if not hasattr(x, '_obj') else 'ref' for x in args))
    return rows

def totals(plan):
    kinds = " ".join(f"{k}={v!r}" for k, v in sorted(plan.flops_by_kind.items()))
    return f"flops={plan.flops!r} flops_skipped={plan.flops_skipped!r} by_kind: {kinds}"

def compiled(kind, cin, cfg, B, H, W, twin, off=(), **attrs):
    """-> lines of the setup and the step plan of one network, built as NetRuntime builds them."""
    net = SDNet(kind, cin, **cfg)
    for name in off:
        setattr(net, name, False)
    for name, v in attrs.items():
        setattr(net, name, v)
    net.load_state_dict(net.synthetic_state_dict(meta=True), "cpu", materialize=False)
    rt = NetRuntime(net, "cpu")
    wiring = ("plain",)
    if kind == "unet" and cin == 4:
        sh = rt._residual_shapes(B, H, W, with_up=True)
        wiring = ("brushnet", {k: [0] * len(v) for k, v in sh.items()})
    rt.ensure(B, H, W, 77, net.cin0, wiring, cond_hw=(8 * H, 8 * W) if kind == "controlnet" else None, twin=twin)
    base, pb_ = rt.arena.base, net.params.buf
    RANGES[:] = [("A", base, base + rt.arena.size + 4096), ("W", pb_.data_ptr(), pb_.data_ptr() + pb_.numel() + 4096)]
    rows = []
    for tag, plan in (("setup", rt.setup_plan), ("step", rt.step_plan)):
        rows.append(f"## {kind} cin={cin} {net.dtype} B={B} {H}x{W} twin={twin} {tag}: {len(plan.calls)} launches")
        rows += desc(plan)
        rows.append(f"# {tag} {totals(plan)}")
    rows.append(f"# arena peak={rt.arena.peak}")
    return rows

lines = []
n_full = 0
NETS = (("unet", 9, {}), ("unet", 4, {}), ("brushnet", 4, dict(conditioning_channels=5)), ("controlnet", 4, dict(conditioning_channels=3)))
full = [(kind, cin, cfg, B, hw, hw, twin) for (B, hw) in ((8, 64), (2, 16)) for kind, cin, cfg in NETS for twin in (False, True)]
full += [("unet", 9, {}, 2, H, W, twin) for H, W, twin in ((32, 32, False), (16, 8, True), (8, 8, False), (29, 32, False), (13, 10, False))]
full += [("unet", 9, dict(dtype=torch.float16), 2, 64, 64, False)]
for case in full:
    lines += compiled(*case)
    n_full += 2
# VAE: every runtime's own _build on a dry arena, and per network the packed bytes and the offset table as digests
def vae_net(tag, net):
    net.load_state_dict(net.synthetic_state_dict(seed=1), "cpu")
    buf = net.params.buf
    table = repr(sorted((k, p - buf.data_ptr()) for k, p in net.P.items()))
    lines.append(f"## {tag}")
    lines.append(f"sha256 {hashlib.sha256(buf.numpy().tobytes()).hexdigest()} {tag} params.buf, {buf.numel()} bytes")
    lines.append(f"sha256 {hashlib.sha256(table.encode()).hexdigest()} {tag} offsets of {len(net.P)} entries")
    return net

def vae_plan(tag, rt_cls, net, direction, B, H, W):
    global n_full
    dry = Arena()
    lay, plan = rt_cls(net, "cpu", direction)._build(dry, B, H, W)
    buf = net.params.buf
    RANGES[:] = [("A", dry.base, dry.base + (1 << 40)), ("W", buf.data_ptr(), buf.data_ptr() + buf.numel() + 4096)]
    lines.append(f"## {tag} {direction} B={B} {H}x{W}: {len(plan.calls)} launches, taps {' '.join(t[0] for t in lay['taps'])}")
    lines.extend(desc(plan))
    lines.append(f"# {totals(plan)} peak={dry.peak}")
    n_full += 1

n_nets = 0
net = vae_net("vae", VAENet()); n_nets += 1
for h, w in ((16, 16), (13, 10)):
    vae_plan("vae", VAERuntime, net, "decode", 2, h, w)
    vae_plan("vae", VAERuntime, net, "encode", 2, 8 * h, 8 * w)
# TINY's encoder has two levels, the runtime's moments are sized for four (the factor 8): only its decode directions
for name, cfg, dtype, dirs in (("X15", AV.X15, torch.bfloat16, ("encode", "decode", "decode_cond")),
                               ("X15", AV.X15, torch.float16, ("encode", "decode", "decode_cond")),
                               ("TINY", AV.TINY, torch.bfloat16, ("decode", "decode_cond"))):
    tag = f"asym {name} {dtype}"
    net = vae_net(tag, AsymVAENet(cfg["in_channels"], cfg["out_channels"], cfg["latent_channels"], cfg["down"], cfg["layers_down"],
                                  cfg["up"], cfg["layers_up"], cfg["groups"], dtype=dtype)); n_nets += 1
    for h, w in ((8, 8), (5, 7)):
        for d in dirs:
            vae_plan(tag, AsymVAERuntime, net, d, 2, *((8 * h, 8 * w) if d == "encode" else (h, w)))
for name, cfg in (("default", TC.DEFAULT), ("SMALL", TC.SMALL)):
    for dtype in (torch.bfloat16, torch.float16):
        tag = f"taesd {name} {dtype}"
        net = vae_net(tag, TinyVAENet(cfg["in_channels"], cfg["out_channels"], cfg["latent_channels"], cfg["enc_blocks"],
                                      cfg["dec_blocks"], dtype=dtype)); n_nets += 1
        vae_plan(tag, TinyVAERuntime, net, "decode", 2, *TC.DECODE_SHAPES[0])
        vae_plan(tag, TinyVAERuntime, net, "encode", 2, *TC.ENCODE_SHAPES[0])
# switched-off plans, one digest line each
n_digest = 0
def digest(tag, *a, **kw):
    global n_digest
    text = "\n".join(compiled("unet", 9, {}, 2, *a, **kw))
    lines.append(f"sha256 {hashlib.sha256(text.encode()).hexdigest()} {tag}")
    n_digest += 1

for (H, W) in ((64, 64), (32, 32), (29, 32), (13, 10)):
    for twin in (False, True):
        for off in itertools.chain(((),), itertools.combinations(SWITCHES, 1), itertools.combinations(SWITCHES, 2)):
            digest(f"{H}x{W} twin={twin} off={','.join(off) or '-'}", H, W, twin, off)
for hw in (64, 32, 16):
    digest(f"{hw}x{hw} twin=False xattn_wide_max_c=1280", hw, hw, False, xattn_wide_max_c=1280)
open(out, "w").write("\n".join(lines) + "\n")
print(len(lines), "lines,", n_full, "full-text plans,", n_nets, "VAE networks (2 digests each),", n_digest, "digest cases, library",
      L.build_id())
