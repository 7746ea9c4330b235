#!/usr/bin/env python
"""usage: tools/plan_dump.py OUT [TREE] -- every launch of the compiled plans on a CPU arena, no GPU: launch names in order, every
field of each PPGemmArgs and every scalar argument of the other launches, pointers as offsets into the arena (A+) or the
packed weights (W+).  Both UNets (the 4-channel one behind a BrushNet), BrushNet and ControlNet, setup and step plans, twin
prefix asked for and not, at 64x64 latents batch 8 and 16x16 batch 2, and the VAE plans.  Two trees whose dumps are equal
byte for byte compile the same plans (TREE: the checkout to import from, default this one): how a change to the plan
compiler shows that it leaves the shipped shapes alone."""
import os
import sys

out = sys.argv[1]
tree = sys.argv[2] if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, tree)
from powerpaint_amd import _lib as L
from powerpaint_amd.engine import SDNet
from powerpaint_amd.runtime import NetRuntime
from powerpaint_amd.vae import VAENet
from powerpaint_amd.engine import Arena, Builder, Act


RANGES = []
def norm(x):
    if not isinstance(x, int) or isinstance(x, bool):
        return x
    for tag, lo, hi in RANGES:
        if lo <= x < hi:
            return f"{tag}+{x - lo}"
    return x

def desc(plan, base):
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

lines = []
for (B, hw) in ((8, 64), (2, 16)):
    for kind, cin, cfg in (("unet", 9, {}), ("unet", 4, {}), ("brushnet", 4, dict(conditioning_channels=5)), ("controlnet", 4, dict(conditioning_channels=3))):
        for twin in (False, True):
            net = SDNet(kind, cin, **cfg)
            net.load_state_dict(net.synthetic_state_dict(meta=True), "cpu", materialize=False)
            rt = NetRuntime(net, "cpu")
            wiring = ("plain",)
            if kind == "unet" and cin == 4:
                sh = rt._residual_shapes(B, hw, hw, with_up=True)
                wiring = ("brushnet", {k: [0] * len(v) for k, v in sh.items()})
            rt.ensure(B, hw, hw, 77, net.cin0, wiring, cond_hw=(8 * hw, 8 * hw) if kind == "controlnet" else None, twin=twin)
            base = rt.arena.base
            pb_ = net.params.buf
            RANGES[:] = [("A", base, base + rt.arena.size + 4096), ("W", pb_.data_ptr(), pb_.data_ptr() + pb_.numel() + 4096)]
            pbase = 0
            for tag, plan in (("setup", rt.setup_plan), ("step", rt.step_plan)):
                lines.append(f"## {kind} cin={cin} B={B} {hw}x{hw} twin={twin} {tag}: {len(plan.calls)} launches")
                lines += desc(plan, min(base, pbase))
# VAE
net = VAENet(); net.load_state_dict(net.synthetic_state_dict(seed=1), "cpu")
for hw in (64, 16):
    dry = Arena(); pb = Builder(dry)
    net.build_decode(pb, Act(dry.alloc(hw * hw * 16), 1, hw, hw, 8), dry.alloc(4 * 64 * hw * hw * 4))
    RANGES[:] = [("A", dry.base, dry.base + (1 << 40)), ("W", net.params.buf.data_ptr(), net.params.buf.data_ptr() + net.params.buf.numel() + 4096)]
    lines.append(f"## vae decode {hw}"); lines += desc(pb.plan, dry.base)
    dry = Arena(); pb = Builder(dry)
    net.build_encode(pb, Act(dry.alloc(64 * hw * hw * 16), 1, 8 * hw, 8 * hw, 8))
    lines.append(f"## vae encode {hw}"); lines += desc(pb.plan, dry.base)
open(out, "w").write("\n".join(lines) + "\n")
print(len(lines), "lines")
