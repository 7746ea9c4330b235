#!/usr/bin/env python
"""usage: tools/loop_dump.py OUT [TREE] -- the step programs `DenoiseLoop.bind` assembles, on tiny networks on the GPU (`bind`
allocates there; no denoise step runs).  Per case: the launches of `loop.program.calls` in order with their entry points, every
scalar argument and every field of each ctypes struct (PPGemmArgs) verbatim, every address replaced by its order of first
appearance within the case -- two runs whose buffers sit elsewhere compare equal, a mis-wired pointer does not -- and
`program.flops`.  Cases: the eleven scheduler classes x {UNet alone, BrushNet + 4-channel UNet, one ControlNet, two ControlNets
whose guidance windows differ (the program of every active set)} x CFG on / off; DDIM at eta = 0.5; the 4-channel blend for DDIM,
LCM, Euler a and Heun; guess mode with a ControlNet; a duck-typed scheduler; each refusal as one line carrying the error text;
DeepCache on every configuration (the shallow program next to the full one; two ControlNets: per set); perturbed-attention
guidance and guidance_rescale, alone and together; a MultiControlNetModel around one net; keep_closed_nets.
Two trees whose dumps are equal byte for byte bind the same programs (TREE: the checkout to import from, default this one)."""
import ctypes
import os
import sys

out = sys.argv[1]
tree = sys.argv[2] if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, tree)
import torch
from powerpaint_amd import _lib as L
from powerpaint_amd import models as PM, pipelines as PP, schedulers as PS
from powerpaint_amd.engine import DeepCache
from powerpaint_amd.pipelines._loop import DenoiseLoop

DEV = "cuda:0"
TINY = dict(block_out_channels=(320, 640), layers_per_block=1, down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
            up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"))
NO_UP = {k: v for k, v in TINY.items() if k != "up_block_types"}
SD15 = dict(timestep_spacing="leading", steps_offset=1)
CLASSES = [("DDIMScheduler", {}), ("DPMSolverMultistepScheduler", {}), ("PNDMScheduler", {}), ("UniPCMultistepScheduler", {}),
           ("LCMScheduler", {}), ("EulerDiscreteScheduler", SD15), ("EulerAncestralDiscreteScheduler", SD15),
           ("HeunDiscreteScheduler", SD15), ("KDPM2DiscreteScheduler", SD15), ("KDPM2AncestralDiscreteScheduler", SD15),
           ("LMSDiscreteScheduler", SD15)]
B, S, STEPS = 2, 8, 4


class Duck:
    """A scheduler outside the package: the diffusers protocol, nothing else."""
    order, init_noise_sigma = 1, 1.0

    def __init__(self):
        self.timesteps = torch.tensor([801, 601, 401, 201])

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step(self, model_output, timestep, sample, generator=None, return_dict=True):
        return (sample - 0.1 * model_output,)


def describe(program):
    """One line per launch; addresses (integers from 2^32 up, pointer fields of a struct) numbered by first appearance."""
    seen = {}

    def norm(x, pointer=False):
        if isinstance(x, bool) or not isinstance(x, int) or (x < (1 << 32) and not (pointer and x)):
            return repr(x)
        return f"@{seen.setdefault(x, len(seen))}"

    def fields(obj):
        parts = []
        for fld, typ in obj._fields_:
            v = getattr(obj, fld)
            if isinstance(v, ctypes.Array):
                parts.append(f"{fld}=[{','.join(norm(0 if x is None else x) for x in v)}]")
            else:
                parts.append(f"{fld}={norm(0 if v is None else v, pointer=typ is L.vp)}")
        return "{" + " ".join(parts) + "}"

    rows = []
    for fn, args, name in program.calls:
        cells = [fields(a._obj) if hasattr(a, "_obj") else norm(a) for a in args]
        rows.append(f"{name} {getattr(fn, '__name__', '?')} " + " ".join(cells))
    rows.append(f"# flops={program.flops!r} launches={len(program.calls)}")
    return rows


def net(cls, seed, **kw):
    m = cls(device=DEV, **kw)
    return m.load_state_dict(m.net.synthetic_state_dict(device=DEV, seed=seed))


torch.cuda.set_device(0)
unet9 = net(PM.UNet2DConditionModel, 0, in_channels=9, **TINY)
unet4 = net(PM.UNet2DConditionModel, 1, in_channels=4, **TINY)
brush = net(PM.BrushNetModel, 2, in_channels=4, conditioning_channels=5, **TINY)
cnets = [net(PM.ControlNetModel, 3 + i, in_channels=4, **NO_UP) for i in range(2)]
g = torch.Generator().manual_seed(0)
mask = torch.zeros(B, 1, S, S)
mask[:, :, 2:6, 1:5] = 1
mil = (torch.randn(B, 4, S, S, generator=g) * 0.5).to(DEV)
mask = mask.to(DEV)
cond5 = torch.cat([mil, mask], 1)
imgs = [torch.rand(B, 3, 8 * S, 8 * S, generator=g).to(DEV) for _ in cnets]
blend = (torch.randn(1, 4, S, S, generator=g), mask[:1, :1].cpu(), torch.randn(B, 4, S, S, generator=g))
ROWS = PP.StableDiffusionControlNetInpaintPipeline.control_schedule(STEPS, [0.5, 0.8], [0.0, 0.25], [0.5, 0.75])
assert len({tuple(k for k, v in enumerate(r) if v != 0.0) for r in ROWS}) > 2, ROWS


def pe(do_cfg):
    return torch.randn((2 if do_cfg else 1) * B, 77, 768, generator=torch.Generator().manual_seed(5)).to(DEV)


def scheduler(name, opts):
    sch = getattr(PS, name)(**opts) if name != "Duck" else Duck()
    if name != "Duck":
        sch.set_timesteps(STEPS, device=DEV)
    return sch


def set_programs(loop, active, deep):
    """-> (full, shallow or None): the programs of one set of active ControlNets, its row of scales written."""
    ent = loop._entry(active)
    if deep and ent.program[True] is None:
        loop._build(ent, True)
    loop._set_scales(ent, next((r for r in ROWS if tuple(k for k, v in enumerate(r) if v != 0.0) == active), [0.5, 0.8]))
    return ent.program


def bound(config, sch, do_cfg, deep=False, keep_closed_nets=False, **kw):
    """-> [(tag, program)] of one bind; deep: DeepCache on every network, the shallow program behind each full one."""
    for m in [unet9, unet4, brush] + cnets:
        m.net.deepcache = DeepCache(0, 2) if deep else None
    p, shape, v1 = pe(do_cfg), (B, 4, S, S), [(mask, 4), (mil, 5)]
    if config == "unet":
        loop = DenoiseLoop(unet9, sch).bind(shape, do_cfg, 7.5, p, static_inputs=v1, **kw)
    elif config == "unet4":
        loop = DenoiseLoop(unet4, sch).bind(shape, do_cfg, 7.5, p, **kw)
    elif config == "brushnet":
        loop = DenoiseLoop(unet4, sch, side=brush, side_kind="brushnet").bind(
            shape, do_cfg, 7.5, p, prompt_embeds_side=p, side_static_inputs=[(cond5, 4)], side_scale=0.9, **kw)
    elif config == "controlnet":
        loop = DenoiseLoop(unet9, sch, side=cnets[0], side_kind="controlnet").bind(
            shape, do_cfg, 7.5, p, prompt_embeds_side=p, static_inputs=v1, controlnet_cond=imgs[0], side_scale=0.7, **kw)
    elif config == "wrapped controlnet":
        loop = DenoiseLoop(unet9, sch, side=PM.MultiControlNetModel(cnets[:1]), side_kind="controlnet").bind(
            shape, do_cfg, 7.5, p, prompt_embeds_side=p, static_inputs=v1, controlnet_cond=imgs[:1], side_scale=[0.7], **kw)
    else:
        loop = DenoiseLoop(unet9, sch, side=PM.MultiControlNetModel(cnets), side_kind="controlnet",
                           keep_closed_nets=keep_closed_nets).bind(
            shape, do_cfg, 7.5, p, prompt_embeds_side=p, static_inputs=v1, controlnet_cond=imgs, side_scale=[0.5, 0.8], **kw)
        sets = sorted({tuple(k for k, v in enumerate(r) if v != 0.0) for r in ROWS} | {(0, 1)})
        progs = [(f"set {k}", set_programs(loop, k, deep)) for k in sets]
        return [(tag + sfx, pr) for tag, pair in progs for sfx, pr in zip(("", " shallow"), pair) if pr is not None]
    return [("", loop.program)] + ([(" shallow", loop.program_shallow)] if deep else [])


lines, n_cases = [], 0


def case(tag, config, name, opts, do_cfg, env=None, **kw):
    global n_cases
    n_cases += 1
    saved = {k: os.environ.get(k) for k in env or {}}
    os.environ.update(env or {})
    try:
        for sub, program in bound(config, scheduler(name, opts), do_cfg, **kw):
            lines.append(f"## {tag} {sub}".rstrip())
            lines.extend(describe(program))
    except L.PPError as e:
        lines.append(f"## {tag}: refused: {e}")
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


for name, opts in CLASSES:
    for config in ("unet", "brushnet", "controlnet", "two controlnets"):
        for do_cfg in (True, False):
            case(f"{name} {config} cfg={do_cfg}", config, name, opts, do_cfg)
for do_cfg in (True, False):
    case(f"DDIMScheduler eta=0.5 unet cfg={do_cfg}", "unet", "DDIMScheduler", {}, do_cfg, eta=0.5,
         generator=torch.Generator().manual_seed(1))
for name, opts in (CLASSES[0], CLASSES[4], CLASSES[6], CLASSES[7]):
    case(f"{name} unet4 blend cfg=True", "unet4", name, opts, True, blend=blend)
for do_cfg in (True, False):
    case(f"DDIMScheduler controlnet guess_mode cfg={do_cfg}", "controlnet", "DDIMScheduler", {}, do_cfg, guess_mode=True)
for config in ("unet", "controlnet"):
    case(f"duck-typed scheduler {config} cfg=True", config, "Duck", {}, True)
case("KDPM2DiscreteScheduler unet4 blend", "unet4", "KDPM2DiscreteScheduler", SD15, True, blend=blend)
case("EulerDiscreteScheduler unet PP_LAB=1 PP_TEMB_TABLE=0", "unet", "EulerDiscreteScheduler", SD15, True,
     env=dict(PP_LAB="1", PP_TEMB_TABLE="0"))
ALL = ("unet", "brushnet", "controlnet", "two controlnets")
for name, opts in (CLASSES[0], CLASSES[4], CLASSES[6], CLASSES[7]):
    for config in ALL:
        for do_cfg in (True, False):
            case(f"{name} {config} cfg={do_cfg} DeepCache", config, name, opts, do_cfg, deep=True)
for config in ("unet", "controlnet", "two controlnets"):
    case(f"duck-typed scheduler {config} cfg=True DeepCache", config, "Duck", {}, True, deep=True)
for config in ALL:
    for do_cfg in (True, False):
        case(f"DDIMScheduler {config} cfg={do_cfg} pag", config, "DDIMScheduler", {}, do_cfg, pag_scale=3.0, pag_adaptive_scale=0.1)
for name, opts in (CLASSES[0], CLASSES[6]):
    for config in ALL:
        for pag_scale in (0.0, 3.0):
            case(f"{name} {config} guidance_rescale pag_scale={pag_scale}", config, name, opts, True, guidance_rescale=0.7,
                 pag_scale=pag_scale)
case("duck-typed scheduler two controlnets cfg=True", "two controlnets", "Duck", {}, True)
for do_cfg in (True, False):
    case(f"DDIMScheduler wrapped controlnet cfg={do_cfg}", "wrapped controlnet", "DDIMScheduler", {}, do_cfg)
    case(f"DDIMScheduler two controlnets keep_closed_nets cfg={do_cfg}", "two controlnets", "DDIMScheduler", {}, do_cfg,
         keep_closed_nets=True)
case("DDIMScheduler wrapped controlnet DeepCache", "wrapped controlnet", "DDIMScheduler", {}, True, deep=True)
case("DDIMScheduler two controlnets keep_closed_nets DeepCache", "two controlnets", "DDIMScheduler", {}, True, deep=True,
     keep_closed_nets=True)
assert sum(": refused: " in ln for ln in lines) == 2, "both refusals were to be met, and nothing else refused"
open(out, "w").write("\n".join(lines) + "\n")
print(len(lines), "lines,", n_cases, "cases,", sum(ln.startswith("## ") for ln in lines), "programs and refusals, library",
      L.build_id())
