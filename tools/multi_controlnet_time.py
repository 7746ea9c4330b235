#!/usr/bin/env python
"""Time the ControlNet inpainting call with one net, two nets, and two nets with net 0's window closed after half the steps.

Config-4 shape by default: batch 4, CFG 7.5, 512x512 (64x64 latents), bf16, 50 DDIM steps, random-init weights and the
synthetic inputs of bench.py (same seeds).  The three variants are built once and timed ALTERNATING, `--reps` rounds of one
pipeline call each behind `--warmup` untimed calls per variant (graphs captured, code objects loaded), host clock around
work that ends in a device synchronise; every round's figure is printed so the spread can be seen.  A record, not a gate:

    python tools/multi_controlnet_time.py > profiles/multi_controlnet_time.txt

What to expect if the launch plan is right: "one" equals `bench.py --config controlnet` of the same
build on the same box; "two" adds about what "one" adds over `bench.py --config v1` (no add launches, no extra pass over
the residuals); "two, net 0 closed at half" sits about midway between "one" and "two".
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-gpu", type=int, default=4)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--denoise-steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--tiny", action="store_true", help="reduced networks (a rehearsal of the script, not a measurement)")
    args = ap.parse_args()

    import bench
    from powerpaint_amd import _lib as L, models as PM, pipelines as PP, schedulers as PS
    dev = "cuda:0"
    torch.cuda.set_device(0)
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]
    net_kw = dict(dtype=dtype)
    if args.tiny:
        net_kw.update(block_out_channels=(320, 640), layers_per_block=1,
                      down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
                      up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"))
    unet = PM.UNet2DConditionModel(in_channels=9, device=dev, **net_kw)
    cn_kw = {k: v for k, v in net_kw.items() if k != "up_block_types"}
    nets = [PM.ControlNetModel(in_channels=4, device=dev, **cn_kw) for _ in range(2)]
    for i, m in enumerate([unet] + nets):
        m.load_state_dict(m.net.synthetic_state_dict(device=dev, seed=i))
    kw = bench.synthetic_inputs("controlnet", dev, 0, args.per_gpu, args.latent, args.denoise_steps)
    img = kw.pop("control_image")
    kw.pop("controlnet_conditioning_scale")
    g = torch.Generator().manual_seed(77)
    img2 = torch.rand(img.shape, generator=g).to(dev)

    def pipe(cn):
        return PP.StableDiffusionControlNetInpaintPipeline(unet=unet, controlnet=cn, scheduler=PS.DDIMScheduler())

    variants = [
        ("one net", pipe(nets[0]), dict(control_image=img, controlnet_conditioning_scale=0.5)),
        ("two nets", pipe(nets), dict(control_image=[img, img2], controlnet_conditioning_scale=[0.5, 0.8])),
        ("two nets, net 0 closed at half", pipe(nets),
         dict(control_image=[img, img2], controlnet_conditioning_scale=[0.5, 0.8], control_guidance_start=[0.0, 0.0],
              control_guidance_end=[0.5, 1.0])),
    ]
    print(f"build {L.lib().pp_build_id().decode()}  device {torch.cuda.get_device_name(0)}  batch {args.per_gpu} CFG 7.5 "
          f"{args.latent * 8}x{args.latent * 8} {args.dtype} {args.denoise_steps} DDIM steps, hipGraph replay"
          f"{'  (TINY networks: rehearsal)' if args.tiny else ''}")
    for name, p, extra in variants:
        for _ in range(args.warmup):
            out = p(**kw, **extra)[0]
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        loop = p._loop
        sets = {k: len(v.program[False].calls) for k, v in loop._sets.items()} if loop._multi else None
        print(f"{name}: launches per step {len(loop.program.calls)}, twin prefix UNet {loop.rt.twin} nets "
              f"{[r.twin for r in loop.side_rts]}" + (f", launches per active set {sets}" if sets else ""))
    times = {name: [] for name, _, _ in variants}
    for r in range(args.reps):
        for name, p, extra in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p(**kw, **extra)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / args.denoise_steps)
    for name, _, _ in variants:
        v = times[name]
        print(f"{name}: ms per denoise step, per round {[round(x, 3) for x in v]}  median {statistics.median(v):.3f}  "
              f"min {min(v):.3f}  max {max(v):.3f}")
    one, two, half = (statistics.median(times[n]) for n, _, _ in variants)
    print(f"second net adds {two - one:.3f} ms per step; closing net 0 at half gives back {two - half:.3f} ms "
          f"({(two - half) / max(two - one, 1e-9):.2f} of one net's cost; 0.5 expected)")
    for _, p, _ in variants:
        p._loop.flush_faults()


if __name__ == "__main__":
    main()
