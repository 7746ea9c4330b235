#!/usr/bin/env python
"""What FreeU costs per denoising step: the headline configuration with `unet.enable_freeu(0.9, 0.2, 1.5, 1.6)` against the
same build without it.

Headline shape by default: ppt-v1, batch 4, CFG 7.5, 512x512 (64x64 latents), bf16, 50 DDIM steps, random-init weights and the
synthetic inputs of bench.py (same seeds).  Two UNets with the same weights, one with FreeU on, are built once and timed
ALTERNATING, `--reps` rounds of one pipeline call each behind `--warmup` untimed calls per variant (graphs captured, code
objects loaded), host clock around work that ends in a device synchronise; every round's figure is printed so the spread can
be seen.  Then one step of the FreeU variant is replayed eagerly with a HIP event pair around every launch (five times, the
median per launch is kept) for the six pp_freeu launch times.  A record, not a gate:

    python tools/freeu_cost.py > profiles/freeu_cost.txt

The expectation to confirm or refute (DESIGN.md "FreeU"): the step grows by the six small launches and by nothing else.
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
    ap.add_argument("--reps", type=int, default=5)
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
        net_kw.update(block_out_channels=(320, 320, 640, 640), layers_per_block=1)
    unets = [PM.UNet2DConditionModel(in_channels=9, device=dev, **net_kw) for _ in range(2)]
    for m in unets:
        m.load_state_dict(m.net.synthetic_state_dict(device=dev, seed=0))
    unets[1].enable_freeu(s1=0.9, s2=0.2, b1=1.5, b2=1.6)
    kw = bench.synthetic_inputs("v1", dev, 0, args.per_gpu, args.latent, args.denoise_steps)
    variants = [(name, PP.StableDiffusionInpaintPipeline(unet=u, scheduler=PS.DDIMScheduler()))
                for name, u in zip(("FreeU off", "FreeU on"), unets)]
    print(f"build {L.lib().pp_build_id().decode()}  device {torch.cuda.get_device_name(0)}  ppt-v1 batch {args.per_gpu} CFG 7.5 "
          f"{args.latent * 8}x{args.latent * 8} {args.dtype} {args.denoise_steps} DDIM steps, hipGraph replay"
          f"{'  (TINY networks: rehearsal)' if args.tiny else ''}")
    for name, p in variants:
        for _ in range(args.warmup):
            out = p(**kw)[0]
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        names = [c[2] for c in p._loop.program.calls]
        print(f"{name}: launches per step {len(names)} (freeu {names.count('freeu')}, groupnorm_stats "
              f"{names.count('groupnorm_stats')}), twin prefix {p._loop.rt.twin}")
    times = {name: [] for name, _ in variants}
    for r in range(args.reps):
        for name, p in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p(**kw)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / args.denoise_steps)
    for name, _ in variants:
        v = times[name]
        print(f"{name}: ms per denoise step, per round {[round(x, 3) for x in v]}  median {statistics.median(v):.3f}  "
              f"min {min(v):.3f}  max {max(v):.3f}")
    off, on = (statistics.median(times[n]) for n, _ in variants)
    spread = max(max(v) - min(v) for v in times.values())
    # the six launches, eagerly, an event pair around each (an event pair adds a few microseconds of its own to a launch)
    loop = variants[1][1]._loop
    st = torch.cuda.current_stream()
    idx = [i for i, c in enumerate(loop.program.calls) if c[2] == "freeu"]
    per = []
    for _ in range(5):
        loop.scheduler.reset()
        loop.program.run_timed(st)
        per.append([loop.program.last_launch_ms[i] * 1e3 for i in idx])
    loop.scheduler.reset()
    med = [statistics.median(col) for col in zip(*per)]
    for i, us in zip(idx, med):
        a = loop.program.calls[i][1]
        print(f"freeu launch {i}: B {a[6]} {a[7]}x{a[8]} Ch {a[2]} Cs {a[5]}: {us:.1f} us")
    print(f"six pp_freeu launches: {sum(med):.1f} us (event-timed, eager); step delta (medians) {(on - off) * 1e3:.1f} us; "
          f"largest round-to-round spread of one variant {spread * 1e3:.1f} us")
    for _, p in variants:
        p._loop.flush_faults()


if __name__ == "__main__":
    main()
