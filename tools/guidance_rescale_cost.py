#!/usr/bin/env python
"""What `guidance_rescale` costs per network evaluation.

ppt-v2 headline (BrushNet + UNet, batch `--per-gpu`, CFG 7.5, DPM-Solver++, hipGraph replay, the synthetic inputs of bench.py),
four arms built once, each its own pipeline, timed ALTERNATING (`--reps` rounds of one pipeline call behind `--warmup` untimed
calls), all in this one process on one GPU:
    (i)   guidance_rescale = 0                   the plan without it: the baseline
    (ii)  guidance_rescale = 0.7                 one pp_cfg_rescale launch in front of the step launch
    (iii) pag_scale = 3, layers "mid"            PAG alone: pp_pag_combine in that place
    (iv)  pag_scale = 3 and guidance_rescale     pp_cfg_rescale on three segments in the place of pp_pag_combine
The arm spread is the largest (max - min) over the rounds of one arm: a difference between arms below it is not resolved.
Then one eager evaluation of each arm with an event pair around every launch (an event pair adds a few microseconds of its
own): the per-launch times of pp_cfg_rescale and pp_pag_combine.
A record, not a gate:   python tools/guidance_rescale_cost.py > profiles/guidance_rescale_step.txt
(1024^2 fp16: --latent 128 --dtype fp16 --per-gpu 1).  `--arms ii,iii --reps 1 --no-split` is the short run for a
`rocprofv3 --kernel-trace --stats` pass of its own, which has cfg_rescale_kernel and pag_combine_kernel side by side.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = {"i": ("(i) guidance_rescale 0", False, 0.0), "ii": ("(ii) guidance_rescale 0.7", False, 0.7),
        "iii": ('(iii) PAG "mid"', True, 0.0), "iv": ('(iv) PAG "mid" + guidance_rescale 0.7', True, 0.7)}
KERNELS = ("cfg_rescale", "pag_combine")


def launch_times(pipe, rounds=5):
    """One eager evaluation, event-timed per launch, median over `rounds` -> ({kernel: [us per launch]}, launches)."""
    loop = pipe._loop
    st = torch.cuda.current_stream()
    runs = []
    for _ in range(rounds):
        loop.scheduler.reset()
        loop.program.run_timed(st)
        runs.append(list(loop.program.last_launch_ms))
    loop.scheduler.reset()
    ms = [statistics.median(col) for col in zip(*runs)]
    kern = {k: [] for k in KERNELS}
    for c, t in zip(loop.program.calls, ms):
        if c[2] in kern:
            kern[c[2]].append(t * 1e3)
    return kern, len(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-gpu", type=int, default=4)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--denoise-steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--arms", default="i,ii,iii,iv")
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--tiny", action="store_true", help="reduced networks (a rehearsal of the script, not a measurement)")
    args = ap.parse_args()

    import bench
    from powerpaint_amd import _lib as L
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = "cuda:0"
    torch.cuda.set_device(0)
    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    print(f"build {L.lib().pp_build_id().decode()}  device {torch.cuda.get_device_name(0)}")
    net_kw = dict(block_out_channels=(320, 320, 640, 640), layers_per_block=1) if args.tiny else {}
    arms = []
    for key in args.arms.split(","):
        name, pag, phi = ARMS[key]
        pipe, _, _ = bench.build_pipeline("v2", dev, 0, 1, net_kw=net_kw, dtype=dtype)
        kw = bench.synthetic_inputs("v2", dev, 0, args.per_gpu, args.latent, args.denoise_steps)
        if pag:
            pipe.set_pag_applied_layers("mid")
            kw["pag_scale"] = 3.0
        if phi:
            kw["guidance_rescale"] = phi
        arms.append((name, pipe, kw))
    px = args.latent * 8
    print(f"ppt-v2 batch {args.per_gpu} CFG 7.5 {px}x{px} {args.dtype} {args.denoise_steps} DPM-Solver++ steps, hipGraph replay"
          f"{'  (TINY networks: rehearsal)' if args.tiny else ''}")
    for name, p, kw in arms:
        for _ in range(args.warmup):
            out = p(**kw)[0]
        torch.cuda.synchronize()
        if args.warmup:
            assert torch.isfinite(out).all()
            names = [c[2] for c in p._loop.program.calls]
            print(f"{name}: UNet batch {p._loop.rt.B}, launches per evaluation {len(names)} (" +
                  ", ".join(f"{k} {names.count(k)}" for k in KERNELS) + ")")
    times = {name: [] for name, _, _ in arms}
    for _ in range(args.reps):
        for name, p, kw in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p(**kw)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / args.denoise_steps)
    med = {}
    for name, _, _ in arms:
        v = times[name]
        med[name] = statistics.median(v)
        print(f"{name}: ms per evaluation, per round {[round(x, 3) for x in v]}  median {med[name]:.3f}  min {min(v):.3f}  "
              f"max {max(v):.3f}")
    spread = max(max(v) - min(v) for v in times.values())
    print(f"arm spread (largest max - min over the rounds of one arm): {spread:.3f} ms")
    for a, b in (("i", "ii"), ("iii", "iv")):
        na, nb = ARMS[a][0], ARMS[b][0]
        if na in med and nb in med:
            print(f"{nb} - {na} = {(med[nb] - med[na]) * 1e3:+.1f} us per evaluation")
    if not args.no_split:
        for name, p, _ in arms:
            kern, n = launch_times(p)
            for k, v in kern.items():
                if v:
                    print(f"{name}: one eager evaluation, event-timed, {n} launches: {len(v)} pp_{k} launch(es), "
                          f"per launch {[round(x, 1) for x in v]} us")
    for _, p, _ in arms:
        p._loop.flush_faults()


if __name__ == "__main__":
    main()
