"""Token merging: what a denoising step costs with and without it -> profiles/tome_step.txt (a record, not a gate).

  python tools/tome_step.py [--config v1] [--latent 64] [--per-gpu 4] [--dtype bf16] [--denoise-steps 50] [--rounds 3]

The benchmark's pipeline and inputs (bench.build_pipeline / synthetic_inputs), one process, one build.  Arms: unpatched and
tome.apply_patch(pipe, ratio) for ratio 0.25 / 0.5 / 0.75, alternating over `--rounds` rounds (every arm once per round, one
warm-up call per arm after its re-plan); the figure of an arm is the median over rounds of (wall time of a call, device
synchronised) / (network evaluations), the spread is max - min over the rounds.  Then, per arm, ONE eager replay of the step
program with a HIP event pair around every launch (Plan.run_timed): the new launches beside the attention launches.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import tome  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="v1", choices=["v1", "v2", "controlnet"])
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--per-gpu", type=int, default=4)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--denoise-steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    pipe, nets, _ = bench.build_pipeline(args.config, dev, 0, 1, dtype=dtype)
    kw = bench.synthetic_inputs(args.config, dev, 0, args.per_gpu, args.latent, args.denoise_steps)
    arms = [None, 0.25, 0.5, 0.75]
    times = {a: [] for a in arms}
    launches = {}

    def set_arm(a):
        if a is None:
            tome.remove_patch(pipe)
        else:
            tome.apply_patch(pipe, ratio=a, generator=torch.Generator().manual_seed(0))

    for rnd in range(args.rounds):
        for a in arms:
            set_arm(a)
            pipe(**kw)                                   # re-plan + capture
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipe(**kw)[0]
            torch.cuda.synchronize()
            times[a].append((time.perf_counter() - t0) * 1e3 / len(pipe.scheduler.timesteps))
            assert torch.isfinite(out).all()
            if rnd == 0:
                per = pipe._loop.program.run_timed(torch.cuda.current_stream())
                launches[a] = {k: v for k, v in per.items() if k.startswith("tome") or k == "attention"}
                launches[a]["(all launches)"] = sum(per.values())
    lines = [f"[tome step] build {L.build_id()}  {torch.cuda.get_device_name(0)}  config {args.config} latent {args.latent} "
             f"per-gpu {args.per_gpu} {args.dtype} {args.denoise_steps} steps, {args.rounds} rounds, arms alternating"]
    base = statistics.median(times[None])
    for a in arms:
        t = times[a]
        lines.append(f"  {'unpatched' if a is None else 'ratio %.2f' % a:10s}: {statistics.median(t):8.3f} ms / evaluation "
                     f"(spread {max(t) - min(t):.3f} over {len(t)} rounds; {statistics.median(t) / base:6.3f} x unpatched)")
    lines.append("  per-launch, one eager replay with HIP events around every launch (ms per evaluation, summed by name):")
    for a in arms:
        lines.append(f"  {'unpatched' if a is None else 'ratio %.2f' % a:10s}: " +
                     "  ".join(f"{k} {v:.3f}" for k, v in sorted(launches[a].items())))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
