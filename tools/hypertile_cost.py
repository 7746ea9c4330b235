#!/usr/bin/env python
"""What HyperTile (powerpaint_amd/hypertile.py) does to the cost of a network evaluation, and to the attention launches it tiles.

ppt-v2 headline (BrushNet + UNet, batch `--per-gpu`, CFG 7.5, DPM-Solver++, hipGraph replay, the synthetic inputs of bench.py).
One process per shape; the arms -- unpatched, and hypertile.apply_patch(pipe, tile_size) per `--tile-sizes` entry -- are built
once, each its own pipeline, and timed ALTERNATING over `--reps` rounds of one pipeline call behind `--warmup` untimed calls.
The baseline is the unpatched arm of the same process: boxes differ by up to 20 %, a figure from another run is no baseline.
Then one eager evaluation per arm with an event pair around every launch (`--split-rounds` times, median per launch; an event
pair adds a few microseconds of its own): the self-attention launches the patch tiles, before and after, against the
1 / (nh nw) FLOP ratio.
A record, not a gate:
    python tools/hypertile_cost.py >> profiles/hypertile_step.txt                                   (512^2 bf16 batch 4)
    python tools/hypertile_cost.py --latent 128 --dtype fp16 --per-gpu 1 --tile-sizes 256,512 >> profiles/hypertile_step.txt
`--arms 256 --reps 1 --no-split` is the short run for a `rocprofv3 --kernel-trace --stats` pass of its own.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def attention_launches(pipe, rounds):
    """-> [(network, launch index in the program, entry name, geometry, median ms)] of every "attention" launch of one eager
    evaluation, and the sum over all launches."""
    loop = pipe._loop
    side = {id(c) for c in loop.side_rt.step_plan.calls} if loop.side_rt is not None else set()
    st = torch.cuda.current_stream()
    runs = []
    for _ in range(rounds):
        loop.scheduler.reset()
        loop.program.run_timed(st)
        runs.append(list(loop.program.last_launch_ms))
    loop.scheduler.reset()
    ms = [statistics.median(col) for col in zip(*runs)]
    out = []
    for i, (c, t) in enumerate(zip(loop.program.calls, ms)):
        if c[2] != "attention":
            continue
        a = list(c[1])
        tiled = c[0].__name__ == "pp_attention_fwd_tiled"
        geo = f"B{a[8]} {a[10]}x{a[11]} tokens in {a[12]}x{a[13]} tiles d{a[14]}" if tiled else f"B{a[8]} nq{a[10]} nk{a[11]} d{a[12]}"
        out.append(("side" if id(c) in side else "unet", i, c[0].__name__, geo, t))
    return out, sum(ms), len(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-gpu", type=int, default=4)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--denoise-steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tile-sizes", default="256")
    ap.add_argument("--arms", default=None, help="comma list out of: off, <tile size>; default off + every --tile-sizes entry")
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--split-rounds", type=int, default=5)
    ap.add_argument("--tiny", action="store_true", help="reduced networks (a rehearsal of the script, not a measurement)")
    args = ap.parse_args()

    import bench
    from powerpaint_amd import _lib as L
    from powerpaint_amd import hypertile
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = "cuda:0"
    torch.cuda.set_device(0)
    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    keys = args.arms.split(",") if args.arms else ["off"] + args.tile_sizes.split(",")
    px = args.latent * 8
    print(f"[hypertile step] build {L.lib().pp_build_id().decode()}  {torch.cuda.get_device_name(0)}  ppt-v2 batch {args.per_gpu} "
          f"CFG 7.5 {px}x{px} {args.dtype} {args.denoise_steps} DPM-Solver++ steps, hipGraph replay, {args.reps} rounds, arms "
          f"alternating{'  (TINY networks: rehearsal)' if args.tiny else ''}")
    net_kw = dict(block_out_channels=(320, 320, 640, 640), layers_per_block=1) if args.tiny else {}
    arms = []
    for key in keys:
        pipe, _, _ = bench.build_pipeline("v2", dev, 0, 1, net_kw=net_kw, dtype=dtype)
        kw = bench.synthetic_inputs("v2", dev, 0, args.per_gpu, args.latent, args.denoise_steps)
        name = "unpatched"
        if key != "off":
            hypertile.apply_patch(pipe, tile_size=int(key))
            nh, nw = hypertile.layout(args.latent, args.latent, int(key))
            name = f"tile_size {key} ({nh}x{nw} tiles)"
        arms.append((name, pipe, kw))
    for name, p, kw in arms:
        for _ in range(args.warmup):
            out = p(**kw)[0]
        torch.cuda.synchronize()
        if args.warmup:
            assert torch.isfinite(out).all()
            lay = {n: r.net.hypertile_layout(args.latent, args.latent) for n, r in (("unet", p._loop.rt), ("side", p._loop.side_rt))
                   if r is not None}
            print(f"  {name}: launches per evaluation {len(p._loop.program.calls)}; tiled blocks " +
                  ", ".join(f"{n} {sum(1 for v in d.values() if v[2])} of {len(d)}" for n, d in lay.items()))
    times = {name: [] for name, _, _ in arms}
    for _ in range(args.reps):
        for name, p, kw in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p(**kw)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / args.denoise_steps)
    med = {name: statistics.median(v) for name, v in times.items()}
    base = med.get("unpatched")
    for name, v in times.items():
        rel = f"; {med[name] / base:.3f} x unpatched ({med[name] - base:+.3f} ms)" if base and name != "unpatched" else ""
        print(f"  {name}: {med[name]:.3f} ms / evaluation (median; per round {[round(x, 3) for x in v]}, spread "
              f"{max(v) - min(v):.3f}){rel}")
    if not args.no_split:
        per = {}
        for name, p, _ in arms:
            per[name], total, n = attention_launches(p, args.split_rounds)
            print(f"  {name}: one eager evaluation, event-timed, {n} launches, {total:.3f} ms in all; attention launches "
                  f"{sum(t for *_, t in per[name]):.3f} ms")
        ref = per.get("unpatched")
        for name, rows in per.items():
            if name == "unpatched" or not ref:
                continue
            print(f"  {name}: the launches the patch tiles, per launch (us), unpatched -> patched:")
            b = a = 0.0
            for r0, r1 in zip(ref, rows):
                if r1[2] != "pp_attention_fwd_tiled":
                    continue
                assert r0[:2] == r1[:2], "the two programs differ in more than the tiled launches"
                print(f"    {r1[0]:4s} #{r1[1]:3d} {r0[3]} -> {r1[3]}: {r0[4] * 1e3:8.1f} -> {r1[4] * 1e3:8.1f}  ({r1[4] / r0[4]:.3f})")
                b, a = b + r0[4], a + r1[4]
            if b:
                nh, nw = [int(x) for x in name.split("(")[1].split(" ")[0].split("x")]
                print(f"    sum {b:.3f} -> {a:.3f} ms ({a / b:.3f}; the FLOP ratio is {1.0 / (nh * nw):.4f})")
    for _, p, _ in arms:
        p._loop.flush_faults()


if __name__ == "__main__":
    main()
