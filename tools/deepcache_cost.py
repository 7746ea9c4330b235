#!/usr/bin/env python
"""What DeepCache (powerpaint_amd/deepcache.py) does to the cost of a denoising call: ms per full and per shallow evaluation, ms
per step averaged over the schedule, launches and FLOPs of the two programs, and how far the final latents move.

One process per shape (the synthetic inputs of bench.py, hipGraph replay).  One pipeline per `--branches` entry plus the
unpatched one; an arm is (cache_branch_id, cache_interval) -- the interval is host schedule, so the arms of a branch share
their pipeline, plans and graphs.  Per branch two more arms: interval 1 (every evaluation full: the full program's cost with
the patch in place) and interval = steps (one full evaluation, then shallow ones only: the shallow program's cost).  The arms
are timed ALTERNATING over `--reps` rounds of one pipeline call behind `--warmup` untimed calls; the baseline is the unpatched
arm of the same process (boxes differ by up to 20 %: a figure from another run is no baseline).  Then one eager shallow
evaluation per branch with an event pair around every launch (`--split-rounds` times, median per launch), summed by launch
name.  A record, not a gate:
    python tools/deepcache_cost.py >> profiles/deepcache_step.txt                                       (512^2 bf16 batch 4, v1)
    python tools/deepcache_cost.py --config v2 >> profiles/deepcache_step.txt
    python tools/deepcache_cost.py --latent 128 --dtype fp16 --per-gpu 1 >> profiles/deepcache_step.txt
Kernel trace of shallow evaluations, in a run of its own:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/deepcache_cost.py --trace 20
    python tools/deepcache_cost.py --parse-trace DIR >> profiles/deepcache_step.txt
(`--trace N`: one patched pipeline, one warm call, a 1 s pause, then N eager shallow evaluations and nothing else; `--parse-trace`
sums, by kernel name, what ran behind the last pause of the trace.)
The cosine of the final latents against the unpatched call is reported, ungated: the weights are synthetic (random init), which
tells little about image quality -- it shows that the cache is in use and how the drift orders over the settings, no more.
"""
import argparse
import csv
import glob
import os
import re
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_trace(path):
    files = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
    assert files, f"no *kernel_trace.csv under {path}"
    rows = []
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    cut = max((i for i in range(1, len(rows)) if rows[i][0] - rows[i - 1][1] > 500_000_000), default=0)
    tail = rows[cut:]
    by = {}
    for s, e, n in tail:
        short = re.split(r"[<(]", re.sub(r"^void\s+", "", n.replace("(anonymous namespace)::", "")))[0][-60:]
        t, c = by.get(short, (0, 0))
        by[short] = (t + e - s, c + 1)
    total = sum(t for t, _ in by.values())
    span = tail[-1][1] - tail[0][0]
    print(f"[deepcache trace] {len(tail)} kernels behind the last pause of {os.path.basename(files[0])}: {total / 1e6:.3f} ms of kernel time in "
          f"{span / 1e6:.3f} ms of wall time (eager launches: the gaps are launch latency, which a graph replay does not pay)")
    for n, (t, c) in sorted(by.items(), key=lambda kv: -kv[1][0]):
        print(f"    {t / 1e6:9.3f} ms  {100.0 * t / total:5.1f} %  {c:5d} x  {n}")


def split_by_name(loop, rounds):
    """One eager shallow evaluation, an event pair around every launch -> ({launch name: (ms, count)}, total ms, launches)."""
    st = torch.cuda.current_stream()
    prog = loop.program_shallow
    runs = []
    for _ in range(rounds):
        loop.scheduler.reset()
        prog.run_timed(st)
        runs.append(list(prog.last_launch_ms))
    loop.scheduler.reset()
    ms = [statistics.median(col) for col in zip(*runs)]
    by = {}
    for c, t in zip(prog.calls, ms):
        a, n = by.get(c[2], (0.0, 0))
        by[c[2]] = (a + t, n + 1)
    return by, sum(ms), len(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="v1", choices=["v1", "v2", "controlnet"])
    ap.add_argument("--per-gpu", type=int, default=4)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--denoise-steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--branches", default="0,2")
    ap.add_argument("--intervals", default="2,3,5")
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--split-rounds", type=int, default=5)
    ap.add_argument("--trace", type=int, default=0, metavar="N", help="the short run for a kernel trace (module docstring)")
    ap.add_argument("--parse-trace", default=None, metavar="DIR")
    ap.add_argument("--tiny", action="store_true", help="reduced networks (a rehearsal of the script, not a measurement)")
    args = ap.parse_args()
    if args.parse_trace:
        return parse_trace(args.parse_trace)

    import bench
    from powerpaint_amd import _lib as L
    from powerpaint_amd.deepcache import DeepCacheSDHelper
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = "cuda:0"
    torch.cuda.set_device(0)
    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    N, px = args.denoise_steps, args.latent * 8
    net_kw = dict(block_out_channels=(320, 320, 640, 640), layers_per_block=1) if args.tiny else {}
    branches = [int(b) for b in args.branches.split(",")]
    intervals = [int(i) for i in args.intervals.split(",")]
    kw = bench.synthetic_inputs(args.config, dev, 0, args.per_gpu, args.latent, N)

    if args.trace:
        pipe, _, _ = bench.build_pipeline(args.config, dev, 0, 1, net_kw=net_kw, dtype=dtype, scheduler="ddim")
        DeepCacheSDHelper(pipe).set_params(cache_interval=2, cache_branch_id=branches[0]).enable()
        pipe(**dict(kw, num_inference_steps=2))
        loop = pipe._loop
        torch.cuda.synchronize()
        time.sleep(1.0)
        st = torch.cuda.current_stream().cuda_stream
        for _ in range(args.trace):
            loop.scheduler.reset()
            loop.program_shallow.run(st)
        torch.cuda.synchronize()
        print(f"[deepcache trace] {args.trace} eager shallow evaluations, cache_branch_id {branches[0]}, "
              f"{len(loop.program_shallow.calls)} launches each")
        return

    print(f"[deepcache step] build {L.lib().pp_build_id().decode()}  {torch.cuda.get_device_name(0)}  {args.config} batch "
          f"{args.per_gpu} CFG 7.5 {px}x{px} {args.dtype} {N} DDIM steps, hipGraph replay, {args.reps} rounds, arms alternating"
          f"{'  (TINY networks: rehearsal)' if args.tiny else ''}")
    pipes = {}
    for b in [None] + branches:
        pipe, _, _ = bench.build_pipeline(args.config, dev, 0, 1, net_kw=net_kw, dtype=dtype, scheduler="ddim")
        helper = None
        if b is not None:
            helper = DeepCacheSDHelper(pipe).set_params(cache_interval=2, cache_branch_id=b).enable()
        pipes[b] = (pipe, helper)
    arms = [("unpatched", None, None)]
    for b in branches:
        arms += [(f"id {b} interval {i}", b, i) for i in [1] + intervals + [N]]

    def call(b, i):
        pipe, helper = pipes[b]
        if helper is not None:
            helper.set_params(cache_interval=i, cache_branch_id=b)
        return pipe(**kw)[0]

    outs = {}
    for name, b, i in arms:
        for _ in range(max(args.warmup, 1)):
            outs[name] = call(b, i).float().clone()
        torch.cuda.synchronize()
        assert torch.isfinite(outs[name]).all(), name
    times = {name: [] for name, _, _ in arms}
    for _ in range(args.reps):
        for name, b, i in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(b, i)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / N)
    med = {name: statistics.median(v) for name, v in times.items()}
    base = med["unpatched"]
    ref = outs["unpatched"].flatten()
    print(f"  unpatched: {base:.3f} ms / step (median; per round {[round(x, 3) for x in times['unpatched']]}, spread "
          f"{max(times['unpatched']) - min(times['unpatched']):.3f}); launches per evaluation "
          f"{len(pipes[None][0]._loop.program.calls)}")
    for b in branches:
        loop = pipes[b][0]._loop
        full = med[f"id {b} interval 1"]
        shallow = (med[f"id {b} interval {N}"] * N - full) / (N - 1)
        fr = loop.program_shallow.flops / loop.program.flops
        print(f"  cache_branch_id {b}: full evaluation {full:.3f} ms ({full / base:.3f} x unpatched), shallow evaluation "
              f"{shallow:.3f} ms; time ratio shallow / full {shallow / full:.3f}, FLOP ratio {fr:.3f}; launches per shallow "
              f"evaluation {len(loop.program_shallow.calls)} (full {len(loop.program.calls)}); arena "
              f"{loop.rt.arena.size / pipes[None][0]._loop.rt.arena.size:.3f} x the unpatched UNet's")
        for i in [1] + intervals + [N]:
            name = f"id {b} interval {i}"
            v = times[name]
            nf = len([e for e in range(N) if e % i == 0])
            model = (nf * full + (N - nf) * shallow) / N
            cos = torch.nn.functional.cosine_similarity(outs[name].flatten(), ref, dim=0).item()
            print(f"    interval {i:3d} ({nf} full of {N}): {med[name]:.3f} ms / step = {med[name] / base:.3f} x unpatched "
                  f"({med[name] - base:+.3f} ms; per round spread {max(v) - min(v):.3f}; from the two evaluation costs "
                  f"{model:.3f}); cosine of the final latents against unpatched {cos:.6f}")
    if not args.no_split:
        for b in branches:
            loop = pipes[b][0]._loop
            by, total, n = split_by_name(loop, args.split_rounds)
            print(f"  cache_branch_id {b}: one eager shallow evaluation, event-timed (an event pair adds a few us per launch), "
                  f"{n} launches, {total:.3f} ms in all, by launch name:")
            fl = {}
            for r in [loop.rt] + list(loop.side_rts):
                for k, v in r.shallow_plan.flops_by_kind.items():
                    fl[k] = fl.get(k, 0.0) + v
            for k, (t, c) in sorted(by.items(), key=lambda kv: -kv[1][0]):
                tf = f"  {fl[k] / t / 1e9:7.1f} TFLOP/s" if fl.get(k) and t > 0 else ""
                print(f"      {k:22s} {c:3d} x  {t:8.3f} ms  {100 * t / total:5.1f} %{tf}")
    for pipe, _ in pipes.values():
        pipe._loop.flush_faults()


if __name__ == "__main__":
    main()
