#!/usr/bin/env python
"""What perturbed-attention guidance costs per network evaluation, and where the cost sits.

ppt-v2 headline (BrushNet + UNet, batch `--per-gpu`, CFG 7.5, DPM-Solver++, hipGraph replay, the synthetic inputs of bench.py),
three arms built once, each its own pipeline, timed ALTERNATING (`--reps` rounds of one pipeline call behind `--warmup`
untimed calls), all in this one process on one GPU:
    (i)   pag_scale = 0                       the plan without PAG: batch 2 B
    (ii)  pag_scale = 3, layers "mid"         batch 3 B, one self-attention perturbed
    (iii) pag_scale = 3, every self-attention batch 3 B, sixteen perturbed
Then one eager step of (i) and (ii) with an event pair around every launch (an event pair adds a few microseconds of its own):
the side network's launches at 2 B and 3 B (the difference is its third segment, whose residuals equal the second's), the
UNet's launches in front of the first selected transformer at 3 B (a third of it is the perturbed segment running a prefix in
which it equals the conditional one), and the two new kernels' launches.
A record, not a gate:   python tools/pag_cost.py > profiles/pag_step.txt   (1024^2 fp16: --latent 128 --dtype fp16 --per-gpu 1)
`--arms iii --reps 1 --no-split` is the short run for a `rocprofv3 --kernel-trace --stats` pass of its own.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = {"i": ("(i) PAG off", None), "ii": ('(ii) PAG, "mid"', "mid"), "iii": ("(iii) PAG, all self-attentions", ["down", "mid", "up"])}


def split(pipe, rounds=5):
    """One eager step, event-timed per launch -> {part: ms}: side network, UNet in front of the first identity launch, the rest of
    the UNet, the tail; and the per-launch times of the two PAG kernels."""
    loop = pipe._loop
    side = {id(c) for c in loop.side_rt.step_plan.calls} if loop.side_rt is not None else set()
    unet = {id(c) for c in loop.rt.step_plan.calls}
    calls = loop.program.calls
    first = next((i for i, c in enumerate(calls) if c[2] == "attn_identity_v"), None)
    if first is not None:           # the first launch of that transformer: the nearest GroupNorm statistics / fused front end in front
        first = max(i for i in range(first) if calls[i][2] in ("tfront", "groupnorm_stats", "groupnorm_apply"))
    st = torch.cuda.current_stream()
    runs = []
    for _ in range(rounds):
        loop.scheduler.reset()
        loop.program.run_timed(st)
        runs.append(list(loop.program.last_launch_ms))
    loop.scheduler.reset()
    ms = [statistics.median(col) for col in zip(*runs)]
    out = {"side network": 0.0, "UNet in front of the first selected transformer": 0.0, "UNet": 0.0, "head and tail": 0.0}
    kern = {"attn_identity_v": [], "pag_combine": []}
    for i, (c, t) in enumerate(zip(calls, ms)):
        if id(c) in side:
            out["side network"] += t
        elif id(c) in unet:
            out["UNet"] += t
            if first is not None and i < first:
                out["UNet in front of the first selected transformer"] += t
        else:
            out["head and tail"] += t
        if c[2] in kern:
            kern[c[2]].append(t * 1e3)
    return out, kern, len(calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-gpu", type=int, default=4)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--denoise-steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--arms", default="i,ii,iii")
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
        name, layers = ARMS[key]
        pipe, _, _ = bench.build_pipeline("v2", dev, 0, 1, net_kw=net_kw, dtype=dtype)
        kw = bench.synthetic_inputs("v2", dev, 0, args.per_gpu, args.latent, args.denoise_steps)
        if layers is not None:
            pipe.set_pag_applied_layers(layers)
            kw["pag_scale"] = 3.0
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
            print(f"{name}: UNet batch {p._loop.rt.B}, launches per evaluation {len(names)} (attn_identity_v "
                  f"{names.count('attn_identity_v')}, pag_combine {names.count('pag_combine')})")
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
    base = med.get(ARMS["i"][0])
    if base:
        for name in med:
            if name != ARMS["i"][0]:
                print(f"{name} / (i) = {med[name] / base:.3f}  (+{med[name] - base:.3f} ms; the batch ratio is 1.5)")
    if not args.no_split:
        parts = {}
        for name, p, _ in arms:
            parts[name], kern, n = split(p)
            print(f"{name}: one eager evaluation, event-timed, {n} launches: " +
                  ";  ".join(f"{k} {v:.3f} ms" for k, v in parts[name].items() if v))
            for k, v in kern.items():
                if v:
                    print(f"    {len(v)} pp_{k} launch(es): sum {sum(v):.1f} us, per launch {[round(x, 1) for x in v]}")
        off, mid = parts.get(ARMS["i"][0]), parts.get(ARMS["ii"][0])
        if off and mid:
            tot = sum(v for k, v in mid.items() if not k.startswith("UNet in")) - sum(v for k, v in off.items() if not k.startswith("UNet in"))
            side = mid["side network"] - off["side network"]
            pre = mid["UNet in front of the first selected transformer"] / 3
            print(f'of the {tot:.3f} ms that "mid" adds to an eager evaluation: {side:.3f} ms ({100 * side / tot:.0f} %) is the side '
                  f"network's third segment; {pre:.3f} ms ({100 * pre / tot:.0f} %) is a third of the UNet in front of the first selected "
                  f"transformer (the perturbed segment's share of a prefix it shares with the conditional one)")
    for _, p, _ in arms:
        p._loop.flush_faults()


if __name__ == "__main__":
    main()
