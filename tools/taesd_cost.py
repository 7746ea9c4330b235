#!/usr/bin/env python
"""What AutoencoderTiny (TAESD) costs against AutoencoderKL, and what pp_conv3x3_c64 reaches against the stock implicit-GEMM
launch of the same shape -- random-init weights, ONE process, arms alternating over `--reps` rounds.

    python tools/taesd_cost.py > profiles/taesd.txt

Part 1, per configuration (4 x 512^2 bf16, 1 x 1024^2 fp16; AutoencoderKL computes in bf16 in both): decode and encode of
either VAE, one call per arm and round behind `--warmup` untimed ones, host clock around work that ends in a device
synchronise; every round is printed.  Then one eager replay of the TAESD plans with a HIP event pair around every launch
(three replays, the median per launch is kept), summed by launch name.
Part 2, per mode of pp_conv3x3_c64 (0 stride 1, 1 stride 2, 2 nearest 2x + conv) and OUTPUT side 64, 128, 256, 512 (batch 4,
bf16, bias, no ReLU, no residual): `--inner` back-to-back launches between two HIP events per arm and round; ms per launch
(median of the rounds), the rate = 2 * pixels * 64 * 576 FLOP over that time as a fraction of the dense bf16 peak (2.5 PFLOP/s,
the figure `bench.py --full` uses), and beside it the stock `pp_gemm_bf16` PP_X_CONV3X3 launch (N = 64) of the same shape on
the same tensors.  new / stock > 1 means the new kernel LOSES at that shape.
`--tiny` shrinks everything to a rehearsal of the script.  A record, not a gate.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BF16 = 2.5e15       # dense bf16 FLOP/s of the MI355X (bench.py: MFMA_PEAK_TFLOPS)


def alternate(arms, reps, warmup):
    """arms: [(name, fn)]; ms per call of every arm, one call per arm and round."""
    for _, fn in arms:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in arms}
    for _ in range(reps):
        for name, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return times


def vae_part(B, S, dtype, args, dev):
    from powerpaint_amd import models as PM
    kl_cfg = dict(block_out_channels=(64, 128, 256, 256), layers_per_block=1) if args.tiny else {}
    kl = PM.AutoencoderKL(device=dev, **kl_cfg)
    kl.load_state_dict(kl.net.synthetic_state_dict(seed=0))
    tiny = PM.AutoencoderTiny(device=dev, dtype=dtype)
    tiny.load_state_dict(tiny.net.synthetic_state_dict(seed=0))
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(B, 4, S // 8, S // 8, generator=g) * 3).to(dev)
    img = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
    arms = [("AutoencoderKL decode", lambda: kl.decode(z, return_dict=False)[0]),
            ("AutoencoderTiny decode", lambda: tiny.decode(z, return_dict=False)[0]),
            ("AutoencoderKL encode", lambda: kl.encode(img).latent_dist.mean),
            ("AutoencoderTiny encode", lambda: tiny.encode(img).latents)]
    name = {torch.bfloat16: "bf16", torch.float16: "fp16"}[dtype]
    print(f"\n== {B} x {S}^2, AutoencoderTiny in {name} (AutoencoderKL in bf16) ==")
    times = alternate(arms, args.reps, args.warmup)
    for n, fn in arms:
        assert torch.isfinite(fn()).all(), n
    med = {n: statistics.median(v) for n, v in times.items()}
    for n, _ in arms:
        v = times[n]
        print(f"{n}: ms per call, per round {[round(x, 3) for x in v]}  median {med[n]:.3f}  min {min(v):.3f}  max {max(v):.3f}")
    for what in ("decode", "encode"):
        a, b = med[f"AutoencoderTiny {what}"], med[f"AutoencoderKL {what}"]
        print(f"{what}: AutoencoderTiny / AutoencoderKL = {a / b:.3f} ({b / a:.1f} x faster)" if a <= b else
              f"**{what}: AutoencoderTiny / AutoencoderKL = {a / b:.3f}: the tiny VAE LOSES**")
    st = torch.cuda.current_stream()
    for what, rt in (("decode", tiny._dec), ("encode", tiny._enc)):
        p = rt.plan
        per = []
        for _ in range(3):
            p.run_timed(st)
            per.append(list(p.last_launch_ms))
        ms = [statistics.median(col) for col in zip(*per)]
        by = {}
        for (fn, a, nm), t in zip(p.calls, ms):
            by[nm] = by.get(nm, 0.0) + t
        fl = p.flops_by_kind.get("conv3x3_c64", 0.0)
        print(f"AutoencoderTiny {what}: {len(p.calls)} launches, {p.flops / 1e12:.3f} TFLOP in the 64 -> 64 convs per call; per "
              f"launch name, ms (HIP events, eager, sum {sum(ms):.3f}): " +
              "  ".join(f"{k} {v:.3f}" for k, v in sorted(by.items(), key=lambda kv: -kv[1])) +
              f"; conv3x3_c64 {fl / by['conv3x3_c64'] / 1e9:.0f} TFLOP/s = {fl / by['conv3x3_c64'] / 1e-3 / PEAK_BF16 * 100:.1f} % of "
              "the dense bf16 peak over its launches")


def kernel_part(args, dev):
    from powerpaint_amd import _lib as L
    from powerpaint_amd.engine import Act, Arena, Builder, _align
    lib = L.lib()
    B, dtype = (1 if args.tiny else 4), torch.bfloat16
    dt = L.dtype_code(dtype)
    sides = (16, 32) if args.tiny else (64, 128, 256, 512)
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(64, 576, generator=g) / 24).to(dtype).to(dev)
    bias = torch.randn(64, generator=g).to(dev)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    print(f"\n== pp_conv3x3_c64 against the stock PP_X_CONV3X3 launch (N = 64), batch {B}, bf16, bias, {args.inner} launches per "
          "timing ==")
    lost = []
    for mode in (0, 1, 2):
        for S in sides:
            hin = (S, 2 * S, S // 2)[mode]
            x = torch.randn(B, hin, hin, 64, generator=g).to(dtype).to(dev)
            out_new = torch.empty(B, S, S, 64, dtype=dtype, device=dev)

            def build(arena):
                pb = Builder(arena, dtype=dtype)
                o = pb.conv3x3(Act(x.data_ptr(), B, hin, hin, 64), w.data_ptr(), 64, bias.data_ptr(), stride=2 if mode == 1 else 1,
                               up=(mode == 2))
                return pb.plan, o

            dry = Arena()
            build(dry)
            arena = Arena(_align(dry.peak, 4096), dev)
            plan, o = build(arena)
            assert (o.H, o.W) == (S, S)

            def new():
                L.check(lib.pp_conv3x3_c64(x.data_ptr(), B, hin, hin, w.data_ptr(), bias.data_ptr(), None, mode, 0,
                                           out_new.data_ptr(), dt, st), "pp_conv3x3_c64")

            def stock():
                plan.run(st)

            new(), stock()
            torch.cuda.synchronize()
            a, b = out_new.float(), arena.view(o.ptr, (B, S, S, 64), dtype).float()
            diff = (a - b).abs().max().item()                  # two fp32 summation orders, one 16-bit rounding each
            assert diff <= 2.0 ** -6 * max(1.0, b.abs().max().item()), (mode, S, diff)
            ms = {"new": [], "stock": []}
            for _ in range(args.warmup):
                new(), stock()
            for _ in range(args.reps):
                for name, fn in (("new", new), ("stock", stock)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(args.inner):
                        fn()
                    e1.record(stream)
                    e1.synchronize()
                    ms[name].append(e0.elapsed_time(e1) / args.inner)
            flop = 2.0 * B * S * S * 64 * 576
            mn, msx = statistics.median(ms["new"]), statistics.median(ms["stock"])
            line = (f"mode {mode} output {S:3d}^2: new {mn * 1e3:8.1f} us ({flop / mn / 1e-3 / PEAK_BF16 * 100:5.2f} % of peak, rounds "
                    f"{[round(v * 1e3, 1) for v in ms['new']]})  stock {msx * 1e3:8.1f} us ({flop / msx / 1e-3 / PEAK_BF16 * 100:5.2f} %, "
                    f"rounds {[round(v * 1e3, 1) for v in ms['stock']]}, {plan.describe(0)})  new / stock {mn / msx:.3f}  "
                    f"max |new - stock| {diff:.3g}")
            if mn > msx:
                lost.append((mode, S))
                line = f"**{line}  <- the new kernel LOSES**"
            print(line)
            del x, out_new, arena
    print("the new kernel loses at (mode, output side): " + (", ".join(map(str, lost)) if lost else "nowhere"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--tiny", action="store_true", help="small shapes and a reduced AutoencoderKL (a rehearsal, not a measurement)")
    args = ap.parse_args()
    from powerpaint_amd import _lib as L
    assert torch.cuda.is_available(), "needs a GPU: there is no fallback and no CPU figure"
    dev = "cuda:0"
    torch.cuda.set_device(0)
    print(f"build {L.lib().pp_build_id().decode()}  device {torch.cuda.get_device_name(0)}"
          f"{'  (TINY: rehearsal)' if args.tiny else ''}")
    for B, S, dtype in (((1, 64, torch.bfloat16), (1, 128, torch.float16)) if args.tiny else
                        ((4, 512, torch.bfloat16), (1, 1024, torch.float16))):
        vae_part(B, S, dtype, args, dev)
    kernel_part(args, dev)


if __name__ == "__main__":
    main()
