#!/usr/bin/env python
"""What the AsymmetricAutoencoderKL decode costs: x-1-5 geometry (up (192, 384, 768, 768), four resnets per up block), random-init
weights, `--images` images at `--side`^2 in bf16 -- unconditioned and mask-conditioned -- against the stock AutoencoderKL decode
of the same latents, in ONE process, arms alternating.

    python tools/asym_vae_cost.py > profiles/asym_vae.txt

Per arm: `--reps` rounds of one `decode` call behind `--warmup` untimed ones, host clock around work that ends in a device
synchronise; every round is printed.  Then one eager replay of each plan with a HIP event pair around every launch (three
replays, the median per launch is kept): ms summed by launch name, and for every matrix-core convolution its achieved rate =
the FLOPs the launch executes (2 M N K from its shapes) over its time, as a fraction of the dense bf16 peak (2.5 PFLOP/s,
MI355X).  The three 4x4 stride-2 convs of the condition encoder are listed one by one, next to the 3x3 launches of the same run.
`--once ARM` runs one warmed decode of one arm and nothing else: the command to put under `rocprofv3 --kernel-trace --stats`.
A record, not a gate.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BF16 = 2.5e15       # dense bf16 FLOP/s of the MI355X


def launch_flops(call):
    """FLOPs one launch record executes (0 for launches that are no matrix-core convolution / GEMM)."""
    from powerpaint_amd import _lib as L
    fn, args, name = call
    if name == "conv4x4s2":
        _, B, H, W, cin, _, _, cout = args[:8]
        return 2.0 * B * ((H - 2) // 2 + 1) * ((W - 2) // 2 + 1) * cout * 16 * cin
    a = getattr(args[0], "_obj", None) if args else None
    if isinstance(a, L.PPGemmArgs):
        return (4 if a.subpix else 1) * 2.0 * a.M * a.N * a.K
    return 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--once", choices=["stock", "uncond", "cond"], help="one warmed decode of this arm, for a kernel trace")
    ap.add_argument("--tiny", action="store_true", help="reduced networks (a rehearsal of the script, not a measurement)")
    args = ap.parse_args()

    from powerpaint_amd import _lib as L, models as PM
    assert torch.cuda.is_available(), "needs a GPU: there is no fallback and no CPU figure"
    dev = "cuda:0"
    torch.cuda.set_device(0)
    down, up, ld, lu, sb, sl = (128, 256, 512, 512), (192, 384, 768, 768), 2, 3, (128, 256, 512, 512), 2
    if args.tiny:
        down, up, ld, lu, sb, sl = (64, 128, 256, 256), (64, 128, 256, 256), 1, 1, (64, 128, 256, 256), 1
    asym = PM.AsymmetricAutoencoderKL(down_block_types=("DownEncoderBlock2D",) * 4, down_block_out_channels=down,
                                      layers_per_down_block=ld, up_block_types=("UpDecoderBlock2D",) * 4,
                                      up_block_out_channels=up, layers_per_up_block=lu, device=dev)
    asym.load_state_dict(asym.net.synthetic_state_dict(seed=0))
    stock = PM.AutoencoderKL(block_out_channels=sb, layers_per_block=sl, device=dev)
    stock.load_state_dict(stock.net.synthetic_state_dict(seed=0))
    B, S = args.images, args.side
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(B, 4, S // 8, S // 8, generator=g) * 3).to(dev)
    img = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
    mask = torch.zeros(B, 1, S, S)
    for b in range(B):
        mask[b, :, S // 8 * (1 + b % 3): S // 8 * (5 + b % 3), S // 4: S // 4 * 3] = 1.0
    mask = mask.to(dev)
    arms = [("stock", lambda: stock.decode(z, return_dict=False)[0], lambda: stock._dec.plan),
            ("uncond", lambda: asym.decode(z, return_dict=False)[0], lambda: asym._dec.plan),
            ("cond", lambda: asym.decode(z, image=img, mask=mask, return_dict=False)[0], lambda: asym._dec_cond.plan)]
    print(f"build {L.lib().pp_build_id().decode()}  device {torch.cuda.get_device_name(0)}  {B} images {S}x{S} bf16  "
          f"stock {sb} x{sl + 1}  asymmetric up {up} x{lu + 1}{'  (TINY networks: rehearsal)' if args.tiny else ''}")
    if args.once:
        run = dict((n, f) for n, f, _ in arms)[args.once]
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        out = run()
        torch.cuda.synchronize()
        print(f"{args.once}: one decode, output {tuple(out.shape)} finite {bool(torch.isfinite(out).all())}")
        return
    for name, run, plan in arms:
        for _ in range(args.warmup):
            out = run()
        torch.cuda.synchronize()
        assert torch.isfinite(out).all(), name
        p = plan()
        print(f"{name}: {len(p.calls)} launches, {p.flops_executed / 1e12:.3f} TFLOP executed per call "
              f"({p.flops_executed / B / 1e12:.3f} per image)")
    times = {n: [] for n, _, _ in arms}
    for _ in range(args.reps):
        for name, run, _ in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    base = statistics.median(times["stock"])
    for name, _, plan in arms:
        v = times[name]
        med = statistics.median(v)
        print(f"{name}: ms per decode call, per round {[round(x, 2) for x in v]}  median {med:.2f}  min {min(v):.2f}  max "
              f"{max(v):.2f}  = {med / base:.3f} x stock  ({plan().flops_executed / med / 1e9:.0f} TFLOP/s end to end, "
              f"{plan().flops_executed / med / 1e-3 / PEAK_BF16 * 100:.1f} % of the dense bf16 peak: a whole-call figure)")
    st = torch.cuda.current_stream()
    for name, run, plan in arms:
        run()                                      # (inputs packed; the replays below rerun the plan on them)
        p = plan()
        per = []
        for _ in range(3):
            p.run_timed(st)
            per.append(list(p.last_launch_ms))
        med = [statistics.median(col) for col in zip(*per)]
        by = {}
        for (fn, a, nm), ms in zip(p.calls, med):
            by[nm] = by.get(nm, 0.0) + ms
        print(f"{name}: per launch name, ms (HIP events, eager, sum {sum(med):.2f}): " +
              "  ".join(f"{k} {v:.2f}" for k, v in sorted(by.items(), key=lambda kv: -kv[1])))
        fam = {}
        for call, ms in zip(p.calls, med):
            fl = launch_flops(call)
            if not fl:
                continue
            if call[2] == "conv4x4s2":
                _, b_, h_, w_, cin, _, _, cout = call[1][:8]
                print(f"  conv4x4s2 {h_}x{w_} {cin}->{cout}: {ms:.3f} ms  {fl / 1e9:.0f} GFLOP  {fl / ms / 1e9:.0f} TFLOP/s  "
                      f"{fl / ms / 1e-3 / PEAK_BF16 * 100:.1f} % of peak")
            f = fam.setdefault(call[2], [0.0, 0.0])
            f[0] += fl
            f[1] += ms
        for k, (fl, ms) in fam.items():
            print(f"  {k} (all launches of the name): {ms:.2f} ms  {fl / 1e12:.3f} TFLOP  {fl / ms / 1e9:.0f} TFLOP/s  "
                  f"{fl / ms / 1e-3 / PEAK_BF16 * 100:.1f} % of peak")
        if name == "cond":
            idx = [i for i, c in enumerate(p.calls) if c[2] == "conv3x3"][:1]      # layer 1 of the condition encoder
            for i in idx:
                fl = launch_flops(p.calls[i])
                print(f"  conv3x3 layer 1 of the condition encoder ({p.describe(i)}): {med[i]:.3f} ms  "
                      f"{fl / med[i] / 1e9:.0f} TFLOP/s  {fl / med[i] / 1e-3 / PEAK_BF16 * 100:.1f} % of peak")


if __name__ == "__main__":
    main()
