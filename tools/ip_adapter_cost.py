#!/usr/bin/env python
"""What an IP-Adapter costs per denoising step, and what pp_ip_attn_add does per launch.

1. pp_ip_attn_add alone at the four levels of the headline shape (batch 8 = 4 images x CFG, one image per adapter: nk = 4),
   bf16: device events around `--launches` back-to-back launches, (a) over a ring of buffers larger than the 256 MB last-level
   cache, so every launch streams q and o from HBM, and (b) over one buffer set (what the step sees: q and o were written by the
   launches right in front).  Against the byte floor 3 * M * C * 2 B (read q, read o, write o) over the 6.29 TB/s copy rate
   measured on this part.
2. ms per denoising step of the ppt-v2 headline (BrushNet + UNet, batch 4, CFG 7.5, 512x512, bf16, 50 DPM-Solver++ steps,
   hipGraph replay, the synthetic inputs of bench.py), three arms built once and timed ALTERNATING, `--reps` rounds of one
   pipeline call each behind `--warmup` untimed calls:
     (i)   the plan of a UNet without adapters;
     (ii)  no adapter, every cross-attention forced onto the generic to_q -> attention -> to_out chain (the fused forms off:
           what loading an adapter bypasses -- the part a later change could win back);
     (iii) one base adapter loaded (4 tokens, image-embed dimension 1024), scale 1.
   A record, not a gate:   python tools/ip_adapter_cost.py > profiles/ip_adapter_step.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 6.29e12


def kernel_part(args, L):
    lib = L.lib()
    dt = torch.bfloat16
    st = torch.cuda.current_stream().cuda_stream
    print(f"pp_ip_attn_add per launch, batch {args.batch}, nk {args.nk}, bf16, {args.launches} launches per window (device events)")
    for hw, C in ((64, 320), (32, 640), (16, 1280), (8, 1280)):
        nq, heads, d = hw * hw, 8, C // 8
        M = args.batch * nq
        nbytes = 3 * M * C * 2
        floor_us = nbytes / COPY_RATE * 1e6
        ring = max(2, int(600e6 // (2 * M * C * 2)) + 1)
        k = torch.randn(args.batch, args.nk, C, device="cuda").to(dt)
        v = torch.randn(args.batch, args.nk, C, device="cuda").to(dt)
        res = {}
        for name, n in (("cold (HBM ring)", ring), ("hot (one buffer set)", 1)):
            qs = [torch.randn(M, C, device="cuda").to(dt) for _ in range(n)]
            os_ = [torch.randn(M, C, device="cuda").to(dt) for _ in range(n)]

            def run(count):
                for i in range(count):
                    L.check(lib.pp_ip_attn_add(qs[i % n].data_ptr(), C, k.data_ptr(), v.data_ptr(), os_[i % n].data_ptr(), C,
                                               args.batch, heads, nq, args.nk, d, d ** -0.5, 1e-3, L.PP_DT_BF16, st), "ip_attn_add")
            run(max(n, 10))
            torch.cuda.synchronize()
            wins = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(args.launches)
                e1.record()
                torch.cuda.synchronize()
                wins.append(e0.elapsed_time(e1) * 1e3 / args.launches)
            res[name] = statistics.median(wins)
            del qs, os_
        print(f"  {hw}x{hw} C {C} (M {M}, d {d}): {nbytes / 1e6:.1f} MB, floor {floor_us:.2f} us;  " +
              ";  ".join(f"{nm} {us:.2f} us = {us / floor_us:.2f} x floor ({nbytes / us / 1e6:.2f} TB/s)" for nm, us in res.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-gpu", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--nk", type=int, default=4)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--denoise-steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--tiny", action="store_true", help="reduced networks (a rehearsal of the script, not a measurement)")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()

    import bench
    from powerpaint_amd import _lib as L
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = "cuda:0"
    torch.cuda.set_device(0)
    print(f"build {L.lib().pp_build_id().decode()}  device {torch.cuda.get_device_name(0)}")
    if not args.no_kernel:
        kernel_part(args, L)
    if args.no_step:
        return
    net_kw = dict(block_out_channels=(320, 320, 640, 640), layers_per_block=1) if args.tiny else {}
    arms = []
    for name in ("(i) no adapter", "(ii) no adapter, generic cross-attention chain", "(iii) one adapter"):
        pipe, nets, _ = bench.build_pipeline("v2", dev, 0, 1, net_kw=net_kw)
        unet = nets[0]
        if name.startswith("(ii)"):
            unet.net.fuse_xattn = False            # (what the lab switch PP_XATTN_FUSED=0 sets: no folded cross-attention)
        kw = bench.synthetic_inputs("v2", dev, 0, args.per_gpu, args.latent, args.denoise_steps)
        if name.startswith("(iii)"):
            g = torch.Generator().manual_seed(1)
            D, T = 1024, 4
            width = dict(unet.net._attn_specs())
            ad = {}
            for k_, pre in enumerate(unet.net.ip_attn_order()):
                for n in ("to_k_ip", "to_v_ip"):
                    ad[f"{2 * k_ + 1}.{n}.weight"] = torch.randn(width[pre], 768, generator=g) * 768 ** -0.5
            ip = {"proj.weight": torch.randn(T * 768, D, generator=g) * D ** -0.5, "proj.bias": torch.zeros(T * 768),
                  "norm.weight": torch.ones(768), "norm.bias": torch.zeros(768)}
            pipe.load_ip_adapter({"image_proj": ip, "ip_adapter": ad})
            kw["ip_adapter_image_embeds"] = [torch.randn(2, 1, D, generator=g).to(dev)]
            kw["num_images_per_prompt"] = 1
        arms.append((name, pipe, kw))
    print(f"ppt-v2 batch {args.per_gpu} CFG 7.5 {args.latent * 8}x{args.latent * 8} bf16 {args.denoise_steps} DPM-Solver++ steps, "
          f"hipGraph replay{'  (TINY networks: rehearsal)' if args.tiny else ''}")
    for name, p, kw in arms:
        for _ in range(args.warmup):
            out = p(**kw)[0]
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        names = [c[2] for c in p._loop.program.calls]
        print(f"{name}: launches per step {len(names)} (ip_attn_add {names.count('ip_attn_add')}, xattn_block "
              f"{names.count('xattn_block')}, attention {names.count('attention')}; BrushNet's launches included)")
    times = {name: [] for name, _, _ in arms}
    for r in range(args.reps):
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
        print(f"{name}: ms per denoise step, per round {[round(x, 3) for x in v]}  median {med[name]:.3f}  min {min(v):.3f}  "
              f"max {max(v):.3f}")
    a, b, c = (med[n] for n, _, _ in arms)
    spread = max(max(v) - min(v) for v in times.values())
    print(f"(iii) - (i) = {(c - a) * 1e3:.1f} us per step ({(c / a - 1) * 100:.2f} %), of which (ii) - (i) = {(b - a) * 1e3:.1f} us is the "
          f"price of the generic chain; (iii) - (ii) = {(c - b) * 1e3:.1f} us for the adapter's launches; largest round-to-round "
          f"spread of one arm {spread * 1e3:.1f} us")
    # the adapter's launches, eagerly, an event pair around each (an event pair adds a few microseconds of its own)
    loop = arms[2][1]._loop
    st = torch.cuda.current_stream()
    idx = [i for i, c_ in enumerate(loop.program.calls) if c_[2] == "ip_attn_add"]
    per = []
    for _ in range(5):
        loop.scheduler.reset()
        loop.program.run_timed(st)
        per.append([loop.program.last_launch_ms[i] * 1e3 for i in idx])
    loop.scheduler.reset()
    m = [statistics.median(col) for col in zip(*per)]
    print(f"{len(idx)} pp_ip_attn_add launches inside one eager step, event-timed: sum {sum(m):.1f} us, per launch "
          f"{[round(x, 1) for x in m]}")
    for _, p, _ in arms:
        p._loop.flush_faults()


if __name__ == "__main__":
    main()
