#!/usr/bin/env python
"""What `ip_adapter_masks` cost (and return) per launch and per denoising step -- the method of tools/ip_adapter_cost.py:
arms built once, timed ALTERNATING on one box, `--reps` rounds, the spread of every arm reported.

1. Per launch at the four levels of the headline shape (batch 8 = 4 images x CFG, nk = 4, bf16), three arms:
     (a) pp_ip_attn_add                                   -- the parent's unmasked entry;
     (b) pp_ip_attn_add_masked, weights all 1.0           -- the price of the weight read;
     (c) pp_ip_attn_add_masked, a half-frame rectangle    -- IPAdapterMaskProcessor.downsample of a 512x512 mask whose left
                                                             half is 1: what the zero-row skip returns.
   Each round times `--launches` back-to-back launches of one arm between device events, cold (a ring of q / o buffers larger
   than the 256 MB last-level cache) and hot (one buffer set: what the step sees, q and o written right in front).
2. ms per denoising step of the ppt-v2 headline (BrushNet + UNet, batch 4, CFG 7.5, 512x512, bf16, 50 DPM-Solver++ steps,
   hipGraph replay, bench.py's synthetic inputs), four arms: one adapter unmasked / with a full (all-ones) mask, two adapters
   unmasked / with complementary halves.
   A record, not a gate:   python tools/ip_adapter_masks_cost.py > profiles/ip_adapter_masks_step.txt
"""
import argparse
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def half_frame(size=512):
    m = torch.zeros(1, size, size)
    m[:, :, :size // 2] = 1.0
    return m


def kernel_part(args, L):
    from powerpaint_amd.pipelines.image_processor import IPAdapterMaskProcessor
    lib = L.lib()
    dt = torch.bfloat16
    st = torch.cuda.current_stream().cuda_stream
    print(f"per launch, batch {args.batch}, nk {args.nk}, bf16, {args.launches} launches per window (device events), "
          f"{args.reps} alternating rounds: median [min .. max] us")
    for hw, C in ((64, 320), (32, 640), (16, 1280), (8, 1280)):
        nq, heads, d = hw * hw, 8, C // 8
        M = args.batch * nq
        ring = max(2, int(600e6 // (2 * M * C * 2)) + 1)
        k = torch.randn(args.batch, args.nk, C, device="cuda").to(dt)
        v = torch.randn(args.batch, args.nk, C, device="cuda").to(dt)
        ones = torch.ones(nq, device="cuda")
        half = IPAdapterMaskProcessor.downsample(half_frame(), 1, nq, 1).reshape(nq).cuda()
        zero_rows = int((half == 0).sum())
        arms = (("unmasked", None), ("masked, all ones", ones), ("masked, half frame", half))
        for mode, n in (("cold (HBM ring)", ring), ("hot (one buffer set)", 1)):
            qs = [torch.randn(M, C, device="cuda").to(dt) for _ in range(n)]
            os_ = [torch.randn(M, C, device="cuda").to(dt) for _ in range(n)]

            def run(w, count):
                for i in range(count):
                    q, o = qs[i % n].data_ptr(), os_[i % n].data_ptr()
                    if w is None:
                        rc = lib.pp_ip_attn_add(q, C, k.data_ptr(), v.data_ptr(), o, C, args.batch, heads, nq, args.nk, d,
                                                d ** -0.5, 1e-3, L.PP_DT_BF16, st)
                    else:
                        rc = lib.pp_ip_attn_add_masked(q, C, k.data_ptr(), v.data_ptr(), o, C, args.batch, heads, nq, args.nk,
                                                       d, d ** -0.5, 1e-3, w.data_ptr(), L.PP_DT_BF16, st)
                    L.check(rc, "ip_attn_add")

            times = {name: [] for name, _ in arms}
            for name, w in arms:
                run(w, max(n, 10))
            torch.cuda.synchronize()
            for _ in range(args.reps):
                for name, w in arms:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run(w, args.launches)
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / args.launches)
            med = {nm: statistics.median(t) for nm, t in times.items()}
            spread = max(max(t) - min(t) for t in times.values())
            print(f"  {hw}x{hw} C {C} (M {M}, d {d}; {zero_rows} of {nq} half-frame rows are 0) {mode}: " +
                  ";  ".join(f"{nm} {med[nm]:.2f} [{min(t):.2f} .. {max(t):.2f}]" for nm, t in times.items()) +
                  f";  all ones - unmasked {med['masked, all ones'] - med['unmasked']:+.2f} us, all ones - half frame "
                  f"{med['masked, all ones'] - med['masked, half frame']:+.2f} us, largest spread of an arm {spread:.2f} us")
            del qs, os_


def adapter(unet, g, D=1024, T=4):
    width = dict(unet.net._attn_specs())
    ad = {}
    for k_, pre in enumerate(unet.net.ip_attn_order()):
        for n in ("to_k_ip", "to_v_ip"):
            ad[f"{2 * k_ + 1}.{n}.weight"] = torch.randn(width[pre], 768, generator=g) * 768 ** -0.5
    ip = {"proj.weight": torch.randn(T * 768, D, generator=g) * D ** -0.5, "proj.bias": torch.zeros(T * 768),
          "norm.weight": torch.ones(768), "norm.bias": torch.zeros(768)}
    return {"image_proj": ip, "ip_adapter": ad}


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
    warnings.simplefilter("ignore")
    print(f"build {L.lib().pp_build_id().decode()}  device {torch.cuda.get_device_name(0)}")
    if not args.no_kernel:
        kernel_part(args, L)
    if args.no_step:
        return
    net_kw = dict(block_out_channels=(320, 320, 640, 640), layers_per_block=1) if args.tiny else {}
    size = args.latent * 8
    left = half_frame(size)
    specs = (("one adapter, unmasked", 1, None), ("one adapter, full mask", 1, torch.ones(1, 1, size, size)),
             ("two adapters, unmasked", 2, None), ("two adapters, complementary halves", 2, torch.stack([left, 1.0 - left])))
    arms = []
    for name, n_ad, masks in specs:
        pipe, nets, _ = bench.build_pipeline("v2", dev, 0, 1, net_kw=net_kw)
        unet = nets[0]
        kw = bench.synthetic_inputs("v2", dev, 0, args.per_gpu, args.latent, args.denoise_steps)
        g = torch.Generator().manual_seed(1)
        pipe.load_ip_adapter([adapter(unet, g) for _ in range(n_ad)])
        kw["ip_adapter_image_embeds"] = [torch.randn(2, 1, 1024, generator=g).to(dev) for _ in range(n_ad)]
        kw["num_images_per_prompt"] = 1
        if masks is not None:
            kw["cross_attention_kwargs"] = dict(kw.get("cross_attention_kwargs") or {}, ip_adapter_masks=masks)
        arms.append((name, pipe, kw))
    print(f"ppt-v2 batch {args.per_gpu} CFG 7.5 {size}x{size} bf16 {args.denoise_steps} DPM-Solver++ steps, hipGraph replay"
          f"{'  (TINY networks: rehearsal)' if args.tiny else ''}")
    lib = L.lib()
    for name, p, kw in arms:
        for _ in range(args.warmup):
            out = p(**kw)[0]
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        ip_calls = [c for c in p._loop.program.calls if c[2] == "ip_attn_add"]
        print(f"{name}: launches per step {len(p._loop.program.calls)} (ip_attn_add {len(ip_calls)}, of them masked "
              f"{sum(c[0] is lib.pp_ip_attn_add_masked for c in ip_calls)})")
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
    a, b, c, d = (med[n] for n, _, _ in arms)
    spread = max(max(v) - min(v) for v in times.values())
    print(f"full mask - unmasked (one adapter) = {(b - a) * 1e3:+.1f} us per step ({(b / a - 1) * 100:+.2f} %); complementary halves - "
          f"unmasked (two adapters) = {(d - c) * 1e3:+.1f} us per step ({(d / c - 1) * 100:+.2f} %); largest round-to-round spread of "
          f"one arm {spread * 1e3:.1f} us (the per-call mask preparation on the host, 4 resizes per adapter, is inside the figures)")
    for _, p, _ in arms:
        p._loop.flush_faults()


if __name__ == "__main__":
    main()
