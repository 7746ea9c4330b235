#!/usr/bin/env python
"""What an IP-Adapter Plus costs: per denoising step, and once per call in the setup plan's Resampler.

1. ms per denoising step of the ppt-v2 headline (BrushNet + UNet, batch 4, CFG 7.5, 512x512, bf16, 50 DPM-Solver++ steps,
   hipGraph replay, the synthetic inputs of bench.py) -- the method of tools/ip_adapter_cost.py: four arms built once and
   timed ALTERNATING, `--reps` rounds of one pipeline call each behind `--warmup` untimed calls:
     (i)   the plan of a UNet without adapters;
     (ii)  one base adapter (4 tokens, image-embed dimension 1024);
     (iii) one Plus adapter of the ip-adapter-plus_sd15 sizes (Q 16, dim 768, E 1280, depth 4, 12 heads, ff 3072), one image:
           16 keys per pp_ip_attn_add;
     (iv)  the same with four images per prompt: 64 keys.
   A pipeline call includes the setup plan (once per call), so arms (iii) / (iv) carry the Resampler's share of one call spread
   over the steps.
2. The Resampler part of arm (iii)'s setup plan (batch 8 after CFG, one image, 257 hidden states): ms per pass over its
   10 depth + 3 launches, device events around `--passes` back-to-back passes, and -- from an event pair around every launch
   (which adds a few microseconds of its own to each) -- the share of the four pp_perceiver_attn launches and of the GEMMs.
   A record, not a gate:   python tools/ip_adapter_plus_cost.py > profiles/ip_adapter_plus_step.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SD15_PLUS = dict(Q=16, dim=768, E=1280, depth=4, heads=12, ff=3072)
S = 257


def kv_pairs(net, g):
    width = dict(net._attn_specs())
    return {f"{2 * k + 1}.{n}.weight": torch.randn(width[pre], 768, generator=g) * 768 ** -0.5
            for k, pre in enumerate(net.ip_attn_order()) for n in ("to_k_ip", "to_v_ip")}


def base_adapter(net, g, D=1024, T=4):
    ip = {"proj.weight": torch.randn(T * 768, D, generator=g) * D ** -0.5, "proj.bias": torch.zeros(T * 768),
          "norm.weight": torch.ones(768), "norm.bias": torch.zeros(768)}
    return {"image_proj": ip, "ip_adapter": kv_pairs(net, g)}


def plus_adapter(net, g, Q, dim, E, depth, heads, ff):
    from powerpaint_amd.ip_adapter import plus_image_proj_shapes
    ip = {}
    for k, shp in plus_image_proj_shapes(Q, dim, E, 768, depth, heads * 64, ff).items():
        if k.endswith("bias"):
            ip[k] = torch.zeros(shp)
        elif len(shp) == 1:
            ip[k] = torch.ones(shp)
        else:
            ip[k] = torch.randn(shp, generator=g) * (1.0 if k == "latents" else shp[-1] ** -0.5)
    return {"image_proj": ip, "ip_adapter": kv_pairs(net, g)}


def resampler_part(pipe, passes):
    from powerpaint_amd.engine import Plan
    rt = pipe._loop.rt
    n_res = 10 * SD15_PLUS["depth"] + 3
    sub = Plan()
    sub.calls = rt.setup_plan.calls[:n_res]
    names = [c[2] for c in sub.calls]
    assert names.count("perceiver_attn") == SD15_PLUS["depth"] and names[-1] == "layernorm" and names[0] == "linear", names
    att = [c[1] for c in sub.calls if c[2] == "perceiver_attn"][0]
    st = torch.cuda.current_stream()
    for _ in range(3):
        sub.run(st.cuda_stream)
    torch.cuda.synchronize()
    wins = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(passes):
            sub.run(st.cuda_stream)
        e1.record()
        torch.cuda.synchronize()
        wins.append(e0.elapsed_time(e1) / passes)
    per = []
    for _ in range(7):
        sub.run_timed(st)
        per.append(list(sub.last_launch_ms))
    m = [statistics.median(col) * 1e3 for col in zip(*per)]
    by = {}
    for n, us in zip(names, m):
        by[n] = by.get(n, 0.0) + us
    total = sum(m)
    print(f"Resampler part of the setup plan, batch {att[10]}, {att[4]} + {att[7]} keys, {att[11]} heads of {att[13]}, {n_res} "
          f"launches: {statistics.median(wins) * 1e3:.1f} us per pass (median of 5 windows of {passes} back-to-back passes, "
          f"min {min(wins) * 1e3:.1f}, max {max(wins) * 1e3:.1f})")
    print(f"  an event pair around every launch: sum {total:.1f} us; " +
          "; ".join(f"{n} {us:.1f} us ({100 * us / total:.1f} %, {names.count(n)} launches)" for n, us in sorted(by.items())))
    print(f"  the {names.count('perceiver_attn')} pp_perceiver_attn launches: "
          f"{[round(us, 1) for n, us in zip(names, m) if n == 'perceiver_attn']} us; the GEMMs around each (to_q, to_kv image rows, "
          f"to_kv latent rows | to_out): {[round(us, 1) for us in m[3:6] + m[7:8]]} us in the first layer")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-gpu", type=int, default=4)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--denoise-steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--passes", type=int, default=50)
    ap.add_argument("--tiny", action="store_true", help="reduced networks (a rehearsal of the script, not a measurement)")
    args = ap.parse_args()

    import bench
    from powerpaint_amd import _lib as L
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = "cuda:0"
    torch.cuda.set_device(0)
    print(f"build {L.lib().pp_build_id().decode()}  device {torch.cuda.get_device_name(0)}")
    net_kw = dict(block_out_channels=(320, 320, 640, 640), layers_per_block=1) if args.tiny else {}
    arms = []
    for name in ("(i) no adapter", "(ii) one base adapter", "(iii) one Plus adapter, 16 keys", "(iv) one Plus adapter, four images, 64 keys"):
        pipe, nets, _ = bench.build_pipeline("v2", dev, 0, 1, net_kw=net_kw)
        unet = nets[0]
        kw = bench.synthetic_inputs("v2", dev, 0, args.per_gpu, args.latent, args.denoise_steps)
        g = torch.Generator().manual_seed(1)
        if name.startswith("(ii)"):
            pipe.load_ip_adapter(base_adapter(unet.net, g))
            kw["ip_adapter_image_embeds"] = [torch.randn(2, 1, 1024, generator=g).to(dev)]
        elif not name.startswith("(i)"):
            pipe.load_ip_adapter(plus_adapter(unet.net, g, **SD15_PLUS))
            n = 4 if name.startswith("(iv)") else 1
            kw["ip_adapter_image_embeds"] = [torch.randn(2, n, S, SD15_PLUS["E"], generator=g).to(dev)]
        if "ip_adapter_image_embeds" in kw:
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
        nk = sorted({c[1][9] for c in p._loop.program.calls if c[2] == "ip_attn_add"})
        setup = [c[2] for c in p._loop.rt.setup_plan.calls]
        print(f"{name}: launches per step {len(names)} (ip_attn_add {names.count('ip_attn_add')} with nk {nk}, xattn_block "
              f"{names.count('xattn_block')}, attention {names.count('attention')}; BrushNet's launches included); UNet setup plan "
              f"{len(setup)} launches (perceiver_attn {setup.count('perceiver_attn')})")
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
    print(f"(ii) - (i) = {(b - a) * 1e3:.1f} us per step ({(b / a - 1) * 100:.2f} %); (iii) - (i) = {(c - a) * 1e3:.1f} us "
          f"({(c / a - 1) * 100:.2f} %); (iv) - (i) = {(d - a) * 1e3:.1f} us ({(d / a - 1) * 100:.2f} %); (iii) - (ii) = "
          f"{(c - b) * 1e3:.1f} us, (iv) - (iii) = {(d - c) * 1e3:.1f} us; largest round-to-round spread of one arm "
          f"{spread * 1e3:.1f} us")
    resampler_part(arms[2][1], args.passes)
    for _, p, _ in arms:
        p._loop.flush_faults()


if __name__ == "__main__":
    main()
