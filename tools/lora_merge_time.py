"""Time of a LoRA re-merge of the full SD-1.5 UNet on the device against the only alternative without pp_lora_merge
(`load_state_dict` of a host-merged state dict), and of the first pipeline call after `set_adapters` against the second.

    python tools/lora_merge_time.py [--out FILE] [--skip-pipeline] [--once CASE]

Each re-merge is timed wall clock around a device synchronisation (median of 10 after 2 warm-ups; every timed merge
changes the adapter weight, so nothing is skipped as unchanged).  `--once attn16|all64` runs ONE re-merge of that case
and nothing else: the command to put behind `rocprofv3 --kernel-trace --stats --`.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import models as PM  # noqa: E402
from powerpaint_amd import pipelines as PP  # noqa: E402
from powerpaint_amd import schedulers as PS  # noqa: E402
from powerpaint_amd.lora import unet_targets  # noqa: E402

DEV = "cuda"


def make_factors(targets, weights, rank, seed, rel=0.1, modules=None):
    """{module: (down, up, alpha = rank)}: seeded normal factors, the delta U D scaled to rms = rel * rms(W) of its module."""
    g = torch.Generator("cpu").manual_seed(seed)
    out = {}
    for m in (modules if modules is not None else targets):
        shp = tuple(targets[m])
        down, up = torch.randn(rank, *shp[1:], generator=g), torch.randn(shp[0], rank, generator=g)
        rms = (up @ down.reshape(rank, -1)).pow(2).mean().sqrt().item()
        out[m] = (down, up * (rel * weights[m + ".weight"].pow(2).mean().sqrt().item() / rms), float(rank))
    return out


def merged_on_host(weights, fac, w):
    """"<module>.weight" -> W + w * (alpha / r) U D in fp32 on the host: what a user without the device merge would do."""
    out = {}
    for m, (down, up, alpha) in fac.items():
        k, r = m + ".weight", down.shape[0]
        out[k] = weights[k] + (w * alpha / r) * (up @ down.reshape(r, -1)).reshape(weights[k].shape)
    return out


def timed(fn, n=10, warm=2):
    ts = []
    for i in range(warm + n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(i)
        torch.cuda.synchronize()
        if i >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--once", default=None, choices=["attn16", "all64"])
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    h = PM.UNet2DConditionModel(in_channels=9, device=DEV)
    sd = h.net.synthetic_state_dict(seed=0)
    h.load_state_dict(sd, keep_state_dict=True)
    targets = unet_targets(h.net)
    attn = [m for m in targets if ".attn1." in m or ".attn2." in m]
    cases = {"attn16": ("rank 16, attention projections only (128 modules)", make_factors(targets, sd, 16, 1, modules=attn)),
             "all64": (f"rank 64, all {len(targets)} targets", make_factors(targets, sd, 64, 2))}
    say(f"build {L.build_id()}  device {torch.cuda.get_device_name(0)}  SD-1.5 UNet (9 input channels), bf16, "
        f"parameter buffer {h.param_buffer().numel() / 1e9:.2f} GB")
    if a.once:
        h.load_lora_adapter(cases[a.once][1], "x")
        h.merge_adapters(1.0)
        torch.cuda.synchronize()
        h.set_adapters(["x"], [0.5])
        h.merge_adapters(1.0)                    # <- the re-merge a kernel trace is read for (the second of two)
        torch.cuda.synchronize()
        return
    for key, (what, fac) in cases.items():
        h.load_lora_adapter(fac, key)
        h.set_adapters([key], [1.0])

        def merge(i):
            h.set_adapters([key], [1.0 + 0.01 * (i + 1)])
            h.merge_adapters(1.0)

        med, lo, hi = timed(merge)
        say(f"re-merge on the device, {what}: median {med:.2f} ms (min {lo:.2f}, max {hi:.2f}; 10 after 2 warm-ups, "
            f"{h.net.repack_launches} pp_lora_merge launches)")
        # the alternative: merge on the host into a state dict, pack it on the host, upload
        def reload(i):
            h2.load_state_dict({**sd, **merged_on_host(sd, fac, 1.0 + 0.01 * (i + 1))})

        h.delete_adapters(key)
        if key == "attn16":
            h2 = PM.UNet2DConditionModel(in_channels=9, device=DEV)
            m2, lo2, hi2 = timed(reload, n=3, warm=1)
            say(f"load_state_dict of a host-merged state dict, {what}: median {m2:.0f} ms (min {lo2:.0f}, max {hi2:.0f}; "
                f"3 after 1 warm-up) -> the device merge is {m2 / med:.0f}x faster; one 50-step batch of 4 images is about 440 ms")
            del h2
    if not a.skip_pipeline:
        pipe = PP.StableDiffusionInpaintPipeline(unet=h, scheduler=PS.DDIMScheduler())
        B, s = 4, 64
        g = torch.Generator("cpu").manual_seed(0)
        kw = dict(prompt_embeds=torch.randn(B, 77, 768, generator=g).to(DEV),
                  negative_prompt_embeds=torch.randn(B, 77, 768, generator=g).to(DEV), height=s * 8, width=s * 8,
                  num_inference_steps=50, guidance_scale=7.5, latents=torch.randn(B, 4, s, s, generator=g).to(DEV),
                  mask_latents=torch.ones(B, 1, s, s).to(DEV), masked_image_latents=torch.randn(B, 4, s, s, generator=g).to(DEV),
                  output_type="latent", return_dict=False)
        h.load_lora_adapter(cases["attn16"][1], "p")

        def call():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe(**kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        call(), call()                                  # plans, graphs, caches
        for w in (0.5, 0.8):
            h.set_adapters(["p"], [w])
            first, second = call(), call()
            say(f"pipeline call (50 DDIM steps, batch 4, 64x64 latents) after set_adapters(weight {w}): first {first:.1f} ms, "
                f"second {second:.1f} ms, difference {first - second:.1f} ms (re-merge + one re-capture of the loop)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
