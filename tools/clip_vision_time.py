"""Time of the CLIP vision tower's launch plan on one MI355X, beside transformers' own module in bf16 on the same GPU (what a
user registers as `image_encoder` today).  Random weights: the time does not depend on them.

    python tools/clip_vision_time.py [--out profiles/clip_vision.txt] [--reps 20]

Two shapes: the ViT-H/14 widths at two layers and batch 3 (the largest case of tests/test_clip_vision.py) and the full 32-layer
ViT-H/14 at batch 1.  Per shape, after warm-up: the median over --reps of (a) the plan replayed eagerly with a device-event pair
around every launch (Plan.run_timed: the sum of the kernels' times, launch gaps excluded), (b) one event pair around the whole
eager replay (launch gaps included: what a caller waits for), (c) one event pair around transformers' forward.  The two modules
alternate inside every repetition, so that both see the same state of the box.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd.models import CLIPVisionModelWithProjection  # noqa: E402

VIT_H = dict(hidden_size=1280, num_attention_heads=16, intermediate_size=5120, image_size=224, patch_size=14, projection_dim=1024)


def _wall(fn, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    stream.synchronize()
    return e0.elapsed_time(e1)


def measure(layers: int, batch: int, reps: int, warm: int = 3):
    import transformers
    cfg = dict(VIT_H, num_hidden_layers=layers)
    torch.manual_seed(0)
    hf = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(hidden_act="gelu", **cfg)).eval()
    m = CLIPVisionModelWithProjection(device="cuda", **cfg)
    m.load_state_dict(hf.state_dict())
    hf = hf.to("cuda", torch.bfloat16)
    px = torch.randn(batch, 3, 224, 224, device="cuda")
    px16 = px.bfloat16()
    stream = torch.cuda.current_stream()
    with torch.no_grad():
        for _ in range(warm):
            got = m(px).image_embeds
            want = hf(pixel_values=px16).image_embeds
        cos = torch.nn.functional.cosine_similarity(got.flatten().float(), want.flatten().float(), dim=0).item()
        rt = m._rt
        kern, wall, ref = [], [], []
        by_name = {}
        for _ in range(reps):
            t = rt.plan.run_timed(stream)
            kern.append(sum(t.values()))
            for k, v in t.items():
                by_name.setdefault(k, []).append(v)
            wall.append(_wall(lambda: rt.plan.run(stream.cuda_stream), stream))
            ref.append(_wall(lambda: hf(pixel_values=px16), stream))
    med = statistics.median
    names = ", ".join(f"{k} {med(v):.3f}" for k, v in sorted(by_name.items(), key=lambda kv: -med(kv[1])))
    return dict(layers=layers, batch=batch, launches=len(rt.plan.calls), kern=med(kern), wall=med(wall), ref=med(ref),
                kern_min=min(kern), wall_min=min(wall), ref_min=min(ref), cos=cos, names=names,
                tflops=rt.plan.flops / med(kern) * 1e-9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_vision.txt"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = [f"# tools/clip_vision_time.py on one {torch.cuda.get_device_name(0)}, build {L.build_id()}: the CLIP vision tower's plan (bf16)",
             "# beside transformers.CLIPVisionModelWithProjection in bf16 on the same GPU, alternating; ms, median (min) over "
             f"{a.reps} repetitions after warm-up.",
             "# kernels = sum of per-launch device-event times (Plan.run_timed); replay = one event pair around the eager replay",
             "# (launch gaps included); image_embeds cosine between the two modules as a sanity check of the timed work."]
    for layers, batch in ((2, 3), (32, 1)):
        r = measure(layers, batch, a.reps)
        lines.append(f"[clip_vision] ViT-H/14 widths, {r['layers']} layers, batch {r['batch']}, {r['launches']} launches: kernels "
                     f"{r['kern']:.3f} ({r['kern_min']:.3f}) ms = {r['tflops']:.0f} TFLOP/s of the plan's matmul FLOPs; replay {r['wall']:.3f} "
                     f"({r['wall_min']:.3f}) ms; transformers bf16 eager {r['ref']:.3f} ({r['ref_min']:.3f}) ms; cosine {r['cos']:.5f}")
        lines.append(f"[clip_vision]   per launch name, ms: {r['names']}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
