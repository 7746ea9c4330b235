#!/usr/bin/env python
"""Generate tests/golden/ref_asym_vae.json: what the REFERENCE'S OWN `__call__`s hand to `vae.decode` when the VAE is an
AsymmetricAutoencoderKL, and where they leave the caller's generator.  `StableDiffusionInpaintPipeline.__call__` branches on the
class (pipeline_PowerPaint.py:1041-1051).  `StableDiffusionControlNetInpaintPipeline.__call__` does not
(pipeline_PowerPaint_ControlNet.py:1750-1751 decodes without keyword arguments; the branch at :1317-1325 of that file sits in
`predict_woControl`, which nothing calls): the fixture records that too -- no `image`, no `mask`, generator untouched by a
posterior draw.

The pipelines run through oracle/ref_pipeline.py on the components and inputs of make_ref_pipeline_call.py, with a recording
VAE whose class derives from the `AsymmetricAutoencoderKL` the loaded module's globals hold (so the reference's `isinstance`
branch is taken).  It encodes with the oracle's AutoencoderKL; its `decode` records the keyword arguments it received --
shape, dtype and SHA-256 of `image` and `mask` -- and the generator's state at that moment, then ends the call (nothing
behind the decode touches either).  Results only: no reference text goes into the fixture."""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_ref_pipeline_call as MR  # noqa: E402
from oracle import schedulers as OS, sd_modules as OM  # noqa: E402


class DecodeReached(Exception):
    pass


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def describe(t: torch.Tensor) -> dict:
    return dict(shape=list(t.shape), dtype=str(t.dtype), sha256=sha(t))


def generator_state(g) -> list:
    return [sha(x.get_state()) for x in (g if isinstance(g, list) else [g])]


def recording_vae(base_cls, inner, generator):
    class RecordingVAE(base_cls):
        def __init__(self):
            self.config = inner.config
            self.dtype = torch.float32
            self.seen = None

        def encode(self, x):
            return inner.encode(x)

        def decode(self, z, return_dict=True, **kw):
            self.seen = dict(latents=list(z.shape), kwargs=sorted(kw), generator=generator_state(generator),
                             **{k: describe(kw[k]) for k in ("image", "mask") if k in kw})
            raise DecodeReached()

    return RecordingVAE()


def mask_two_boxes():
    m = torch.zeros(1, 1, 128, 128)
    m[:, :, 8:40, 60:120] = 1.0
    m[:, :, 70:110, 10:50] = 1.0
    return m


def cases():
    """name -> (pipeline kind, generator factory, mask, extra call arguments)"""
    _, mask, _ = MR.inputs()
    return {
        "v1": ("v1", lambda: torch.Generator().manual_seed(5), mask, {}),
        "v1_generator_list": ("v1", lambda: [torch.Generator().manual_seed(7)], mask_two_boxes(), {}),
        "v1_strength": ("v1", lambda: torch.Generator().manual_seed(11), mask, dict(strength=0.6, num_inference_steps=5,
                                                                                  latents=None)),
        "controlnet": ("cn", lambda: torch.Generator().manual_seed(5), mask, {}),
    }


def run_reference(kind, generator, mask, extra):
    from oracle import ref_pipeline
    img, _, lat = MR.inputs()
    if kind == "v1":
        Pipe, _ = ref_pipeline.load_reference_pipeline_class()
        tok, enc, unet, vae = MR.components()
        rec = recording_vae(Pipe._encode_vae_image.__globals__["AsymmetricAutoencoderKL"], vae, generator)
        pipe = Pipe(vae=rec, text_encoder=enc, tokenizer=tok, unet=unet, scheduler=OS.DDIMScheduler(), safety_checker=None,
                    feature_extractor=None, requires_safety_checker=False)
        kw = dict(MR.CALL, image=img, mask=mask, latents=lat.clone())
    else:
        Pipe = ref_pipeline.load_reference_controlnet_pipeline_class(OM.ControlNetModel)
        tok, enc, unet, cn, vae = MR.components_cn()
        rec = recording_vae(Pipe._encode_vae_image.__globals__["AsymmetricAutoencoderKL"], vae, generator)
        pipe = Pipe(vae=rec, text_encoder=enc, tokenizer=tok, unet=unet, controlnet=cn, scheduler=OS.DDIMScheduler(),
                    safety_checker=None, feature_extractor=None, requires_safety_checker=False)
        kw = dict(MR.CALL_CN, image=img, mask=mask, control_image=MR.control_image(), latents=lat.clone())
    kw.update(extra)
    try:
        with torch.no_grad():
            pipe(generator=generator, output_type="pt", return_dict=False, **kw)
    except DecodeReached:
        pass
    assert rec.seen is not None, "the reference did not reach vae.decode"
    return rec.seen


def main():
    out = {}
    for name, (kind, gen, mask, extra) in cases().items():
        out[name] = run_reference(kind, gen(), mask, extra)
        print(name, out[name])
    with open(os.path.join(HERE, "ref_asym_vae.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
