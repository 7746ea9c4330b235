#!/usr/bin/env python
"""Generate the fixtures of the several-ControlNets path from the REFERENCE'S OWN code (run through oracle/ref_pipeline.py):

  ref_pipeline_call_multicn.pt   final latents of `StableDiffusionControlNetInpaintPipeline.__call__`
                                 (pipeline_PowerPaint_ControlNet.py:1349-1760) with a LIST of two ControlNets, per-net scales
                                 [0.5, 0.8], four DDIM steps; three calls: plain; per-net guidance windows
                                 start = [0.0, 0.25], end = [0.5, 0.75] (active nets per step: {0}, {0, 1}, {1}, {});
                                 guess_mode=True.
  ref_multicn_check_inputs.json  what the reference's `check_inputs` (:651-789) answers, behind the list normalisation of
                                 `__call__` (:1493-1503), to a table of control images / scales / windows: exception type and
                                 message, or null.

`oracle/ref_pipeline.load_reference_controlnet_pipeline_class` stubs `MultiControlNetModel` with an empty class (the
reference imports it from diffusers, which is not installed).  After loading, a real class is put into the loaded
pipeline's module namespace: `MultiControlNetModel` below RESTATES the diffusers 0.27 wrapper
(diffusers/pipelines/controlnet/multicontrolnet.py: `nets = ModuleList(...)`, a `forward` that calls every net with its own
image and scale and adds the results) like the other diffusers leaves of the oracle -- parity unpinned for that leaf
(tests/golden/README_multi_controlnet.md says the same beside the fixture rows).
Components: `components_cn()` of make_ref_pipeline_call.py plus a second tiny ControlNet and a second control image made
the same way under other seeds (shared with the tests: `second_controlnet()`, `control_image2()`)."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import make_ref_pipeline_call as M  # noqa: E402
from oracle import schedulers as OS, sd_modules as OM  # noqa: E402

CALL_MCN = dict(M.CALL_CN, num_inference_steps=4, controlnet_conditioning_scale=[0.5, 0.8])
WINDOWS = dict(control_guidance_start=[0.0, 0.25], control_guidance_end=[0.5, 0.75])
CASES = {"plain": {}, "windows": WINDOWS, "guess": dict(guess_mode=True)}


class MultiControlNetModel(torch.nn.Module):
    """diffusers 0.27 `MultiControlNetModel`, restated."""

    def __init__(self, controlnets):
        super().__init__()
        self.nets = torch.nn.ModuleList(controlnets)

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    def forward(self, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale, class_labels=None,
                timestep_cond=None, attention_mask=None, added_cond_kwargs=None, cross_attention_kwargs=None,
                guess_mode=False, return_dict=True):
        for i, (image, scale, controlnet) in enumerate(zip(controlnet_cond, conditioning_scale, self.nets)):
            down_samples, mid_sample = controlnet(sample, timestep, encoder_hidden_states, image, scale,
                                                  guess_mode=guess_mode, return_dict=False)
            if i == 0:
                down_block_res_samples, mid_block_res_sample = down_samples, mid_sample
            else:
                down_block_res_samples = [a + b for a, b in zip(down_block_res_samples, down_samples)]
                mid_block_res_sample = mid_block_res_sample + mid_sample
        return down_block_res_samples, mid_block_res_sample


def second_controlnet():
    torch.manual_seed(38)
    return OM.randomize_zero_convs(M.bf16_(OM.ControlNetModel(
        in_channels=4, **{k: v for k, v in M.TINY.items() if k != "up_block_types"}))).eval()


def control_image2():
    return torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(43))


def reference_pipeline_class():
    from oracle import ref_pipeline
    Pipe = ref_pipeline.load_reference_controlnet_pipeline_class(OM.ControlNetModel)
    Pipe.__init__.__globals__["MultiControlNetModel"] = MultiControlNetModel      # (`__call__` is wrapped by no_grad)
    return Pipe


def reference_pipeline(nets=None):
    Pipe = reference_pipeline_class()
    tok, enc, unet, cn, vae = M.components_cn()
    nets = [cn, second_controlnet()] if nets is None else nets
    return Pipe(vae=vae, text_encoder=enc, tokenizer=tok, unet=unet, controlnet=nets, scheduler=OS.DDIMScheduler(),
                safety_checker=None, feature_extractor=None, requires_safety_checker=False)


def main():
    pipe = reference_pipeline()
    assert isinstance(pipe.controlnet, MultiControlNetModel)
    img, mask, lat = M.inputs()
    out = {}
    for name, extra in CASES.items():
        with torch.no_grad():
            out[name] = pipe(image=img, mask=mask, control_image=[M.control_image(), control_image2()], latents=lat.clone(),
                             generator=torch.Generator().manual_seed(5), output_type="latent", return_dict=False,
                             **CALL_MCN, **extra)[0]
        print(name, tuple(out[name].shape), float(out[name].abs().max()))
    torch.save(out, os.path.join(HERE, "ref_pipeline_call_multicn.pt"))
    cos = lambda a, b: float(torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0))   # noqa: E731
    print("cosine plain / windows", cos(out["plain"], out["windows"]), "plain / guess", cos(out["plain"], out["guess"]))


# ---- check_inputs table.  Images are named, not stored: "t" = a [1,3,128,128] tensor, lists of names nest as written.
_T = "t"
CHECK_CASES = [
    # (control_image, controlnet_conditioning_scale, control_guidance_start, control_guidance_end)
    ([_T, _T], [0.5, 0.8], 0.0, 1.0),
    ([_T, _T], 0.5, 0.0, 1.0),
    ([_T, _T], [0.5, 0.8], [0.0, 0.25], [0.5, 0.75]),
    ([_T, _T], [0.5, 0.8], 0.1, [0.5, 0.75]),
    ([_T, _T], [0.5, 0.8], [0.0, 0.25], 0.9),
    (_T, [0.5, 0.8], 0.0, 1.0),                                  # not a list
    ([[_T, _T], [_T, _T]], [0.5, 0.8], 0.0, 1.0),                # nested
    ([_T, [_T]], [0.5, 0.8], 0.0, 1.0),                          # nested, second entry
    ([_T], [0.5, 0.8], 0.0, 1.0),                                # too few images
    ([_T, _T, _T], [0.5, 0.8], 0.0, 1.0),                        # too many images
    ([_T, _T], [[0.5], [0.8]], 0.0, 1.0),                        # nested scales
    ([_T, _T], [0.5], 0.0, 1.0),                                 # (scale list of another length: the branch that cannot fire)
    ([_T, _T], [0.5, 0.8, 0.1], 0.0, 1.0),                       # (likewise)
    ([_T, _T], [0.5, 0.8], [0.0, 0.25], [0.5]),                  # unequal lengths
    ([_T, _T], [0.5, 0.8], [0.0], [0.5]),                        # equal, not len(nets)
    ([_T, _T], [0.5, 0.8], [0.0, 0.1, 0.2], [0.5, 0.6, 0.7]),
    ([_T, _T], [0.5, 0.8], 0.2, [0.5, 0.6, 0.7]),                # scalar broadcast to a wrong length
    ([_T, _T], [0.5, 0.8], [0.0, 0.6], [0.5, 0.6]),              # start == end
    ([_T, _T], [0.5, 0.8], [0.0, 0.7], [0.5, 0.6]),              # start > end
    ([_T, _T], [0.5, 0.8], [-0.1, 0.0], [0.5, 0.6]),             # start < 0
    ([_T, _T], [0.5, 0.8], [0.0, 0.1], [0.5, 1.1]),              # end > 1
    ([_T, _T], [0.5, 0.8], 0.5, 0.5),                            # scalars, start == end
    ([_T, _T], [0.5, 0.8], -0.5, 1.0),
    ([_T, _T], [0.5, 0.8], 0.0, 1.5),
]


def build_images(spec):
    if isinstance(spec, list):
        return [build_images(s) for s in spec]
    return torch.zeros(1, 3, 128, 128)


def normalise_like_call(start, end, n_nets):
    """pipeline_PowerPaint_ControlNet.py:1493-1503 for a MultiControlNetModel, restated (the reference runs it inline in
    `__call__`, in front of `check_inputs`)."""
    if not isinstance(start, list) and isinstance(end, list):
        start = len(end) * [start]
    elif not isinstance(end, list) and isinstance(start, list):
        end = len(start) * [end]
    elif not isinstance(start, list) and not isinstance(end, list):
        start, end = n_nets * [start], n_nets * [end]
    return start, end


def main_check_inputs():
    pipe = reference_pipeline()
    rows = []
    for image, scale, start, end in CHECK_CASES:
        s, e = normalise_like_call(start, end, 2)
        try:
            pipe.check_inputs("a prompt", build_images(image), 128, 128, 1, None, None, None, scale, s, e)
            res = None
        except Exception as ex:                                   # noqa: BLE001  (the type is the datum)
            res = {"type": type(ex).__name__, "message": str(ex)}
        rows.append(dict(control_image=image, controlnet_conditioning_scale=scale, control_guidance_start=start,
                         control_guidance_end=end, result=res))
        print(image, scale, start, end, "->", res)
    with open(os.path.join(HERE, "ref_multicn_check_inputs.json"), "w") as f:
        json.dump(dict(n_nets=2, cases=rows), f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "check_inputs":
        main_check_inputs()
        sys.exit(0)
    main()
    main_check_inputs()
