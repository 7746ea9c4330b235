"""Several ControlNets in one inpainting call -- the host side (no GPU).

The reference wraps a list of ControlNets in diffusers' `MultiControlNetModel` (pipeline_PowerPaint_ControlNet.py:281,306)
and keeps one control image, one scale and one guidance window per net.  Checked here: the list normalisation and every
input check against the reference's own `check_inputs` (tests/golden/ref_multicn_check_inputs.json, produced by
tests/golden/make_ref_multi_controlnet.py), the per-step scale schedule and the active sets derived from it, and the
construction rules of the wrapper.
"""
import json
import os

import pytest
import torch

from powerpaint_amd import _lib as L
from powerpaint_amd import models as PM, pipelines as PP

HERE = os.path.dirname(os.path.abspath(__file__))
TINY_CN = dict(block_out_channels=(320, 640), layers_per_block=1, down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"))


def _nets(n=2, **kw):
    return [PM.ControlNetModel(in_channels=4, device="cuda", **dict(TINY_CN, **kw)) for _ in range(n)]


def _pipe(nets):
    return PP.StableDiffusionControlNetInpaintPipeline(controlnet=nets)


def _images(spec):
    if isinstance(spec, list):
        return [_images(s) for s in spec]
    return torch.zeros(1, 3, 128, 128)


def test_a_list_or_tuple_of_controlnets_is_wrapped_in_order():
    a, b, c = _nets(3)
    for given in ([a, b, c], (a, b, c)):
        pipe = _pipe(given)
        assert isinstance(pipe.controlnet, PM.MultiControlNetModel)
        assert [id(n) for n in pipe.controlnet.nets] == [id(a), id(b), id(c)]
    w = PM.MultiControlNetModel([b, a])
    assert _pipe(w).controlnet is w and w.nets[0] is b and w.nets[1] is a
    assert w.dtype == torch.bfloat16 and w.device == a.device and w.to(torch.bfloat16) is w
    assert _pipe(a).controlnet is a                                   # a single net stays what it was


def test_wrapper_refuses_nets_that_cannot_share_residual_buffers():
    a = _nets(1)[0]
    with pytest.raises(L.PPError, match="torch.float16"):
        PM.MultiControlNetModel([a, _nets(1, dtype=torch.float16)[0]])
    with pytest.raises(L.PPError, match="block_out_channels"):
        PM.MultiControlNetModel([a, _nets(1, block_out_channels=(320, 1280))[0]])
    with pytest.raises(L.PPError, match="not a ControlNetModel"):
        PM.MultiControlNetModel([a, object()])
    with pytest.raises(L.PPError):
        PM.MultiControlNetModel([])
    with pytest.raises(L.PPError, match="torch.float16"):
        PM.MultiControlNetModel([a, a]).to(torch.float16)              # (as the single net: packed in one format)
    w = PM.MultiControlNetModel([a, a])
    with pytest.raises(L.PPError, match="list of 2"):
        w.per_net([1.0], "conditioning_scale")
    with pytest.raises(L.PPError, match="list of 2"):
        w.per_net(1.0, "conditioning_scale")


def test_input_checks_match_the_reference_check_inputs():
    """Same arguments, same verdict as the reference's `check_inputs` behind its own list normalisation: exception type and
    message, or acceptance.  Rejections are also raised by `__call__` itself, before anything else happens."""
    with open(os.path.join(HERE, "golden", "ref_multicn_check_inputs.json")) as f:
        gold = json.load(f)
    pipe = _pipe(_nets(gold["n_nets"]))
    assert len(gold["cases"]) >= 24 and sum(c["result"] is None for c in gold["cases"]) >= 5
    for c in gold["cases"]:
        img, sc = _images(c["control_image"]), c["controlnet_conditioning_scale"]
        st, en = c["control_guidance_start"], c["control_guidance_end"]

        def check():
            s, e = pipe.align_control_guidance(st, en, gold["n_nets"])
            pipe.check_multi_control_inputs(img, sc, s, e)

        want = c["result"]
        if want is None:
            check()
            continue
        for fn in (check, lambda: pipe(promptA="a", promptB="a", control_image=img, controlnet_conditioning_scale=sc,
                                       control_guidance_start=st, control_guidance_end=en)):
            with pytest.raises(Exception) as ei:
                fn()
            assert type(ei.value).__name__ == want["type"] and str(ei.value) == want["message"], (c, ei.value)


def test_guidance_window_alignment():
    al = PP.StableDiffusionControlNetInpaintPipeline.align_control_guidance
    assert al(0.0, 1.0, 3) == ([0.0] * 3, [1.0] * 3)
    assert al(0.1, [0.5, 0.6], 3) == ([0.1, 0.1], [0.5, 0.6])           # (to the OTHER list's length, not to the nets')
    assert al([0.1, 0.2, 0.3, 0.4], 0.9, 2) == ([0.1, 0.2, 0.3, 0.4], [0.9] * 4)
    assert al([0.1], [0.5, 0.6], 2) == ([0.1], [0.5, 0.6])              # (two lists pass through; check_inputs refuses them)


def _ref_keep(n_steps, starts, ends):
    """pipeline_PowerPaint_ControlNet.py:1651-1658, restated."""
    controlnet_keep = []
    for i in range(n_steps):
        keeps = [1.0 - float(i / n_steps < s or (i + 1) / n_steps > e) for s, e in zip(starts, ends)]
        controlnet_keep.append(keeps)
    return controlnet_keep


SCHEDULES = [
    # (steps, scales, starts, ends, active sets per step or None)
    (4, [0.5, 0.8], [0.0, 0.25], [0.5, 0.75], [(0,), (0, 1), (1,), ()]),
    (4, [0.5, 0.8], [0.0, 0.0], [1.0, 1.0], [(0, 1)] * 4),
    (3, [1.0, 1.0, 1.0], [0.0, 0.34, 0.67], [0.33, 0.66, 1.0], None),
    (50, [0.5, 0.8], [0.0, 0.5], [0.5, 1.0], [(0,)] * 25 + [(1,)] * 25),
    (50, [0.7, 0.3, 1.2], [0.1, 0.0, 0.35], [0.9, 0.42, 1.0], None),
    (7, [0.5, 0.8], [0.2, 0.4], [0.6, 0.8], None),
    (1, [0.5, 0.8], [0.0, 0.5], [1.0, 1.0], [(0,)]),
    (10, [0.5, 0.0], [0.0, 0.0], [1.0, 1.0], [(0,)] * 10),              # a zero scale is a closed net at every step
    (5, [0.5], [0.0, 0.0], [1.0, 1.0], None),                           # (zip: the net without a scale never runs)
]


@pytest.mark.parametrize("n,scales,starts,ends,sets", SCHEDULES)
def test_scale_schedule_and_active_sets(n, scales, starts, ends, sets):
    rows = PP.StableDiffusionControlNetInpaintPipeline.control_schedule(n, scales, starts, ends)
    keep = _ref_keep(n, starts, ends)
    want = [[c * s for c, s in zip(scales, keep[i])] for i in range(n)]              # :1681
    assert rows == want
    active = [tuple(k for k, v in enumerate(r) if v != 0.0) for r in rows]
    assert active == [tuple(k for k, (c, kp) in enumerate(zip(scales, keep[i])) if c * kp != 0.0) for i in range(n)]
    if sets is not None:
        assert active == sets
    # the set changes at most 2 N times over a schedule
    assert sum(a != b for a, b in zip(active, active[1:])) <= 2 * len(starts)


def test_fixture_is_what_the_generator_describes():
    """Three frozen calls, far apart from each other: dropping a net, a scale or a window cannot pass the 0.9997 gate."""
    g = torch.load(os.path.join(HERE, "golden", "ref_pipeline_call_multicn.pt"), weights_only=False)
    one = torch.load(os.path.join(HERE, "golden", "ref_pipeline_call_cn.pt"), weights_only=False)["latents"]
    assert set(g) == {"plain", "windows", "guess"} and all(tuple(v.shape) == (1, 4, 16, 16) for v in g.values())
    cos = lambda a, b: torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0).item()   # noqa: E731
    assert cos(g["plain"], g["windows"]) < 0.995 and cos(g["plain"], g["guess"]) < 0.97
    assert tuple(one.shape) == tuple(g["plain"].shape)
