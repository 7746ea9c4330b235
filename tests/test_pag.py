"""CPU: perturbed-attention guidance off the device -- the layer resolver on the tiny net's module names, the per-row scale
rule, the combine, the batch layout, the refusals, the argument checks of the two entry points and the ABI version.
The float64 restatement is tests/pag_cases.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import pag_cases as PC  # noqa: E402
from oracle import sd_modules as OM  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import pag  # noqa: E402

TINY = dict(block_out_channels=(320, 640), layers_per_block=1,
            down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"))
PREFIXES = ["down_blocks.0.attentions.0", "mid_block.attentions.0", "up_blocks.1.attentions.0", "up_blocks.1.attentions.1"]


@pytest.fixture(scope="module")
def names():
    """The tiny net's self-attention modules as `named_modules()` spells them (registration order: down, up, mid)."""
    got = PC.attn1_names(OM.UNet2DConditionModel(in_channels=4, **TINY))
    assert sorted(got) == sorted(pag.attn1_names(PREFIXES))
    return got


def test_resolver_on_the_tiny_net(names):
    mid = "mid_block.attentions.0.transformer_blocks.0.attn1"
    down = "down_blocks.0.attentions.0.transformer_blocks.0.attn1"
    ups = ["up_blocks.1.attentions.0.transformer_blocks.0.attn1", "up_blocks.1.attentions.1.transformer_blocks.0.attn1"]
    assert pag.resolve_layers("mid", names) == [mid]
    assert pag.resolve_layers("down", names) == [down]
    assert sorted(pag.resolve_layers(["down", "mid", "up"], names)) == sorted(names)
    assert pag.resolve_layers("up_blocks.1.attentions.1", names) == [ups[1]]
    assert pag.resolve_layers(["mid", "mid_block"], names) == [mid]               # an overlap selects once
    assert sorted(pag.resolve_layers(r"blocks\.(0|1)\.attentions", names)) == sorted([down] + ups)    # entries are regular expressions
    for spec in ("mid", "down", ["down", "mid", "up"], "up_blocks.1.attentions.1", r"attentions\.0"):
        assert pag.resolve_layers(spec, names) == PC.resolve(spec, names)
    # the execution-order prefixes the engine keys its plans by
    assert pag.resolve_prefixes("mid", PREFIXES) == ("mid_block.attentions.0",)
    assert pag.resolve_prefixes(["up", "down"], PREFIXES) == (PREFIXES[0], PREFIXES[2], PREFIXES[3])


def test_an_entry_that_selects_nothing_is_named(names):
    with pytest.raises(ValueError, match="nonexistent"):
        pag.resolve_layers("nonexistent", names)
    with pytest.raises(ValueError, match="nonexistent"):
        pag.resolve_layers(["mid", "nonexistent"], names)
    with pytest.raises(ValueError, match="nonexistent"):
        pag.resolve_prefixes("nonexistent", PREFIXES)
    for bad in (None, 3, [], ["mid", 3]):
        with pytest.raises(ValueError, match="pag_applied_layers"):
            pag.resolve_layers(bad, names)


def test_fake_integral_match_is_discarded(names):
    """Entry "0" must not select `...transformer_blocks.0` through its trailing 0 alone: where the last dot-component of the
    entry and of the name are both numeric and equal, the match does not count.  (A self-attention module's own name ends in
    `attn1`, so over those the rule never fires: there "0" is an ordinary search.)"""
    block = "mid_block.attentions.0.transformer_blocks.0"
    with pytest.raises(ValueError, match="0"):
        pag.resolve_layers("0", [block])
    with pytest.raises(ValueError):
        pag.resolve_layers("transformer_blocks.0", [block])
    assert pag.resolve_layers("0", [block, block + ".attn1"]) == [block + ".attn1"]
    assert pag.resolve_layers("blocks.0", ["blocks.0", "blocks.0.attn1", "blocks.1.attn1"]) == ["blocks.0.attn1"]
    assert pag.resolve_layers("1", ["a.0", "a.1", "a.11"]) == ["a.11"]            # a.1 is the fake match; a.11 is a real one
    assert pag.resolve_layers("0", names) == PC.resolve("0", names) == names     # (every name holds a 0 and ends in attn1)
    for spec, pool in (("0", [block, block + ".attn1"]), ("1", ["a.0", "a.1", "a.11"])):
        assert pag.resolve_layers(spec, pool) == PC.resolve(spec, pool)


def test_scale_rule():
    ts = [981.0, 741.0, 500.5, 261.0, 21.0]
    assert pag.scale_rows(3.0, 0.0, ts) == [3.0] * 5                               # constant: unchanged across rows
    rows = pag.scale_rows(3.0, 0.01, ts)
    want = [float(PC.scale_f64(3.0, 0.01, t)) for t in ts]
    assert rows == want
    # exactly 0 where pag_scale < pag_adaptive_scale * (1000 - t): 1000 - t > 300
    assert [r == 0.0 for r in rows] == [False, False, True, True, True] and min(rows) == 0.0
    assert rows[0] == pytest.approx(3.0 - 0.19) and rows[1] == pytest.approx(3.0 - 2.59)
    # fractional timesteps (the midpoint rows of the two-stage samplers) and tensors are accepted
    assert pag.scale_rows(3.0, 0.004, torch.tensor([900.25, 250.75], dtype=torch.float64)) == \
        [float(PC.scale_f64(3.0, 0.004, 900.25)), float(PC.scale_f64(3.0, 0.004, 250.75))]
    assert pag.scale_rows(3.0, 0.004, [250.75])[0] == pytest.approx(3.0 - 0.004 * 749.25)
    with pytest.raises(ValueError):
        pag.scale_rows(-1.0, 0.0, ts)


def test_combine_and_layout():
    g = torch.Generator().manual_seed(0)
    for cfg in (True, False):
        segs = 3 if cfg else 2
        eps = torch.randn(segs * 2, 4, 3, 3, generator=g, dtype=torch.float64)
        got = pag.combine(eps, cfg, 7.5, 3.0)
        want = PC.combine_f64(eps.reshape(segs, -1).numpy(), cfg, 7.5, 3.0)
        assert np.allclose(got.reshape(-1).numpy(), want, rtol=0, atol=1e-12)
        assert pag.segments(cfg) == segs
    pair = torch.arange(4.0).reshape(4, 1)
    assert pag.layout(pair, 2, True).flatten().tolist() == [0, 1, 2, 3, 2, 3]       # [uncond, cond] -> [uncond, cond, cond]
    assert pag.layout(pair[:2], 2, True).flatten().tolist() == [0, 1, 0, 1, 0, 1]   # un-duplicated: every segment
    assert pag.layout(pair[:2], 2, False).flatten().tolist() == [0, 1, 0, 1]
    assert torch.equal(pag.layout(pair, 2, True), PC.layout(pair, 2, True))
    assert pag.layout(None, 2, True) is None
    with pytest.raises(L.PPError):
        pag.layout(torch.zeros(5, 1), 2, True)


def test_refusals_name_the_feature():
    with pytest.raises(L.PPError, match=r"token merging \(ToMe"):
        pag.check_supported(tome=True)
    with pytest.raises(L.PPError, match="guess_mode"):
        pag.check_supported(guess_mode=True)
    for kw in (dict(tome=True), dict(guess_mode=True)):
        with pytest.raises(L.PPError, match="perturbed-attention guidance"):
            pag.check_supported(**kw)
    pag.check_supported()


def test_the_loop_refuses_guess_mode_and_tome_before_anything_runs():
    """DenoiseLoop.bind raises by name before it touches a device."""
    from types import SimpleNamespace
    from powerpaint_amd.engine import ToMe
    from powerpaint_amd.pipelines._loop import DenoiseLoop
    from powerpaint_amd.schedulers import DDIMScheduler
    unet = SimpleNamespace(net=SimpleNamespace(tome=None), device="cpu")
    loop = DenoiseLoop(unet, DDIMScheduler())
    with pytest.raises(L.PPError, match="guess_mode"):
        loop.bind((1, 4, 8, 8), True, 7.5, None, guess_mode=True, pag_scale=3.0)
    unet.net.tome = ToMe(0.5, 1, 2, 2, True)
    with pytest.raises(L.PPError, match="ToMe"):
        loop.bind((1, 4, 8, 8), True, 7.5, None, pag_scale=3.0)


def test_bad_args_are_rejected_without_a_gpu():
    lib = L.lib()
    ok = (0x1000, 64, 1, 1, 64, 320, 0x2000, 320)
    assert lib.pp_attn_identity_v(None, *ok[1:], None) == -1
    assert lib.pp_attn_identity_v(*ok[:6], None, 320, None) == -1
    for i, bad in ((1, 60), (1, 68), (2, -1), (3, 0), (4, 0), (5, 324), (5, 0), (7, 312), (7, 324), (0, 0x1001), (6, 0x2001)):
        a = list(ok)
        a[i] = bad                      # ldvt < n, ldvt % 8, batch0 < 0, batch 0, n 0, C % 8, C 0, ldo < C, ldo % 8, odd pointers
        assert lib.pp_attn_identity_v(*a, None) == -1, (i, bad)
    okc = (0x1000, 1, 7.5, 0x2000, 0x3000, 16)
    for i, bad in ((0, None), (3, None), (4, None), (5, 0), (5, -4), (1, 2), (0, 0x1002)):
        a = list(okc)
        a[i] = bad
        assert lib.pp_pag_combine(*a, None) == -1, (i, bad)


def test_abi_version_is_unchanged():
    assert L.ABI_VERSION == 29 and L.lib().pp_abi_version() == 29
