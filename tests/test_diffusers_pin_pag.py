"""Parity pin: the restated rules of perturbed-attention guidance (powerpaint_amd/pag.py, tests/pag_cases.py) against
diffusers' own `PAGMixin` (0.30 is the first release that has it).  Skipped where `diffusers.pipelines.pag` does not import --
README.md says "parity unpinned until this runs".  Three questions: does the layer resolver select the modules
`_set_pag_attn_processor` hands the identity processor to, is the scale rule `_get_pag_scale`, and is the combine
`_apply_perturbed_attention_guidance` (with the batch layout of `_prepare_perturbed_attention_guidance`)."""
import os
import sys

import pytest
import torch

pytest.importorskip("diffusers.pipelines.pag")
import diffusers  # noqa: E402
from diffusers.pipelines.pag.pag_utils import PAGMixin  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import pag_cases as PC  # noqa: E402
from powerpaint_amd import pag  # noqa: E402

TINY = dict(block_out_channels=(320, 640), layers_per_block=1, cross_attention_dim=768, attention_head_dim=8,
            down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"))


class _Pipe(PAGMixin):
    def __init__(self, unet, scale=3.0, adaptive=0.0):
        self.unet, self._pag_scale, self._pag_adaptive_scale = unet, scale, adaptive


def _self_attention_names(unet):
    from diffusers.models.attention_processor import Attention
    return [n for n, m in unet.named_modules() if isinstance(m, Attention) and not m.is_cross_attention]


@pytest.mark.parametrize("layers", ["mid", "down", ["down", "mid", "up"], "up_blocks.1.attentions.1", "0",
                                    r"blocks\.(0|1)\.attentions"])
def test_resolver_selects_what_set_pag_attn_processor_selects(layers):
    unet = diffusers.UNet2DConditionModel(in_channels=4, out_channels=4, **TINY)
    names = _self_attention_names(unet)
    before = dict(unet.attn_processors)
    pipe = _Pipe(unet)
    pipe.set_pag_applied_layers(layers)
    pipe._set_pag_attn_processor(pag_applied_layers=pipe.pag_applied_layers, do_classifier_free_guidance=True)
    changed = [n[:-len(".processor")] for n, p in unet.attn_processors.items() if p is not before[n]]
    assert sorted(changed) == sorted(pag.resolve_layers(layers, names)) == sorted(PC.resolve(layers, names))


def test_an_entry_that_selects_nothing_raises_there_too():
    unet = diffusers.UNet2DConditionModel(in_channels=4, out_channels=4, **TINY)
    pipe = _Pipe(unet)
    pipe.set_pag_applied_layers("nonexistent")
    with pytest.raises(ValueError, match="nonexistent"):
        pipe._set_pag_attn_processor(pag_applied_layers=pipe.pag_applied_layers, do_classifier_free_guidance=True)
    with pytest.raises(ValueError, match="nonexistent"):
        pag.resolve_layers("nonexistent", _self_attention_names(unet))


@pytest.mark.parametrize("adaptive", [0.0, 0.004, 0.01])
def test_scale_rule_is_get_pag_scale(adaptive):
    pipe = _Pipe(None, 3.0, adaptive)
    pipe.set_pag_applied_layers("mid")
    ts = [981.0, 741.0, 500.5, 261.0, 21.0]
    assert pag.scale_rows(3.0, adaptive, ts) == pytest.approx([float(pipe._get_pag_scale(t)) for t in ts], abs=1e-12)


@pytest.mark.parametrize("cfg", [True, False])
def test_combine_and_layout_are_the_mixins(cfg):
    pipe = _Pipe(None, 3.0, 0.0)
    pipe.set_pag_applied_layers("mid")
    g = torch.Generator().manual_seed(0)
    segs = 3 if cfg else 2
    eps = torch.randn(segs * 2, 4, 8, 8, generator=g, dtype=torch.float64)
    want = pipe._apply_perturbed_attention_guidance(eps, cfg, 7.5, 500)
    assert torch.allclose(pag.combine(eps, cfg, 7.5, 3.0), want, atol=1e-12, rtol=0)
    cond, uncond = torch.randn(2, 77, 8, generator=g), torch.randn(2, 77, 8, generator=g)
    want = pipe._prepare_perturbed_attention_guidance(cond, uncond, cfg)
    src = torch.cat([uncond, cond]) if cfg else cond
    assert torch.equal(pag.layout(src, 2, cfg), want)
