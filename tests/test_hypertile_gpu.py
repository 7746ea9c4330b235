"""-m gpu: HyperTile through the engine -- a small UNet against the CPU oracle whose top-level attn1 is wrapped by the restatement
of tests/hypertile_cases.py, bitwise identity after removal, a tiled and an untiled block in one plan, and pipeline calls
through the fused loop (graph replay against eager replay; PAG + LoRA + strength < 1).

The networks are test_models_gpu.make_tiny's (top level: C = 320, 8 heads, head dim 40) with the top-level self-attentions made
to MATTER: to_q, to_k and to_v times SHARP = 2 (scores times 4: a more peaked softmax instead of a near-uniform average over
random keys), on both sides.  With make_tiny's own weights every query averages its keys almost uniformly, the mean over a tile
is close to the mean over the grid, and no gate could tell the patched from the unpatched network.  The gate is the one of the
small-network tests (test_models_gpu.close: cosine >= 0.999, max-abs <= 3e-2 max(1, max|ref|)); the unpatched network must FAIL
it against the tiled oracle.  Measured at 16 x 64 (MI355X): patched against the tiled oracle cosine 0.999963 / max-abs 0.012,
unpatched against the tiled oracle cosine 0.99793 / max-abs 0.082 (bound 0.042).  (A factor of 4 makes the softmax so peaked
that the 16-bit network itself leaves the gate: cosine 0.99901, max-abs 0.060 against the tiled oracle.)
"""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import hypertile_cases as HC  # noqa: E402
from lora_cases import make_factors  # noqa: E402
from oracle import sd_modules as OM  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import hypertile  # noqa: E402
from powerpaint_amd import pipelines as PP  # noqa: E402
from powerpaint_amd import schedulers as PS  # noqa: E402
from powerpaint_amd.lora import unet_targets  # noqa: E402
from test_models_gpu import DEV, close, gen, make_tiny  # noqa: E402

TOP = ["down_blocks.0.attentions.0", "up_blocks.1.attentions.0", "up_blocks.1.attentions.1"]
H16, W64 = 16, 64            # tile_size 256 -> 1 x 2 tiles of 16 x 32 = 512 tokens
SHARP = 2.0                  # factor on the top-level attn1 to_q / to_k / to_v weights (module docstring)


def sharpened(kind="unet", seed=0, **extra):
    """make_tiny with peaked top-level self-attentions (module docstring); the same weights on both sides."""
    o, h = make_tiny(kind, seed=seed, **extra)
    with torch.no_grad():
        for n, p in o.named_parameters():
            if ".attn1.to_" in n and n.endswith(".weight") and "to_out" not in n and p.shape[0] == 320:
                p.copy_((p * SHARP).to(torch.bfloat16).float())
    sd = {k: v.detach().clone() for k, v in o.state_dict().items()}
    h.load_state_dict(sd, keep_state_dict=True)
    return o, h, sd


@functools.lru_cache(maxsize=None)
def _unet4():
    return sharpened("unet", in_channels=4)


class OracleHyperTile:
    """Wraps OM.BasicTransformerBlock.forward: x = x + from_tiles(attn1(to_tiles(norm1(x)))) where the tokens are the latent
    grid itself (h * w of them); every other block runs as it is."""

    def __init__(self, h, w, tile_size=256):
        self.h, self.w = h, w
        self.nh, self.nw = HC.layout(h, w, tile_size)
        self.tiled = 0

    def __enter__(self):
        self.orig, this = OM.BasicTransformerBlock.forward, self

        def fwd(blk, x, ctx):
            if x.shape[1] != this.h * this.w or this.nh * this.nw == 1:
                return this.orig(blk, x, ctx)
            this.tiled += 1
            a = blk.attn1(HC.to_tiles(blk.norm1(x), this.h, this.w, this.nh, this.nw))
            x = x + HC.from_tiles(a, x.shape[0], this.h, this.w, this.nh, this.nw)
            x = x + blk.attn2(blk.norm2(x), ctx)
            return x + blk.ff(blk.norm3(x))

        OM.BasicTransformerBlock.forward = fwd
        return self

    def __exit__(self, *exc):
        OM.BasicTransformerBlock.forward = self.orig


@functools.lru_cache(maxsize=None)
def _references(h, w):
    """-> (x, e, the oracle's plain output, its output with the tiled top level): computed once, never modified."""
    o, _, _ = _unet4()
    x, e = gen(2, 4, h, w, seed=1), gen(2, 77, 768, seed=2)
    with torch.no_grad():
        plain = o(x, 500, e)[0]
        with OracleHyperTile(h, w) as orc:
            tiled = o(x, 500, e)[0]
    return x, e, plain, tiled, orc.tiled


def _tiled_calls(rt):
    return [c for c in rt.step_plan.calls if c[0] is L.lib().pp_attention_fwd_tiled]


def test_small_network_against_the_oracle():
    _, hnet, _ = _unet4()
    x, e, plain, tiled, n_tiled = _references(H16, W64)
    assert n_tiled == 3
    xd, ed = x.to(DEV), e.to(DEV)
    hypertile.apply_patch(hnet)
    try:
        lay = hnet.net.hypertile_layout(H16, W64)
        assert all(lay[p] == (1, 2, True, "tiled") for p in TOP) and [p for p, v in lay.items() if v[2]] == TOP
        out = hnet(xd, 500, ed, return_dict=False)[0].clone()
        assert len(_tiled_calls(hnet.rt)) == 3
    finally:
        hypertile.remove_patch(hnet)
    unpatched = hnet(xd, 500, ed, return_dict=False)[0].clone()
    assert not _tiled_calls(hnet.rt)

    def fig(a, b):
        a, b = a.float().cpu(), b.float().cpu()
        return (f"cosine {torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0).item():.6f}, "
                f"max-abs {float((a - b).abs().max()):.4f}")

    print(f"[hypertile] {H16}x{W64}, max|ref| {float(tiled.abs().max()):.3f}: oracle tiled against plain {fig(tiled, plain)}; "
          f"patched against tiled {fig(out, tiled)}; unpatched against plain {fig(unpatched, plain)}; "
          f"unpatched against tiled {fig(unpatched, tiled)}")
    close(out, tiled, f"hypertile unet tiny {H16}x{W64}, 1x2 tiles")
    close(unpatched, plain, f"hypertile unet tiny {H16}x{W64}, unpatched against the plain oracle")
    with pytest.raises(AssertionError):                      # the patch has an observable effect at this gate
        close(unpatched, tiled, f"hypertile unet tiny {H16}x{W64}, UNPATCHED against the tiled oracle (must fail)")
    with pytest.raises(AssertionError):
        close(out, plain, f"hypertile unet tiny {H16}x{W64}, PATCHED against the plain oracle (must fail)")


def test_removed_is_bitwise_the_never_patched_network():
    _, hnet, _ = _unet4()
    x, e = gen(2, 4, H16, W64, seed=1).to(DEV), gen(2, 77, 768, seed=2).to(DEV)
    want = hnet(x, 500, e, return_dict=False)[0].clone()
    hypertile.apply_patch(hnet)
    got = hnet(x, 500, e, return_dict=False)[0].clone()
    assert not torch.equal(got, want) and bool(torch.isfinite(got).all())
    hypertile.apply_patch(hnet, tile_size=2048)              # one tile everywhere: the unpatched launches under another key
    assert torch.equal(hnet(x, 500, e, return_dict=False)[0], want)
    hypertile.remove_patch(hnet)
    assert torch.equal(hnet(x, 500, e, return_dict=False)[0], want)


def test_a_tiled_and_an_untiled_block_in_one_plan():
    """8 x 64: the top level tiles (1 x 2 tiles of 8 x 32 = 256 keys, the kernel's minimum), the mid block on the 4 x 32 grid does
    not (depth 1); 16 x 40: side(40) = 40 and side(16) = 16, nothing is split; both decisions are in hypertile_layout, and the
    network with one tiled and one untiled kind of block agrees with the oracle."""
    o, hnet, _ = _unet4()
    hypertile.apply_patch(hnet)
    try:
        lay = hnet.net.hypertile_layout(8, 64)
        assert all(lay[p] == (1, 2, True, "tiled") for p in TOP)
        assert lay["mid_block.attentions.0"][:3] == (1, 1, False) and "depth 1" in lay["mid_block.attentions.0"][3]
        x, e = gen(2, 4, 8, 64, seed=3), gen(2, 77, 768, seed=2)
        out = hnet(x.to(DEV), 500, e.to(DEV), return_dict=False)[0].clone()
        names = [c[2] for c in hnet.rt.step_plan.calls]
        assert len(_tiled_calls(hnet.rt)) == 3 and names.count("attention") > 3
        with torch.no_grad(), OracleHyperTile(8, 64) as orc:
            ref = o(x, 500, e)[0]
        assert orc.tiled == 3
        close(out, ref, "hypertile unet tiny 8x64: tiled top level, untiled mid block")
        lay = hnet.net.hypertile_layout(16, 40)
        assert all(v[:3] == (1, 1, False) for v in lay.values()) and "one tile" in lay[TOP[0]][3]
        x2 = gen(2, 4, 16, 40, seed=4)
        out2 = hnet(x2.to(DEV), 500, e.to(DEV), return_dict=False)[0].clone()
        assert not _tiled_calls(hnet.rt)
    finally:
        hypertile.remove_patch(hnet)
    assert torch.equal(hnet(x2.to(DEV), 500, e.to(DEV), return_dict=False)[0], out2)


def test_pipeline_graph_against_eager_and_with_pag_lora_strength():
    """One ControlNet inpainting pipeline (UNet + ControlNet, both patched), 3 DDIM steps on a 16 x 64 latent."""
    _, hc = make_tiny("controlnet")
    _, hu, sd = sharpened("unet", seed=1, in_channels=9)
    B, N = 1, 3
    lat, mask, mil = gen(B, 4, H16, W64, seed=0), torch.zeros(B, 1, H16, W64), gen(B, 4, H16, W64, seed=1, scale=0.5)
    mask[:, :, 4:12, 8:40] = 1.0
    pe = gen(2 * B, 77, 768, seed=2)
    img = torch.rand(B, 3, 8 * H16, 8 * W64, generator=torch.Generator().manual_seed(3))
    pipe = PP.StableDiffusionControlNetInpaintPipeline(unet=hu, controlnet=hc, scheduler=PS.DDIMScheduler(),
                                                       pag_applied_layers="mid")
    kw = dict(prompt_embeds=pe[B:].to(DEV), negative_prompt_embeds=pe[:B].to(DEV), height=8 * H16, width=8 * W64,
              control_image=img.to(DEV), num_inference_steps=N, guidance_scale=7.5, latents=lat.to(DEV),
              mask_latents=mask.to(DEV), masked_image_latents=mil.to(DEV), output_type="latent", return_dict=False)
    never = pipe(**kw)[0].clone()
    hypertile.apply_patch(pipe)
    try:
        assert hu.net.hypertile is not None and hc.net.hypertile is not None
        assert pipe.use_graph
        out = pipe(**kw)[0].clone()
        assert len(_tiled_calls(hu.rt)) == 3 and len(_tiled_calls(hc.rt)) == 1
        pipe.use_graph = False
        eager = pipe(**kw)[0].clone()
        pipe.use_graph = True
        assert torch.equal(out, eager), "graph replay and eager replay differ"
        assert bool(torch.isfinite(out).all()) and not torch.equal(out, never)

        # PAG on the mid block + a LoRA + strength 0.6 (the schedule is entered late): finite, the same bits twice
        hu.load_lora_adapter(make_factors(unet_targets(hu.net), sd, 4, seed=51), "ht")
        try:
            more = dict(kw, pag_scale=3.0, strength=0.6, num_inference_steps=5)
            a = pipe(**more)[0].clone()
            b = pipe(**more)[0].clone()
            assert len(_tiled_calls(hu.rt)) == 3 and hu.rt.B == 3 * B
            assert "attn_identity_v" in [c[2] for c in hu.rt.step_plan.calls]
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and not torch.equal(a, out)
            # ... and with PAG on a TILED block: the tiled launch runs on the leading items
            pipe.set_pag_applied_layers(["down", "mid"])
            c = pipe(**more)[0].clone()
            d = pipe(**more)[0].clone()
            calls = hu.rt.step_plan.calls
            first = next(i for i, cl in enumerate(calls) if cl[2] == "attn_identity_v")
            assert calls[first - 1][0] is L.lib().pp_attention_fwd_tiled and list(calls[first - 1][1])[8] == 2 * B
            assert bool(torch.isfinite(c).all()) and torch.equal(c, d) and not torch.equal(c, a)
        finally:
            hu.delete_adapters(hu.list_adapters())
            pipe.set_pag_applied_layers("mid")
    finally:
        hypertile.remove_patch(pipe)
    assert torch.equal(pipe(**kw)[0], never)
