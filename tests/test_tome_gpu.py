"""-m gpu: token merging through the engine -- a small UNet against the CPU oracle with `BasicTransformerBlock.forward` wrapped
by the restatement of tests/tome_cases.py, and one BrushNet-pipeline call through the fused loop and graph replay.

Decisions.  The oracle computes its own decisions and their margins from ITS hidden state (fp32 arithmetic on bf16-rounded
weights); the GPU's are read back through NetRuntime.tome_decisions().  Per source token two decisions are compared:
  * its best destination; margin = best minus second-best cosine;
  * whether it is merged; margin = 2 |score - b| with b the midpoint of the r-th and (r+1)-th highest score (for the two
    sources at the boundary that is the r-th minus (r+1)-th gap).
Wherever the oracle's margin is >= TAU the GPU's decision must equal the oracle's.  Below TAU the decision is ambiguous (the two
hidden states differ by the 16-bit rounding of every activation in front of the block): at most 10 % of a block's decisions
may be, and the oracle is then run again WITH the GPU's decisions and must agree with the GPU's output at the tolerance
tests/test_models_gpu.py uses for the unpatched network (cosine >= 0.999, max-abs <= 3e-2 max(1, max|ref|)).

TAU is a measurement (profiles/tome_parity_achieved.txt): the largest oracle margin at which any GPU decision differed from
the oracle's in the measuring run, 1.379e-3, times four.  The latents were then chosen on the CPU so that the oracle alone
stays under the 10 % cap; on THOSE the largest margin of a differing decision is 3.681e-3 (6x10, fixed windows, duplicated
halves) -- under TAU by a factor 1.5, not 4.  Four times that figure and the 10 % cap do not fit together on this network
(the file has the search): the bf16 rounding of the activations in front of a block moves cosines by a few 1e-3, the size of
the margins themselves.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import tome_cases as TC  # noqa: E402
from oracle import sd_modules as OM  # noqa: E402
from powerpaint_amd import pipelines as PP  # noqa: E402
from powerpaint_amd import schedulers as PS  # noqa: E402
from powerpaint_amd import tome  # noqa: E402
from test_models_gpu import DEV, close, gen, make_tiny  # noqa: E402

TAU = 4 * 1.379e-3         # four times the largest margin of a differing decision (profiles/tome_parity_achieved.txt)
TOP = ["down_blocks.0.attentions.0", "up_blocks.1.attentions.0", "up_blocks.1.attentions.1"]


def smooth_latents(B, C, h, w, seed, twin=False):
    """Spatially smooth latents (low frequencies + a little noise): neighbouring tokens are similar, as in a real image."""
    x = TC.smooth_tokens(1 if twin else B, h, w, C, seed, noise=0.3).reshape(-1, h, w, C).permute(0, 3, 1, 2).float()
    return x.repeat(B, 1, 1, 1).contiguous() if twin else x.contiguous()


class OracleToMe:
    """Wraps OM.BasicTransformerBlock.forward: x = unmerge(attn1(merge(norm1(x)))) + x at the top level (tokens == h*w)."""

    def __init__(self, h, w, ratio, wins, gpu=None):
        self.h, self.w, self.wins, self.gpu = h, w, wins, gpu
        nd = TC.window_count(h, w, 2, 2)
        self.r = TC.merged_count(h * w, ratio, nd)
        self.nkept = h * w - nd - self.r
        self.decisions = []

    def __enter__(self):
        self.orig, this, self.k = OM.BasicTransformerBlock.forward, self, 0

        def fwd(blk, x, ctx):
            if x.shape[1] != this.h * this.w or not this.r:
                return this.orig(blk, x, ctx)
            i = this.k
            this.k += 1
            decs = []
            for b in range(x.shape[0]):
                kw = {}
                if this.gpu is not None:
                    best, _, pos = this.gpu[i]
                    gb = b % best.shape[0]                      # (twin prefix: the block ran on one CFG half)
                    kw = dict(best_override=best[gb], merged_override=(best[gb] >= 0) & (pos[gb] >= this.nkept))
                decs.append(TC.decide(x[b], this.h, this.w, 2, 2, this.wins[i], this.r, **kw))
            this.decisions.append(decs)
            n1 = blk.norm1(x)
            m = torch.stack([TC.merge_rows(n1[b], d) for b, d in enumerate(decs)]).to(x.dtype)
            a = blk.attn1(m)
            x = x + torch.stack([a[b][d["pos"]] for b, d in enumerate(decs)])
            x = x + blk.attn2(blk.norm2(x), ctx)
            return x + blk.ff(blk.norm3(x))

        OM.BasicTransformerBlock.forward = fwd
        return self

    def __exit__(self, *exc):
        OM.BasicTransformerBlock.forward = self.orig


def compare_decisions(dec, gpu, nkept, r):
    """One block, one batch item.  -> (differing decisions as [(margin, kind)], ambiguous count at TAU, decisions)."""
    best, score, pos = gpu
    src = dec["src"]
    g_best = best.to(torch.int64)[src]
    g_merged = (pos.to(torch.int64)[src] >= nkept)
    s = dec["score"][src]
    if 0 < r < src.numel():
        top = torch.sort(s, descending=True).values
        sel_margin = 2 * (s - (top[r - 1] + top[r]) / 2).abs()
    else:
        sel_margin = torch.full_like(s, float("inf"))
    bm = dec["best_margin"][src]
    diffs = [(float(m), "best") for m in bm[g_best != dec["best"][src]]]
    diffs += [(float(m), "merged") for m in sel_margin[g_merged != dec["merged"][src]]]
    amb = int((bm < TAU).sum()) + int((sel_margin < TAU).sum())
    return diffs, amb, 2 * src.numel()


def run_case(h, w, use_rand, twin, seed=2, ratio=0.5):
    """-> dict(out, ref, ref_gpu_decisions, diffs, worst ambiguous share, draws ok)."""
    o, hnet = make_tiny("unet", in_channels=4)
    B = 2
    x, e = smooth_latents(B, 4, h, w, seed, twin=twin), gen(B, 77, 768, seed=2)
    tome.apply_patch(hnet, ratio=ratio, use_rand=use_rand, generator=torch.Generator().manual_seed(77))
    rt = hnet.prepare((B, 4, h, w), e.to(DEV), twin=twin)
    rt.load_input([(x.to(DEV), 0)])
    rt.set_timestep(500)
    rt.run_step()
    out = rt.eps_tensor().float().cpu()
    blocks = rt.tome_blocks()
    assert list(blocks) == TOP
    table = rt.tome_table().cpu()
    assert table.shape[0] == 1
    wins = [table[0, b.offset:b.offset + b.nd] for b in blocks.values()]
    # the windows are the generator's draws, in execution order (none with use_rand off)
    ref_draws = TC.Draws(torch.Generator().manual_seed(77), use_rand)
    assert all(torch.equal(w_, ref_draws.draw(h, w, 2, 2, B)) for w_ in wins)
    assert bool(torch.stack(wins).any()) == use_rand
    gpu = [tuple(t.cpu() for t in rt.tome_decisions()[pre]) for pre in blocks]
    assert gpu[0][0].shape[0] in (1, B)               # (1: the twin prefix ran this block on one CFG half)
    with torch.no_grad():
        with OracleToMe(h, w, ratio, wins) as orc:
            ref = o(x, 500, e)[0]
        with OracleToMe(h, w, ratio, wins, gpu=gpu) as orc2:
            ref_gpu = o(x, 500, e)[0]
    assert len(orc.decisions) == len(orc2.decisions) == 3
    diffs, worst_share = [], 0.0
    for i, decs in enumerate(orc.decisions):
        amb = tot = 0
        for b, d in enumerate(decs):
            g = tuple(t[b % gpu[i][0].shape[0]] for t in gpu[i])
            df, a, n = compare_decisions(d, g, orc.nkept, orc.r)
            diffs += [(m, k, i, b) for m, k in df]
            amb, tot = amb + a, tot + n
        worst_share = max(worst_share, amb / tot)
    tome.remove_patch(hnet)
    return dict(out=out, ref=ref, ref_gpu=ref_gpu, diffs=diffs, share=worst_share)


@pytest.mark.parametrize("twin", [False, True])
@pytest.mark.parametrize("use_rand", [True, False])
@pytest.mark.parametrize("h,w", [(8, 8), (6, 10)])
def test_small_network_against_the_oracle(h, w, use_rand, twin):
    res = run_case(h, w, use_rand, twin)
    worst = max([m for m, *_ in res["diffs"]], default=0.0)
    print(f"[tome parity] {h}x{w} use_rand={use_rand} twin={twin}: {len(res['diffs'])} differing decisions, largest margin "
          f"{worst:.3e} (TAU {TAU:.3e}); ambiguous share {res['share']:.3f}")
    assert res["share"] <= 0.10, "more than 10 % of a block's decisions are ambiguous at TAU: choose other inputs"
    assert all(m < TAU for m, *_ in res["diffs"]), ("a decision differs where the oracle's margin is >= TAU", res["diffs"][:5])
    close(res["out"], res["ref_gpu"], f"tome unet tiny {h}x{w} rand={use_rand} twin={twin} (GPU decisions)")
    if not res["diffs"]:
        close(res["out"], res["ref"], f"tome unet tiny {h}x{w} rand={use_rand} twin={twin}")


def test_ratio_zero_is_bitwise_the_unpatched_network():
    _, hnet = make_tiny("unet", in_channels=4)
    x, e = gen(2, 4, 8, 8, seed=1).to(DEV), gen(2, 77, 768, seed=2).to(DEV)
    want = hnet(x, 500, e, return_dict=False)[0].clone()
    tome.apply_patch(hnet, ratio=0.0)
    assert torch.equal(hnet(x, 500, e, return_dict=False)[0], want)
    tome.apply_patch(hnet, ratio=0.5)
    got = hnet(x, 500, e, return_dict=False)[0].clone()
    assert not torch.equal(got, want) and bool(torch.isfinite(got).all())
    tome.remove_patch(hnet)
    assert torch.equal(hnet(x, 500, e, return_dict=False)[0], want)


def test_pipeline_replays_with_fresh_windows_every_step():
    """One BrushNet-pipeline call of 3 DDIM steps at 64 x 64 pixels through the fused loop and graph replay."""
    _, hb = make_tiny("brushnet")
    _, hu = make_tiny("unet", seed=1, in_channels=4)
    B, hh, N = 1, 8, 3
    lat = gen(B, 4, hh, hh, seed=0)
    mask = torch.zeros(B, 1, hh, hh)
    mask[:, :, 2:6, 2:6] = 1.0
    cl = torch.cat([gen(B, 4, hh, hh, seed=1, scale=0.5), mask], 1)
    pe, peU = gen(2 * B, 77, 768, seed=2), gen(2 * B, 77, 768, seed=3)
    pipe = PP.StableDiffusionPowerPaintBrushNetPipeline(unet=hu, brushnet=hb, scheduler=PS.DDIMScheduler())
    kw = dict(prompt_embeds=pe[B:].to(DEV), negative_prompt_embeds=pe[:B].to(DEV), prompt_embedsU=peU[B:].to(DEV),
              negative_prompt_embedsU=peU[:B].to(DEV), conditioning_latents=cl.to(DEV), num_inference_steps=N,
              guidance_scale=7.5, latents=lat.to(DEV), output_type="latent", return_dict=False)
    never = pipe(**kw)[0].clone()

    def patched():
        tome.apply_patch(pipe, generator=torch.Generator().manual_seed(5))
        seen = []
        out = pipe(callback=lambda i, t, l: seen.append(hu.rt.tome_decisions()[TOP[0]][0][0].cpu()), **kw)[0].clone()
        return out, seen, hu.rt.tome_table().cpu()

    assert pipe.use_graph
    out1, seen, table = patched()
    assert "tome_match" in [c[2] for c in hu.rt.step_plan.calls] and table.shape[0] == N and len(seen) == N
    blk = hu.rt.tome_blocks()[TOP[0]]
    for i, best in enumerate(seen):                   # step i matched around the destinations of table row i
        _, dst = TC.partition(hh, hh, 2, 2, table[i, blk.offset:blk.offset + blk.nd])
        assert (best < 0).nonzero().flatten().tolist() == dst.tolist(), f"step {i} did not use table row {i}"
    assert len({tuple(table[i].tolist()) for i in range(N)}) == N, "the replayed steps must draw different windows"
    assert bool(torch.isfinite(out1).all()) and not torch.equal(out1, never)
    out2, _, table2 = patched()                       # the same seed: the same windows, the same bits
    assert torch.equal(table, table2) and torch.equal(out1, out2)
    tome.remove_patch(pipe)
    assert torch.equal(pipe(**kw)[0], never)
