"""-m gpu: IP-Adapter masks on the HIP path -- pp_ip_attn_add_masked alone against a float64 evaluation of its formula and
against pp_ip_attn_add bit for bit, the UNet against the oracle UNet with the restated masked processor
(tests/ip_mask_cases.py), and the BrushNet pipeline against the reference's own `__call__` (tests/golden/ref_ip_adapter_masks.pt).
The kernel's gate is derived in tests/ip_mask_cases.py's docstring; the network and loop gates are the project's
(ip_adapter_cases.net_gate / loop_gate).  Achieved numbers are printed and appended to
profiles/ip_adapter_masks_parity_achieved.txt before anything is asserted."""
import functools
import os
import sys
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import ip_adapter_cases as IC  # noqa: E402
import ip_mask_cases as MC  # noqa: E402
from oracle import sd_modules as OM  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import models as PM  # noqa: E402
from powerpaint_amd import pipelines as PP  # noqa: E402
from powerpaint_amd import schedulers as PS  # noqa: E402

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
GUARD = 3            # sentinel rows behind the last row of o


def record(line: str):
    print(line)
    try:
        with open(os.path.join(ROOT, "profiles", "ip_adapter_masks_parity_achieved.txt"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run_kernel(q, k, v, o, batch, heads, d, nq, nk, qk_scale, ip_scale, dtype, w=None):
    """o: [batch * nq][ldo] host tensor -> the device result [batch * nq + GUARD][ldo] (guard rows and row gaps hold a
    sentinel), the device copy of q after the launch, the sentinel.  w: fp32 [nq] -> the masked entry; None -> pp_ip_attn_add."""
    C = heads * d
    ldq, ldo = q.shape[1], o.shape[1]
    sent = torch.tensor(-1234.0).to(dtype)
    od = torch.full((batch * nq + GUARD, ldo), float(sent), dtype=dtype)
    od[:batch * nq, :C] = o[:, :C]
    od = od.to(DEV)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    if w is None:
        L.check(L.lib().pp_ip_attn_add(qd.data_ptr(), ldq, kd.data_ptr(), vd.data_ptr(), od.data_ptr(), ldo, batch, heads, nq,
                                       nk, d, qk_scale, ip_scale, L.dtype_code(dtype), _stream()), "pp_ip_attn_add")
    else:
        wd = w.to(device=DEV, dtype=torch.float32).contiguous()
        assert wd.numel() == nq
        L.check(L.lib().pp_ip_attn_add_masked(qd.data_ptr(), ldq, kd.data_ptr(), vd.data_ptr(), od.data_ptr(), ldo, batch, heads,
                                              nq, nk, d, qk_scale, ip_scale, wd.data_ptr(), L.dtype_code(dtype), _stream()),
                "pp_ip_attn_add_masked")
    torch.cuda.synchronize()
    return od.cpu(), qd.cpu(), sent


def _bits(t):
    return t.contiguous().view(torch.int16)


def _check(out, sent, q_after, q, k, v, o, batch, heads, d, nq, nk, qk_scale, ip_scale, w, dtype, what):
    C, M = heads * d, batch * nq
    assert torch.equal(q_after, q), f"{what}: q was modified"
    assert bool((out[M:] == sent).all()), f"{what}: rows behind the last row were written"
    if out.shape[1] > C:
        assert bool((out[:M, C:] == sent).all()), f"{what}: the gaps between rows were written"
    dead = (w == 0).repeat(batch)
    assert torch.equal(_bits(out[:M, :C][dead]), _bits(o[:, :C][dead])), f"{what}: a row of weight 0 changed"
    ref, mag, smax = MC.kernel_ref(q, k, v, o, batch, heads, d, nq, nk, qk_scale, ip_scale, w)
    got = out[:M, :C].double()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    tol = MC.kernel_gate(ref, mag, smax, d, nk, dtype)
    return float(((got - ref).abs() / tol).max())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("heads,d", IC.KERNEL_HEADS_D)
def test_pp_ip_attn_add_masked_against_float64(heads, d, dtype):
    """The grid of tests/test_ip_adapter_gpu.py -- nq 1 / 64 / 100 (partial row groups), nk 1 / 4 (registers) and 8 / 16
    (streamed), batch 2 with different K / V per item, dense and gapped strides -- under MC.kernel_weights: 1.0, fractions, the
    bicubic overshoots -0.09375 and 1.09375, and zero runs of 7, 30, 5 and 13 rows.  At one head of 40 channels a wave takes 12
    rows at a time: zero and live rows share a group, and rows [24, 48) are two whole groups that are skipped; at the other
    shapes (one row per group) every zero row is a skipped group and [17, 47) holds whole skipped passes."""
    C, batch = heads * d, 2
    worst = {}
    for nq in IC.KERNEL_NQ:
        w = MC.kernel_weights(nq)
        for nk in IC.KERNEL_NK:
            for ldq, ldo in ((C, C), (2 * C, C + 8)):
                q, k, v, o = IC.kernel_inputs(batch, heads, d, nq, nk, dtype, ldq, ldo, seed=nq * 100 + nk)
                qk, sc = d ** -0.5, 0.7
                out, q_after, sent = _run_kernel(q, k, v, o, batch, heads, d, nq, nk, qk, sc, dtype, w)
                worst[(nq, nk, ldo)] = _check(out, sent, q_after, q, k, v, o, batch, heads, d, nq, nk, qk, sc, w, dtype,
                                              f"heads {heads} d {d} nq {nq} nk {nk} ldq {ldq} ldo {ldo}")
    top = max(worst, key=worst.get)
    record(f"[ip_adapter_masks] kernel heads {heads} d {d} {str(dtype)[6:]}: worst err / bound over {len(worst)} shapes "
           f"{worst[top]:.3g} at (nq, nk, ldo) = {top}")
    assert worst[top] <= 1.0, (top, worst[top])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("nk", [4, 16])
@pytest.mark.parametrize("heads,d", [(8, 40), (1, 40), (8, 160)])
def test_all_ones_weights_are_pp_ip_attn_add_bit_for_bit(heads, d, nk, dtype):
    batch, nq, C = 2, 100, heads * d
    q, k, v, o = IC.kernel_inputs(batch, heads, d, nq, nk, dtype, 2 * C, C + 8, seed=3)
    want, _, _ = _run_kernel(q, k, v, o, batch, heads, d, nq, nk, d ** -0.5, 0.7, dtype)
    got, q_after, _ = _run_kernel(q, k, v, o, batch, heads, d, nq, nk, d ** -0.5, 0.7, dtype, torch.ones(nq))
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(q_after, q)
    assert not torch.equal(_bits(got[:batch * nq, :C]), _bits(o[:, :C]))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("nk", [4, 16])
@pytest.mark.parametrize("heads,d", [(8, 40), (1, 40)])
def test_zero_weights_keep_the_bits_of_o(heads, d, nk, dtype):
    """All-zero weights: nothing changes.  Zero rows among live ones: their bits stay -- signed zeros and values far below one
    unit of the term (adding a rounded 0 * term would turn -0.0 into +0.0) -- while the live rows do change."""
    batch, nq, C = 2, 100, heads * d
    q, k, v, o = IC.kernel_inputs(batch, heads, d, nq, nk, dtype, seed=5)
    plant = torch.tensor([0.0, -0.0, 1.0, -1.0, 6e-8, -6e-8, 3.0, -3.0]).to(dtype)
    w = MC.kernel_weights(nq)
    for r in (3, 9, 24, 46, 57, 82):                          # rows of weight 0: first / last of a run, inside a skipped group
        assert w[r] == 0
        o[r, :8] = plant
        o[nq + r, C - 8:] = plant
    out, q_after, _ = _run_kernel(q, k, v, o, batch, heads, d, nq, nk, d ** -0.5, 1.0, dtype, torch.zeros(nq))
    assert torch.equal(_bits(out[:batch * nq]), _bits(o)) and torch.equal(q_after, q)
    out, q_after, _ = _run_kernel(q, k, v, o, batch, heads, d, nq, nk, d ** -0.5, 1.0, dtype, w)
    dead = (w == 0).repeat(batch)
    assert torch.equal(_bits(out[:batch * nq][dead]), _bits(o[dead])) and torch.equal(q_after, q)
    changed = (_bits(out[:batch * nq]) != _bits(o)).any(dim=1)
    assert torch.equal(changed, ~dead)
    # ip_scale = 0: no launch, no change, whatever the weights
    out, q_after, _ = _run_kernel(q, k, v, o, batch, heads, d, nq, nk, d ** -0.5, 0.0, dtype, w)
    assert torch.equal(_bits(out[:batch * nq]), _bits(o)) and torch.equal(q_after, q)


# ------------------------------------------------------------------------------------------------------------ network
TINY = dict(block_out_channels=(320, 640), layers_per_block=1,
            down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"))
# name -> (latent h, w; mask H, W): the latents' own aspect, an odd second level (9x6), an off-aspect mask (padded weights)
NET_SHAPES = {"16x16": ((16, 16), (128, 128)), "18x12": ((18, 12), (144, 96)), "16x16-mask128x64": ((16, 16), (128, 64))}


def _net_masks(n_adapters, mask_hw):
    H, W = mask_hw
    if n_adapters == 1:
        return MC.rect_mask(H, W, H // 8 + 3, W // 8, H // 2 + 5, 5 * W // 8 + 3).unsqueeze(0)
    left = MC.rect_mask(H, W, 0, 0, H, W // 2 + 3)
    return torch.stack([left, 1.0 - left])


@functools.lru_cache(maxsize=None)
def _oracle_case(n_adapters, shape):
    """(oracle state dict, adapter state dicts, inputs, the masked reference) -- computed once, shared by the dtypes."""
    hw, mask_hw = NET_SHAPES[shape]
    scales = [1.0] if n_adapters == 1 else [0.7, 0.4]
    torch.manual_seed(1234)
    o = OM.UNet2DConditionModel(in_channels=4, **TINY).eval()
    with torch.no_grad():
        for p in o.parameters():
            if p.dim() >= 2:
                p.copy_(p.to(torch.bfloat16).float())
    sd = {k: v.clone() for k, v in o.state_dict().items()}
    sds = [IC.adapter_state_dict(o, 50 + i, std=1.0) for i in range(n_adapters)]
    ipu = MC.MaskedIPUNet(o, sds, scales).eval()
    g = torch.Generator().manual_seed(hw[0] * 10 + n_adapters)
    B = 2
    x = torch.randn(B, 4, *hw, generator=g)
    ehs = torch.randn(B, 77, 768, generator=g)
    embeds = [torch.randn(B, 1 + i, IC.EMBED_DIM, generator=g) for i in range(n_adapters)]
    masks = _net_masks(n_adapters, mask_hw)
    with torch.no_grad():
        ref = ipu(x, torch.tensor(500), ehs, added_cond_kwargs={"image_embeds": embeds},
                  cross_attention_kwargs={"ip_adapter_masks": masks})[0]
    return sd, sds, scales, x, ehs, embeds, masks, ref


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", list(NET_SHAPES))
@pytest.mark.parametrize("n_adapters", [1, 2])
def test_unet_with_masks_against_the_oracle(n_adapters, shape, dtype):
    """The tiny UNet (head dims 40 and 80), one adapter with a rectangle and two with complementary parts (the second adapter
    with two images per prompt: 8 tokens, the streamed form), against the oracle UNet with the restated masked processor at
    the project's network gates; the same call WITHOUT masks must fail that gate."""
    sd, sds, scales, x, ehs, embeds, masks, ref = _oracle_case(n_adapters, shape)
    h = PM.UNet2DConditionModel(in_channels=4, device=DEV, dtype=dtype, **TINY).load_state_dict(sd)
    h._load_ip_adapter_weights(sds)
    h.set_ip_adapter_scale(scales)
    t = torch.tensor(500)
    kw = dict(added_cond_kwargs={"image_embeds": [e.to(DEV) for e in embeds]}, return_dict=False)
    plain = h(x.to(DEV), t, ehs.to(DEV), **kw)[0].clone()
    assert all(c[0] is L.lib().pp_ip_attn_add for c in h.rt.step_plan.calls if c[2] == "ip_attn_add")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                       # (the off-aspect mask warns, as in diffusers)
        out = h(x.to(DEV), t, ehs.to(DEV), cross_attention_kwargs={"ip_adapter_masks": masks.to(DEV)}, **kw)[0].clone()
    ip_calls = [c for c in h.rt.step_plan.calls if c[2] == "ip_attn_add"]
    assert len(ip_calls) == 4 * n_adapters and all(c[0] is L.lib().pp_ip_attn_add_masked for c in ip_calls)
    cos, err, ok = IC.net_gate(out, ref, dtype)
    pcos, perr, pok = IC.net_gate(plain, ref, dtype)
    record(f"[ip_adapter_masks] tiny UNet {shape} {n_adapters} adapter(s) {str(dtype)[6:]}: cosine {cos:.6f} max-abs {err:.4g} "
           f"(max|ref| {float(ref.abs().max()):.3g}); unmasked output against it: cosine {pcos:.6f} max-abs {perr:.4g}")
    assert ok, (cos, err)
    assert not pok, "the unmasked output passes the gate: the test would not notice dropped masks"
    # masks dropped again: the unmasked plan and its output, bit for bit
    again = h(x.to(DEV), t, ehs.to(DEV), **kw)[0]
    assert torch.equal(again, plain)
    assert all(c[0] is L.lib().pp_ip_attn_add for c in h.rt.step_plan.calls if c[2] == "ip_attn_add")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unet_with_a_base_and_a_plus_adapter_under_masks(dtype):
    """Base and Plus adapters are alike to the step plan: a base adapter on the left part and a Plus adapter of two images (32
    tokens, the streamed form) on the right, 16x16 latents, against the oracle UNet behind the restated projections
    (ip_plus_cases.PlusIPUNet) with the restated masked processor."""
    import ip_plus_cases as PC
    scales = [0.7, 0.4]
    torch.manual_seed(1234)
    o = OM.UNet2DConditionModel(in_channels=4, **TINY).eval()
    with torch.no_grad():
        for p in o.parameters():
            if p.dim() >= 2:
                p.copy_(p.to(torch.bfloat16).float())
    h = PM.UNet2DConditionModel(in_channels=4, device=DEV, dtype=dtype, **TINY).load_state_dict(o.state_dict())
    sds = [IC.adapter_state_dict(o, 60, std=1.0), PC.plus_state_dict(o, 61, std=1.0, **PC.FIX)]
    ipu = MC.as_masked(PC.PlusIPUNet(o, sds, scales)).eval()
    g = torch.Generator().manual_seed(7)
    B = 2
    x, ehs = torch.randn(B, 4, 16, 16, generator=g), torch.randn(B, 77, 768, generator=g)
    embeds = [torch.randn(B, 1, IC.EMBED_DIM, generator=g), torch.randn(B, 2, PC.FIX_S, PC.FIX["E"], generator=g)]
    masks = _net_masks(2, (128, 128))
    t = torch.tensor(500)
    with torch.no_grad():
        ref = ipu(x, t, ehs, added_cond_kwargs={"image_embeds": embeds}, cross_attention_kwargs={"ip_adapter_masks": masks})[0]
    h._load_ip_adapter_weights(sds)
    h.set_ip_adapter_scale(scales)
    kw = dict(added_cond_kwargs={"image_embeds": [e.to(DEV) for e in embeds]}, return_dict=False)
    plain = h(x.to(DEV), t, ehs.to(DEV), **kw)[0].clone()
    out = h(x.to(DEV), t, ehs.to(DEV), cross_attention_kwargs={"ip_adapter_masks": masks}, **kw)[0].clone()
    ip_calls = [c for c in h.rt.step_plan.calls if c[2] == "ip_attn_add"]
    assert len(ip_calls) == 8 and all(c[0] is L.lib().pp_ip_attn_add_masked for c in ip_calls)
    assert sorted({c[1][9] for c in ip_calls}) == [4, 32]
    cos, err, ok = IC.net_gate(out, ref, dtype)
    pcos, perr, pok = IC.net_gate(plain, ref, dtype)
    record(f"[ip_adapter_masks] tiny UNet 16x16 base+plus {str(dtype)[6:]}: cosine {cos:.6f} max-abs {err:.4g} (max|ref| "
           f"{float(ref.abs().max()):.3g}); unmasked output against it: cosine {pcos:.6f} max-abs {perr:.4g}")
    assert ok, (cos, err)
    assert not pok, "the unmasked output passes the gate: the test would not notice dropped masks"


# ------------------------------------------------------------------------------------------------------------ pipeline
@functools.lru_cache(maxsize=None)
def _fixture(name="ref_ip_adapter_masks.pt"):
    return torch.load(os.path.join(HERE, "golden", name), weights_only=False)


def _pipeline(dtype, case):
    """The BrushNet pipeline of tests/test_ip_adapter_gpu.py with the adapters of `case` (an ip_adapter_cases name) loaded."""
    import make_ref_ip_adapter as M
    import make_ref_lcm as ML
    import make_ref_pipeline_call as MP
    from test_lcm_gpu import _hip_text_vae
    tok, enc, u4, bn, vae = ML.components("v2")
    he, hv = _hip_text_vae(enc, vae, MP)
    hu = PM.UNet2DConditionModel(in_channels=4, device=DEV, dtype=dtype, **ML.CFG).load_state_dict(u4.state_dict())
    hb = PM.BrushNetModel(in_channels=4, conditioning_channels=5, device=DEV, dtype=dtype, **ML.CFG).load_state_dict(bn.state_dict())
    sch = PS.DPMSolverMultistepScheduler.from_config(PS.PNDMScheduler().config)        # the SD-1.5 config: leading, offset 1
    pipe = PP.StableDiffusionPowerPaintBrushNetPipeline(vae=hv, text_encoder=he, text_encoder_brushnet=he, tokenizer=tok,
                                                        unet=hu, brushnet=hb, scheduler=sch)
    img, mask3, _ = MP.inputs_v2()
    rep = torch.cat([img.repeat(M.NB, 1, 1, 1)] * 2)
    dist = hv.encode(rep.to(DEV)).latent_dist
    torch.manual_seed(9)
    noise = torch.randn(dist.mean.shape)                          # CPU global RNG, as in the reference run
    cl = (dist.mean + dist.std * noise.to(DEV)) * hv.config.scaling_factor
    keep = (torch.cat([mask3.repeat(M.NB, 1, 1, 1)] * 2).sum(1)[:, None] < 0).float()
    cond = torch.cat([cl, torch.nn.functional.interpolate(keep, size=cl.shape[-2:]).to(DEV)], 1)
    pipe.load_ip_adapter(IC.case_adapters(u4, case))
    pipe.set_ip_adapter_scale(IC.CASES[case]["scales"])
    embeds = [e.to(DEV) for e in IC.case_prompt(case, 0)["ip_adapter_image_embeds"]]

    def call(masks=None, graph=True):
        pipe.use_graph = graph
        g = torch.Generator().manual_seed(IC.SEED)
        kw = dict(cross_attention_kwargs={"ip_adapter_masks": masks.to(DEV)}) if masks is not None else {}
        out = pipe(conditioning_latents=cond, latents=ML.start_latents().to(DEV), generator=g, output_type="latent",
                   return_dict=False, ip_adapter_image_embeds=embeds, **kw, **M.CALL)[0]
        return out.float().cpu(), g

    return pipe, call


def _against(out, gen, want, next_draw, what):
    cos, err, ok = IC.loop_gate(out, want)
    record(f"[ip_adapter_masks] {what}: cosine {cos:.6f} max-abs {err:.4g} of max|ref| {float(want.abs().max()):.4g}")
    assert torch.equal(torch.randn(4, generator=gen), next_draw), f"{what}: the generator is not where the reference leaves it"
    assert ok, (what, cos, err)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(MC.CASES))
def test_brushnet_pipeline_with_masks_against_the_reference_call(name, dtype):
    """Every fixture case, graph replay on."""
    gold = _fixture()[name]
    assert not IC.loop_gate(gold["unmasked"], gold["latents"])[2]
    pipe, call = _pipeline(dtype, MC.CASES[name][0])
    out, g = call(MC.case_masks(name), graph=True)
    unet_calls = [c for c in pipe._loop.rt.step_plan.calls if c[2] == "ip_attn_add"]
    side_names = [c[2] for c in pipe._loop.side_rt.step_plan.calls]
    n_x = len(pipe.unet.net._attn_specs())
    assert len(unet_calls) == n_x * IC.CASES[MC.CASES[name][0]]["n"] and "ip_attn_add" not in side_names
    assert all(c[0] is L.lib().pp_ip_attn_add_masked for c in unet_calls)
    assert pipe._loop.graph is not None
    _against(out, g, gold["latents"], gold["next_draw"], f"BrushNet pipeline, masks `{name}`, graph, {str(dtype)[6:]}")


def test_new_masks_reuse_the_graph_and_dropping_them_restores_the_unmasked_pipeline():
    G, P = _fixture(), _fixture("ref_ip_adapter.pt")
    pipe, call = _pipeline(torch.bfloat16, "one")
    out, g = call(MC.case_masks("one"))
    _against(out, g, G["one"]["latents"], G["one"]["next_draw"], "masks `one`, first call")
    graph, plan = pipe._loop.graph, pipe._loop.rt.step_plan
    assert graph is not None
    out2, g2 = call(MC.case_masks("one_b"))
    assert pipe._loop.graph is graph and pipe._loop.rt.step_plan is plan, "new masks of the same count re-captured the graph"
    _against(out2, g2, G["one_b"]["latents"], G["one_b"]["next_draw"], "masks `one_b`, second call on the captured graph")
    assert not IC.loop_gate(out2, G["one"]["latents"])[2]
    out3, g3 = call(None)
    _against(out3, g3, P["one"]["latents"], P["one"]["next_draw"], "no masks afterwards (ref_ip_adapter.pt `one`)")
    assert all(c[0] is L.lib().pp_ip_attn_add for c in pipe._loop.rt.step_plan.calls if c[2] == "ip_attn_add")
