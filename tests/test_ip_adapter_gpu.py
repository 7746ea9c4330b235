"""-m gpu: IP-Adapter image prompts on the HIP path -- pp_ip_attn_add alone against a float64 evaluation of its formula, the
UNet with one and two adapters against the oracle UNet with the restated IPAttention (tests/ip_adapter_cases.py), and the
BrushNet pipeline against the reference's own `__call__` (tests/golden/ref_ip_adapter.pt).

The kernel's gate (ip_adapter_cases.kernel_gate), per output element, with u = 2^-24 (fp32 unit roundoff):

    |out - ref| <= r16 |ref| + u (2 (d + 2) S + nk + 40) (|o| + |ip_scale| sum_j |p_j v_j|) [+ 2^-24 for fp16]

  * r16 |ref|: the ONE rounding to the output format, 2^-8 |ref| for bf16 and 2^-11 |ref| for fp16 (the issue's figures: a
    full unit in the last place, twice the round-to-nearest half unit); fp16 adds its subnormal spacing 2^-24 as a floor.
  * the fp32 term is relative to the magnitudes that are summed, |o| + |ip_scale| sum_j |p_j v_j|:
      - a score is d fused multiply-adds and log2(d / 8) + 1 partial sums and one multiply by qk_scale: its error is at most
        (d + 2) u S with S = max_j qk_scale sum_i |q_i k_ji| (computed from the INPUTS, per row and head).  A score error e
        multiplies p_j by exp(e) in the numerator and moves the denominator by as much: 2 (d + 2) u S relative, to first order
        -- this is the term that grows with the logits (S ~ 100 in the large-logit case: 2e-3, more than an fp16 rounding);
      - exp: the argument (s_j - m) in [-160, 0] is formed in fp32 and scaled by log2(e) in fp32, 2 u |s_j - m| -- terms that
        weigh anything have |s_j - m| < 17 -- plus the hardware exp2's ~1 ulp: bounded by 36 u;
      - the nk-term sums of the numerator and the denominator (nk u), the division and the final multiply-add (4 u).
  Nothing in the gate comes from the kernel's output.
Achieved numbers are printed and appended to profiles/ip_adapter_parity_achieved.txt before anything is asserted.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import ip_adapter_cases as IC  # noqa: E402
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
        with open(os.path.join(ROOT, "profiles", "ip_adapter_parity_achieved.txt"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run_kernel(q, k, v, o, batch, heads, d, nq, nk, qk_scale, ip_scale, dtype):
    """o: [batch * nq][ldo] host tensor -> the device result [batch * nq + GUARD][ldo] (guard rows and row gaps hold a
    sentinel), and the device copy of q after the launch."""
    C = heads * d
    ldq, ldo = q.shape[1], o.shape[1]
    sent = torch.tensor(-1234.0).to(dtype)
    od = torch.full((batch * nq + GUARD, ldo), float(sent), dtype=dtype)
    od[:batch * nq, :C] = o[:, :C]
    od = od.to(DEV)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    L.check(L.lib().pp_ip_attn_add(qd.data_ptr(), ldq, kd.data_ptr(), vd.data_ptr(), od.data_ptr(), ldo, batch, heads, nq, nk,
                                   d, qk_scale, ip_scale, L.dtype_code(dtype), _stream()), "pp_ip_attn_add")
    torch.cuda.synchronize()
    return od.cpu(), qd.cpu(), sent


def _check(out, sent, q_after, q, k, v, o, batch, heads, d, nq, nk, qk_scale, ip_scale, dtype, what):
    C = heads * d
    M = batch * nq
    assert torch.equal(q_after, q), f"{what}: q was modified"
    assert bool((out[M:] == sent).all()), f"{what}: rows behind the last row were written"
    if out.shape[1] > C:
        assert bool((out[:M, C:] == sent).all()), f"{what}: the gaps between rows were written"
    ref, mag, smax = IC.kernel_ref(q, k, v, o, batch, heads, d, nq, nk, qk_scale, ip_scale)
    got = out[:M, :C].double()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    tol = IC.kernel_gate(ref, mag, smax, d, nk, dtype)
    return float(((got - ref).abs() / tol).max())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("heads,d", IC.KERNEL_HEADS_D)
def test_pp_ip_attn_add_against_float64(heads, d, dtype):
    """Every (nq, nk) of the grid at batch 2 with different K / V per item: nq = 1 and 100 leave partial row groups (and, at
    one head of 40 channels, 12 rows per wave pass), nk = 1 / 4 run the register form, 8 / 16 the streamed one; dense strides
    and ldq = 2 C, ldo = C + 8 (row gaps, which must keep their sentinel, as must the rows behind the last)."""
    C, batch = heads * d, 2
    worst = {}
    for nq in IC.KERNEL_NQ:
        for nk in IC.KERNEL_NK:
            for ldq, ldo in ((C, C), (2 * C, C + 8)):
                q, k, v, o = IC.kernel_inputs(batch, heads, d, nq, nk, dtype, ldq, ldo, seed=nq * 100 + nk)
                assert not torch.equal(k[0], k[1])
                qk, sc = d ** -0.5, 0.7
                out, q_after, sent = _run_kernel(q, k, v, o, batch, heads, d, nq, nk, qk, sc, dtype)
                w = _check(out, sent, q_after, q, k, v, o, batch, heads, d, nq, nk, qk, sc, dtype,
                           f"heads {heads} d {d} nq {nq} nk {nk} ldq {ldq} ldo {ldo}")
                worst[(nq, nk, ldo)] = w
    top = max(worst, key=worst.get)
    record(f"[ip_adapter] kernel heads {heads} d {d} {str(dtype)[6:]}: worst err / bound over {len(worst)} shapes "
           f"{worst[top]:.3g} at (nq, nk, ldo) = {top}")
    assert worst[top] <= 1.0, (top, worst[top])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pp_ip_attn_add_scale_zero_is_bit_identical(dtype):
    heads, d, nq, nk, batch = 8, 40, 100, 4, 2
    q, k, v, o = IC.kernel_inputs(batch, heads, d, nq, nk, dtype, seed=5)
    o[0, :8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 6e-8, -6e-8, 3.0, -3.0]).to(dtype)      # (signed zeros, tiny values)
    out, q_after, sent = _run_kernel(q, k, v, o, batch, heads, d, nq, nk, d ** -0.5, 0.0, dtype)
    assert torch.equal(out[:batch * nq].view(torch.int16), o.view(torch.int16)) and torch.equal(q_after, q)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("nk", [4, 16])
def test_pp_ip_attn_add_large_logits(nk, dtype):
    """|qk_scale * q . k| up to about 80: the maximum is subtracted, nothing overflows, and the result stays inside the gate
    (whose score term is what grows here)."""
    heads, d, nq, batch = 8, 80, 64, 2
    q, k, v, o = IC.kernel_inputs(batch, heads, d, nq, nk, dtype, seed=9, logit=80.0)
    qk = d ** -0.5
    s = torch.einsum("bqhd,bkhd->bhqk", q.double().view(batch, nq, heads, d), k.double().view(batch, nk, heads, d)) * qk
    assert 50.0 < float(s.abs().max()) < 160.0, float(s.abs().max())
    out, q_after, sent = _run_kernel(q, k, v, o, batch, heads, d, nq, nk, qk, 1.0, dtype)
    w = _check(out, sent, q_after, q, k, v, o, batch, heads, d, nq, nk, qk, 1.0, dtype, f"large logits nk {nk}")
    record(f"[ip_adapter] kernel large logits (max |s| {float(s.abs().max()):.1f}) nk {nk} {str(dtype)[6:]}: worst err / bound {w:.3g}")
    assert w <= 1.0, w


# ------------------------------------------------------------------------------------------------------------ network
TINY = dict(block_out_channels=(320, 640), layers_per_block=1,
            down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"))


def _tiny_pair(dtype, n_adapters, scales):
    torch.manual_seed(1234)
    o = OM.UNet2DConditionModel(in_channels=4, **TINY).eval()
    with torch.no_grad():
        for p in o.parameters():
            if p.dim() >= 2:
                p.copy_(p.to(torch.bfloat16).float())
    h = PM.UNet2DConditionModel(in_channels=4, device=DEV, dtype=dtype, **TINY).load_state_dict(o.state_dict())
    sds = [IC.adapter_state_dict(o, 50 + i, std=1.0) for i in range(n_adapters)]
    ipu = IC.IPUNet(o, sds, scales).eval()
    return o, ipu, h, sds


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("hw", [(8, 8), (5, 6)], ids=["8x8", "5x6"])
@pytest.mark.parametrize("n_adapters", [1, 2])
def test_unet_with_adapters_against_the_oracle(n_adapters, hw, dtype):
    """The tiny UNet (head dims 40 and 80) at 8x8 and at 5x6 latents (an odd level below: 3x3), one adapter and two (the second
    with two images per prompt: 8 tokens, the streamed form), against the oracle UNet with IPAttention at the project's
    network gates; the adapter-free HIP output must FAIL the same gate."""
    scales = [1.0] if n_adapters == 1 else [0.7, 0.4]
    o, ipu, h, sds = _tiny_pair(dtype, n_adapters, scales)
    g = torch.Generator().manual_seed(hw[0] * 10 + n_adapters)
    B = 2
    x = torch.randn(B, 4, *hw, generator=g)
    ehs = torch.randn(B, 77, 768, generator=g)
    embeds = [torch.randn(B, 1 + i, IC.EMBED_DIM, generator=g) for i in range(n_adapters)]
    t = torch.tensor(500)
    with torch.no_grad():
        ref = ipu(x, t, ehs, added_cond_kwargs={"image_embeds": embeds})[0]
    plain = h(x.to(DEV), t, ehs.to(DEV), return_dict=False)[0]
    with pytest.raises(L.PPError):
        h(x.to(DEV), t, ehs.to(DEV), added_cond_kwargs={"image_embeds": embeds})         # no adapter loaded: refused
    h._load_ip_adapter_weights(sds)
    h.set_ip_adapter_scale(scales)
    with pytest.raises(ValueError, match="ip_image_proj"):
        h(x.to(DEV), t, ehs.to(DEV))
    out = h(x.to(DEV), t, ehs.to(DEV), added_cond_kwargs={"image_embeds": [e.to(DEV) for e in embeds]}, return_dict=False)[0]
    names = [c[2] for c in h.rt.step_plan.calls]
    assert names.count("ip_attn_add") == 4 * n_adapters and "xattn_block" not in names
    cos, err, ok = IC.net_gate(out, ref, dtype)
    pcos, perr, pok = IC.net_gate(plain, ref, dtype)
    record(f"[ip_adapter] tiny UNet {hw[0]}x{hw[1]} {n_adapters} adapter(s) {str(dtype)[6:]}: cosine {cos:.6f} max-abs {err:.4g} "
           f"(max|ref| {float(ref.abs().max()):.3g}); adapter-free output against it: cosine {pcos:.6f} max-abs {perr:.4g}")
    assert ok, (cos, err)
    assert not pok, "the adapter-free output passes the gate: the test would not notice a missing adapter"
    # unloaded again: the output of the UNet that never had one, bit for bit
    h._unload_ip_adapter()
    again = h(x.to(DEV), t, ehs.to(DEV), return_dict=False)[0]
    assert torch.equal(again, plain)


# ------------------------------------------------------------------------------------------------------------ pipeline
_GOLD = None


def _fixture():
    global _GOLD
    if _GOLD is None:
        _GOLD = torch.load(os.path.join(HERE, "golden", "ref_ip_adapter.pt"), weights_only=False)
    return _GOLD


def _pipeline(dtype, case=None):
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
    if case is not None:
        pipe.load_ip_adapter(IC.case_adapters(u4, case))
        pipe.set_ip_adapter_scale(IC.CASES[case]["scales"])
        if IC.CASES[case]["encoder"]:
            pipe.image_encoder = IC.TinyImageEncoder().eval().to(DEV)

    def call(prompt=None, graph=True):
        pipe.use_graph = graph
        g = torch.Generator().manual_seed(IC.SEED)
        prompt = {k: ([e.to(DEV) for e in v] if isinstance(v, list) else v.to(DEV)) for k, v in (prompt or {}).items()}
        out = pipe(conditioning_latents=cond, latents=ML.start_latents().to(DEV), generator=g, output_type="latent",
                   return_dict=False, **prompt, **M.CALL)[0]
        return out.float().cpu(), g

    return pipe, call


def _against(out, gen, gold, what):
    cos, err, ok = IC.loop_gate(out, gold["latents"])
    pcos, perr, pok = IC.loop_gate(gold["plain"], gold["latents"])
    record(f"[ip_adapter] {what}: cosine {cos:.6f} max-abs {err:.4g} of max|ref| {float(gold['latents'].abs().max()):.4g} "
           f"(adapter-free reference latents: cosine {pcos:.5f}, {perr:.3g})")
    assert torch.equal(torch.randn(4, generator=gen), gold["next_draw"]), f"{what}: the generator is not where the reference leaves it"
    assert not pok
    assert ok, (what, cos, err)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", list(IC.CASES))
def test_brushnet_pipeline_against_the_reference_call(case, dtype):
    pipe, call = _pipeline(dtype, case)
    for graph in (True, False):
        out, g = call(IC.case_prompt(case), graph)
        names = [c[2] for c in pipe._loop.program.calls]
        unet_names = [c[2] for c in pipe._loop.rt.step_plan.calls]
        side_names = [c[2] for c in pipe._loop.side_rt.step_plan.calls]
        n_x = len(pipe.unet.net._attn_specs())                    # (the UNet's cross-attentions only: BrushNet receives nothing)
        assert names.count("ip_attn_add") == unet_names.count("ip_attn_add") == n_x * IC.CASES[case]["n"]
        assert "xattn_block" not in unet_names and "ip_attn_add" not in side_names and "xattn_block" in side_names
        _against(out, g, _fixture()[case], f"BrushNet pipeline, case {case}, {'graph' if graph else 'eager'}, {str(dtype)[6:]}")


def test_second_call_with_other_embeds_matches_its_own_reference():
    pipe, call = _pipeline(torch.bfloat16, "one")
    out, g = call(IC.case_prompt("one", 0))
    _against(out, g, _fixture()["one"], "per-call state, first call")
    out2, g2 = call(IC.case_prompt("one", 1))
    _against(out2, g2, _fixture()["one_b"], "per-call state, second call (other embeds)")
    assert not IC.loop_gate(out2, _fixture()["one"]["latents"])[2]


def test_scale_changes_reach_the_graph_and_unload_restores_the_plain_pipeline():
    pipe, call = _pipeline(torch.bfloat16, "one")
    prompt = IC.case_prompt("one")
    outs = {}
    for s in (1.0, 0.5, 1.0):
        pipe.set_ip_adapter_scale(s)
        a, _ = call(prompt, graph=True)
        b, _ = call(prompt, graph=False)
        assert torch.equal(a, b), f"scale {s}: graph and eager differ"
        if s in outs:
            assert torch.equal(outs[s], a)
        outs[s] = a
    assert not torch.equal(outs[1.0], outs[0.5])
    a, g = call(prompt)
    assert torch.equal(a, outs[1.0])
    _against(a, g, _fixture()["one"], "scale back at 1.0")
    pipe.unload_ip_adapter()
    assert pipe.unet.config.encoder_hid_dim_type is None and pipe.unet.encoder_hid_proj is None
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        call(prompt)
    after, _ = call()
    never, call2 = _pipeline(torch.bfloat16, None)
    want, _ = call2()
    assert torch.equal(after, want), "after unload_ip_adapter the pipeline is not the one that never loaded an adapter"
