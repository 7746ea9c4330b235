"""-m gpu: IP-Adapter Plus on the HIP path -- pp_perceiver_attn alone (an exact walk over every key of both segments, then
random values against a float64 evaluation), pp_ip_attn_add at the token counts Plus brings, the setup plan's Resampler
against the Resampler restated from the file format (tests/ip_plus_cases.py), the UNet with a Plus adapter against the oracle
UNet, and the BrushNet pipeline against the reference's own `__call__` (tests/golden/ref_ip_adapter_plus.pt).

pp_perceiver_attn's gate (ip_plus_cases.perceiver_gate), per output element, with u = 2^-24 (fp32 unit roundoff), d = 64,
S = max_t scale sum_j |q_j k_tj| per (row, head) and M = sum_t |p_t v_t| (both from the INPUTS, in float64):

    |out - ref| <= r16 |ref| + r16 M + u (2 (d + 4) S + 3 nk + 40) M  [+ 2^-24 + nk 2^-25 max|v| for fp16]

  * r16 is the unit roundoff of the 16-bit format, the largest relative error of one rounding to nearest: 2^-8 for bf16 (8
    significant bits), 2^-11 for fp16 (11) -- the figures ip_adapter_cases.kernel_gate uses.
  * r16 |ref|: the ONE rounding of the result; fp16 adds its subnormal spacing 2^-24 as a floor.
  * r16 M: the kernel rounds every probability once to the 16-bit format for the P V matrix product, while the denominator
    sums the unrounded ones: each term p_t v_t moves by at most r16 of itself.  An fp16 probability below 2^-14 is subnormal
    and moves by up to half its spacing, 2^-25, absolutely: nk 2^-25 max|v| in all (the denominator is >= 1).  bf16 has
    fp32's exponent range: no such floor.
  * the fp32 term, relative to M:
      - a score is a 64-term fp32 dot product (the products of two 16-bit numbers are exact in fp32) and one multiply by
        `scale`: its error is at most (d + 2) u S, and a score error e multiplies p_t by exp(e) in the numerator and moves the
        denominator by as much: 2 (d + 2) u S;
      - the keys are walked in tiles with a running maximum: p_t is exp(s_t - m_tile) times the later corrections
        exp(m_old - m_new).  The exponents of that chain add up to m_final - s_t <= 2 S; each is formed in fp32 and scaled by
        log2(e) in fp32, 2 u of its magnitude: 4 u S.  The hardware exp2's ~1 ulp per factor, the per-tile rescaling of the
        accumulators and of the sum, the division and the final multiply: bounded by (nk + 40) u (at most one tile per key);
      - the nk-term fp32 sums of the numerator and the denominator: 2 nk u.
  Nothing in the gate comes from the kernel's output.  Before anything runs on the GPU the test checks on the CPU that an fp32
  evaluation of the same formula stays inside the bound and that the result with ONE key dropped does not.
Achieved numbers are printed and appended to profiles/ip_adapter_plus_parity_achieved.txt before anything is asserted.
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
import ip_plus_cases as PC  # noqa: E402
from oracle import sd_modules as OM  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import models as PM  # noqa: E402
from powerpaint_amd import ops  # noqa: E402

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
D = PC.HEAD_DIM
GUARD = 3             # sentinel rows behind the last row of o, poisoned rows behind each K / V segment
POISON = 3.0e4        # large and finite in both formats


def record(line: str):
    print(line)
    try:
        with open(os.path.join(ROOT, "profiles", "ip_adapter_plus_parity_achieved.txt"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def _segment(rows, cols, ld, dtype):
    """`rows` real rows of `cols` columns inside a poisoned [rows + GUARD][ld] buffer (None for an empty segment)."""
    if rows is None:
        return None, None
    full = torch.full((rows.shape[0] + GUARD, ld), POISON, dtype=dtype)
    full[:rows.shape[0], :cols] = rows[:, :cols]
    full = full.to(DEV)
    return full, full[:rows.shape[0], :cols]


def _launch(q, kv_x, kv_l, batch, heads, nq, scale, dtype, pad=16):
    """q [batch * nq][>= C], kv_x / kv_l [batch * n][>= 2 C] host tensors -> (o [batch * nq][C] on the host, the error text of
    whatever was written outside it or read-only operands that changed, '' if none)."""
    C = heads * D
    sent = float(torch.tensor(-1234.0).to(dtype))
    ofull = torch.full((batch * nq + GUARD, C + pad), sent, dtype=dtype, device=DEV)
    qd = q.to(DEV)
    xf, xv = _segment(kv_x, 2 * C, 2 * C + pad, dtype)
    lf, lv = _segment(kv_l, 2 * C, 2 * C + pad, dtype)
    keep = [t.clone() for t in (qd, xf, lf) if t is not None]
    ops.perceiver_attention(qd[:, :C] if qd.shape[1] > C else qd, xv, lv, batch, heads, nq, scale=scale,
                            out=ofull[:batch * nq, :C])
    torch.cuda.synchronize()
    bad = ""
    if not bool((ofull[batch * nq:] == sent).all()):
        bad += " rows behind the last row of o were written;"
    if not bool((ofull[:batch * nq, C:] == sent).all()):
        bad += " the gaps between the rows of o were written;"
    if not all(torch.equal(a, b) for a, b in zip(keep, [t for t in (qd, xf, lf) if t is not None])):
        bad += " an input was modified;"
    return ofull[:batch * nq, :C].contiguous().cpu(), bad


# ------------------------------------------------------------------------------------------------------ kernel, exact walk
NC = 320          # sign codes: more than the 273 keys of the largest case
A_Q, BIAS = 16.0, 47.0


def _codes():
    g = torch.Generator().manual_seed(99)
    c = torch.where(torch.randn(NC, D - 1, generator=g) >= 0, 1.0, -1.0)
    ham = ((D - 1) - c @ c.t()) / 2 + 1e9 * torch.eye(NC)
    assert int(ham.min()) >= 12, int(ham.min())
    return torch.cat([c, torch.ones(NC, 1)], 1)                   # the constant column carries the bias


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("heads", [1, 12])
@pytest.mark.parametrize("nx,nl", [(1, 0), (10, 16), (257, 16), (64, 64)])
def test_pp_perceiver_attn_exact_walk_over_every_key(nx, nl, heads, dtype):
    """Key t of (item b, head h) is a +-1 code of 63 entries and a constant 1; query i is 16 times the code of its key pi(i) and
    -16 * 47 on the constant.  Any two codes differ in at least 12 places (checked), so with scale 1 the score of pi(i) is
    16 (63 - 47) = 256 and every other one at most 16 (63 - 24 - 47) = -128: all exact integers, all finite, and exp(-384)
    underflows to 0 in fp32 -- o must be V's row pi(i), bit for bit.  pi(b, h, i) = (16 launch + i + 7 b + 3 h) mod nk visits
    every key of both segments over the launches; codes and V differ per item, head and key (a wrong segment, head offset or
    K | V column shows); poisoned rows behind each segment, poisoned pad columns, sentinel-filled o with guard rows."""
    batch, nq, nk, C = 3, 16, nx + nl, heads * D
    codes = _codes()
    g = torch.Generator().manual_seed(nx * 100 + nl + heads)
    b_, t_, h_ = torch.meshgrid(torch.arange(batch), torch.arange(nk), torch.arange(heads), indexing="ij")
    K = codes[(t_ + 5 * h_ + 11 * b_) % NC]                                         # [batch, nk, heads, 64]
    V = torch.randn(batch, nk, heads, D, generator=g).to(dtype)
    V = torch.where(V == 0, torch.ones_like(V), V)                                  # (a signed zero would not survive a sum)
    assert len(torch.unique(V.float().reshape(-1, D), dim=0)) == batch * nk * heads
    kv = torch.cat([K.reshape(batch, nk, C).to(dtype), V.reshape(batch, nk, C)], 2)
    kv_x = kv[:, :nx].reshape(batch * nx, 2 * C)
    kv_l = kv[:, nx:].reshape(batch * nl, 2 * C) if nl else None
    bq, iq, hq = torch.meshgrid(torch.arange(batch), torch.arange(nq), torch.arange(heads), indexing="ij")
    seen = torch.zeros(batch, heads, nk, dtype=torch.bool)
    for launch in range((nk + nq - 1) // nq):
        pi = (nq * launch + iq + 7 * bq + 3 * hq) % nk                              # [batch, nq, heads]
        q = A_Q * codes[(pi + 5 * hq + 11 * bq) % NC]
        q[..., D - 1] = -A_Q * BIAS
        q = q.reshape(batch * nq, C).to(dtype)
        assert torch.equal(q.float(), q.float().round())                           # exact in the format
        o, bad = _launch(q, kv_x, kv_l, batch, heads, nq, 1.0, dtype)
        assert not bad, (launch, bad)
        want = V[bq, pi, hq].reshape(batch * nq, C)
        assert torch.equal(o.view(torch.int16), want.view(torch.int16)), \
            (launch, int((o.view(torch.int16) != want.view(torch.int16)).sum()))
        seen[bq, hq, pi] = True
    assert bool(seen.all())


# ------------------------------------------------------------------------------------------------------ kernel, values
def _top_key(q, kv_x, kv_l, batch, heads, scale):
    """The key with the largest probability for (item 0, query 0, head 0)."""
    nx = kv_x.shape[0] // batch
    k = kv_x[:nx, :D].double()
    if kv_l is not None:
        k = torch.cat([k, kv_l[:kv_l.shape[0] // batch, :D].double()])
    return int((k @ q[0, :D].double()).argmax())


def _values_case(batch, heads, nq, nx, nl, dtype, what, **kw):
    scale = D ** -0.5
    q, kv_x, kv_l = PC.perceiver_inputs(batch, heads, nq, nx, nl, dtype, **kw)
    C = heads * D
    ref, mag, smax, vmax = PC.perceiver_ref(q, kv_x, kv_l, batch, heads, nq, scale)
    tol = PC.perceiver_gate(ref, mag, smax, vmax, nx + nl, dtype)
    # the bound holds for an fp32 evaluation and notices one missing key -- on the CPU, before the kernel runs
    f32 = PC.perceiver_ref(q, kv_x, kv_l, batch, heads, nq, scale, dt=torch.float32)[0].double()
    assert float(((f32 - ref).abs() / tol).max()) <= 1.0, what
    if nx + nl > 1:
        dropped = PC.perceiver_ref(q, kv_x, kv_l, batch, heads, nq, scale, drop=_top_key(q, kv_x, kv_l, batch, heads, scale))[0]
        assert float(((dropped - ref).abs() / tol).max()) > 1.0, f"{what}: the bound would not notice a missing key"
    o, bad = _launch(q, kv_x, kv_l, batch, heads, nq, scale, dtype)
    assert not bad, (what, bad)
    got = o.double()
    assert bool(torch.isfinite(got).all()), what
    return float(((got - ref).abs() / tol).max()), float(smax.max())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("nx,nl", [(257, 16), (577, 64), (3, 1)])
def test_pp_perceiver_attn_against_float64(nx, nl, dtype):
    """nq = 1, 16, 17 and 64 (a lone query, one full tile, a tile of one query behind a full one, four tiles), two heads, two
    batch items with different K / V; 273 and 641 keys end in a partial tile, (3, 1) fits in one; q, K | V with pad columns."""
    worst = {}
    for nq in (1, 16, 17, 64):
        w, _ = _values_case(2, 2, nq, nx, nl, dtype, f"nq {nq} nx {nx} nl {nl}", seed=nq + nx)
        worst[nq] = w
    top = max(worst, key=worst.get)
    record(f"[ip_adapter_plus] perceiver_attn (nx, nl) = ({nx}, {nl}) {str(dtype)[6:]}: worst err / bound over nq in (1, 16, 17, 64) "
           f"{worst[top]:.3g} at nq = {top}")
    assert worst[top] <= 1.0, (top, worst[top])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("where", ["last", "first"])
def test_pp_perceiver_attn_large_logits_across_key_tiles(where, dtype):
    """Logits reaching +-30 and beyond, the key with the largest ones in the LAST tile of the walk (the running maximum rises at
    the end and everything accumulated before is rescaled) and in the FIRST (everything behind it is scaled down)."""
    nx, nl, nq = 257, 16, 17
    big = nx + nl - 1 if where == "last" else 0
    w, smax = _values_case(2, 2, nq, nx, nl, dtype, f"large logits, largest key {where}", seed=3, logit=20.0, big_key=big)
    q, kv_x, kv_l = PC.perceiver_inputs(2, 2, nq, nx, nl, dtype, seed=3, logit=20.0, big_key=big)
    k = torch.cat([kv_x.double().view(2, nx, -1), kv_l.double().view(2, nl, -1)], 1)[:, :, :2 * D].view(2, nx + nl, 2, D)
    s = torch.einsum("bqhd,bkhd->bhqk", q[:, :2 * D].double().view(2, nq, 2, D), k) * D ** -0.5
    assert 30.0 <= float(s.abs().max()) < 120.0 and int(s.abs().amax((0, 1, 2)).argmax()) == big, float(s.abs().max())
    record(f"[ip_adapter_plus] perceiver_attn large logits (max |s| {float(s.abs().max()):.1f}, S {smax:.0f}), largest key in the "
           f"{where} tile, {str(dtype)[6:]}: worst err / bound {w:.3g}")
    assert w <= 1.0, w


# ------------------------------------------------------------------------------------- pp_ip_attn_add at Plus's token counts
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("heads,d", IC.KERNEL_HEADS_D)
def test_pp_ip_attn_add_at_16_to_64_tokens(heads, d, dtype):
    """16 tokens per image and one to four images: nk = 16, 32, 48, 64 (the streamed form, up to its limit), nq = 1 and 100,
    against ip_adapter_cases.kernel_ref / kernel_gate as tests/test_ip_adapter_gpu.py checks the counts up to 16."""
    from test_ip_adapter_gpu import _check, _run_kernel
    C, batch = heads * d, 2
    worst = {}
    for nq in (1, 100):
        for nk in (16, 32, 48, 64):
            q, k, v, o = IC.kernel_inputs(batch, heads, d, nq, nk, dtype, 2 * C, C + 8, seed=nq * 100 + nk)
            qk, sc = d ** -0.5, 0.7
            out, q_after, sent = _run_kernel(q, k, v, o, batch, heads, d, nq, nk, qk, sc, dtype)
            worst[(nq, nk)] = _check(out, sent, q_after, q, k, v, o, batch, heads, d, nq, nk, qk, sc, dtype,
                                     f"heads {heads} d {d} nq {nq} nk {nk}")
    top = max(worst, key=worst.get)
    record(f"[ip_adapter_plus] ip_attn_add heads {heads} d {d} {str(dtype)[6:]}: worst err / bound over nk in (16, 32, 48, 64) "
           f"{worst[top]:.3g} at (nq, nk) = {top}")
    assert worst[top] <= 1.0, (top, worst[top])


# ------------------------------------------------------------------------------------------------------------ network
TINY = dict(block_out_channels=(320, 640), layers_per_block=1,
            down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"))
PLAN_SIZES = dict(E=320, dim=128, heads=2, ff=512, depth=2)
_NETS = {}


def _tiny_pair(dtype):
    """(oracle UNet with bf16-rounded matrices, HIP UNet of `dtype` with its weights): built once per format."""
    if dtype not in _NETS:
        torch.manual_seed(1234)
        o = OM.UNet2DConditionModel(in_channels=4, **TINY).eval()
        with torch.no_grad():
            for p in o.parameters():
                if p.dim() >= 2:
                    p.copy_(p.to(torch.bfloat16).float())
        h = PM.UNet2DConditionModel(in_channels=4, device=DEV, dtype=dtype, **TINY).load_state_dict(o.state_dict())
        _NETS[dtype] = (o, h)
    return _NETS[dtype]


def _tower_gate(got, want):
    """The towers' gate (tests/test_clip.py, tests/test_clip_vision.py)."""
    got, want = got.float().cpu(), want.float()
    cos = torch.nn.functional.cosine_similarity(got.flatten(), want.flatten(), dim=0).item()
    err = (got - want).abs().max().item()
    return cos, err, cos >= 0.9995 and err <= 0.03 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,n", [(2, 1), (2, 2)])
@pytest.mark.parametrize("Q", [4, 16])
def test_setup_plan_resampler_against_the_restated_resampler(Q, B, n, dtype):
    """The image tokens the setup plan leaves for the K_i / V_i GEMMs against the fp32 Resampler on the same 16-bit inputs and
    matrices: E = 320, dim = 128, two heads, ff = 512, depth 2, S = 10 hidden states per image."""
    o, h = _tiny_pair(dtype)
    S = 10
    sd = PC.plus_state_dict(o, 40 + Q, Q=Q, **PLAN_SIZES)
    g = torch.Generator().manual_seed(Q * 10 + n)
    embeds = torch.randn(B, n, S, PLAN_SIZES["E"], generator=g).to(dtype)
    ip = {k: (v.to(dtype).float() if v.dim() >= 2 else v) for k, v in sd["image_proj"].items()}
    with torch.no_grad():
        want = PC.Resampler.from_file(ip)(embeds.float().reshape(B * n, S, -1)).reshape(B, n * Q, IC.CTX)
    h._load_ip_adapter_weights(sd)
    try:
        x, ehs = torch.randn(B, 4, 8, 8, generator=g), torch.randn(B, 77, 768, generator=g)
        h(x.to(DEV), torch.tensor(500), ehs.to(DEV), added_cond_kwargs={"image_embeds": [embeds.to(DEV)]})
        names = [c[2] for c in h.rt.setup_plan.calls]
        assert names.count("perceiver_attn") == PLAN_SIZES["depth"] and names[10 * PLAN_SIZES["depth"] + 2] == "layernorm"
        (ptr, nt), = h.net.ip_tok
        assert nt == n * Q
        torch.cuda.synchronize()
        got = h.rt.arena.view(ptr, (B, n * Q, IC.CTX), dtype).clone()
    finally:
        h._unload_ip_adapter()
    cos, err, ok = _tower_gate(got, want)
    record(f"[ip_adapter_plus] setup-plan Resampler Q {Q} B {B} n {n} {str(dtype)[6:]}: cosine {cos:.6f} max-abs {err:.4g} of "
           f"max|want| {float(want.abs().max()):.3g}")
    assert ok, (cos, err)


def test_resampler_scratch_leaves_the_zero_padding_of_the_text_v_transposed_alone():
    """At the ip-adapter-plus_sd15 sizes the Resampler's W2 GEMM (K = 3072, 128 rows at batch 8) runs split-K: its workspace sits
    on top of the arena while the setup plan is built.  The V^T buffers allocated behind it count on the arena's zeros in their
    pad columns (77 keys in rows of 80: the attention multiplies them by a zero probability), so they must not land on that
    scratch: after two calls the pad columns are still zero and the output is finite."""
    dtype = torch.bfloat16
    o, h = _tiny_pair(dtype)
    sizes = dict(Q=16, dim=768, E=1280, depth=4, heads=12, ff=3072)
    sd = PC.plus_state_dict(o, 77, **sizes)
    g = torch.Generator().manual_seed(3)
    B, S = 8, 10
    x, ehs = torch.randn(B, 4, 8, 8, generator=g), torch.randn(B, 77, 768, generator=g)
    h._load_ip_adapter_weights(sd)
    try:
        for k in range(2):
            emb = torch.randn(B, 1, S, sizes["E"], generator=g)
            out = h(x.to(DEV), torch.tensor(500), ehs.to(DEV), added_cond_kwargs={"image_embeds": [emb.to(DEV)]},
                    return_dict=False)[0]
        torch.cuda.synchronize()
        n_res = 10 * sizes["depth"] + 3
        gemms = [c[1][0]._obj for c in h.rt.setup_plan.calls[:n_res] if c[2] == "linear"]
        assert any(a.workspace for a in gemms), "no Resampler GEMM runs split-K any more: the test has lost its subject"
        assert bool(torch.isfinite(out).all())
        for pre, (k_, c, vt, ldvt) in h.net.kv.items():
            assert ldvt == 80
            pad = h.rt.arena.view(vt, (B * c, ldvt), dtype)[:, 77:]
            assert bool((pad == 0).all()), pre
    finally:
        h._unload_ip_adapter()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kinds", [("plus",), ("base", "plus")], ids=["plus", "base+plus"])
def test_unet_with_a_plus_adapter_against_the_oracle(kinds, dtype):
    """The tiny UNet at 8x8 latents with one Plus adapter, and with a base adapter and a Plus adapter of two images (32 tokens),
    against the oracle UNet with IPAttention behind the restated projections at the project's network gates; the adapter-free
    HIP output must FAIL the same gate, and the unloaded UNet is the one that never had an adapter, bit for bit."""
    o, h = _tiny_pair(dtype)
    scales = [1.0] if len(kinds) == 1 else [0.7, 0.4]
    sds = [PC.plus_state_dict(o, 60 + i, std=1.0, **PC.FIX) if k == "plus" else IC.adapter_state_dict(o, 60 + i, std=1.0)
           for i, k in enumerate(kinds)]
    import copy
    ipu = PC.PlusIPUNet(copy.deepcopy(o), sds, scales).eval()
    g = torch.Generator().manual_seed(len(kinds))
    B = 2
    x, ehs = torch.randn(B, 4, 8, 8, generator=g), torch.randn(B, 77, 768, generator=g)
    embeds = [torch.randn(B, 2, PC.FIX_S, PC.FIX["E"], generator=g) if k == "plus" and len(kinds) > 1 else
              torch.randn(B, 1, PC.FIX_S, PC.FIX["E"], generator=g) if k == "plus" else
              torch.randn(B, 1, IC.EMBED_DIM, generator=g) for k in kinds]
    t = torch.tensor(500)
    with torch.no_grad():
        ref = ipu(x, t, ehs, added_cond_kwargs={"image_embeds": embeds})[0]
    plain = h(x.to(DEV), t, ehs.to(DEV), return_dict=False)[0]
    h._load_ip_adapter_weights(sds)
    try:
        h.set_ip_adapter_scale(scales)
        out = h(x.to(DEV), t, ehs.to(DEV), added_cond_kwargs={"image_embeds": [e.to(DEV) for e in embeds]}, return_dict=False)[0]
        names = [c[2] for c in h.rt.step_plan.calls]
        assert names.count("ip_attn_add") == 4 * len(kinds) and "xattn_block" not in names and "perceiver_attn" not in names
        assert sorted({c[1][9] for c in h.rt.step_plan.calls if c[2] == "ip_attn_add"}) == ([16] if len(kinds) == 1 else [4, 32])
    finally:
        h._unload_ip_adapter()
    cos, err, ok = IC.net_gate(out, ref, dtype)
    pcos, perr, pok = IC.net_gate(plain, ref, dtype)
    record(f"[ip_adapter_plus] tiny UNet 8x8 {'+'.join(kinds)} {str(dtype)[6:]}: cosine {cos:.6f} max-abs {err:.4g} (max|ref| "
           f"{float(ref.abs().max()):.3g}); adapter-free output against it: cosine {pcos:.6f} max-abs {perr:.4g}")
    assert ok, (cos, err)
    assert not pok, "the adapter-free output passes the gate: the test would not notice a missing adapter"
    again = h(x.to(DEV), t, ehs.to(DEV), return_dict=False)[0]
    assert torch.equal(again, plain)


# ------------------------------------------------------------------------------------------------------------ pipeline
_GOLD = None


def _fixture():
    global _GOLD
    if _GOLD is None:
        _GOLD = torch.load(os.path.join(HERE, "golden", "ref_ip_adapter_plus.pt"), weights_only=False)
    return _GOLD


def _pipeline(dtype, case=None, adapters=None, scales=None):
    """tests/test_ip_adapter_gpu.py's pipeline and caller, with the adapters of a Plus fixture case (or `adapters`) loaded."""
    import make_ref_lcm as ML
    from test_ip_adapter_gpu import _pipeline as base_pipeline
    pipe, call = base_pipeline(dtype, None)
    if case is not None or adapters is not None:
        u4 = ML.components("v2")[2]
        pipe.load_ip_adapter(adapters(u4) if adapters is not None else PC.case_adapters(u4, case))
        pipe.set_ip_adapter_scale(scales if scales is not None else PC.CASES[case]["scales"])
        if case is not None and PC.CASES[case]["encoder"]:
            pipe.image_encoder = PC.HiddenStateEncoder().eval().to(DEV)
    return pipe, call


def _against(out, gen, gold, what):
    cos, err, ok = IC.loop_gate(out, gold["latents"])
    pcos, perr, pok = IC.loop_gate(gold["plain"], gold["latents"])
    record(f"[ip_adapter_plus] {what}: cosine {cos:.6f} max-abs {err:.4g} of max|ref| {float(gold['latents'].abs().max()):.4g} "
           f"(adapter-free reference latents: cosine {pcos:.5f}, {perr:.3g})")
    assert torch.equal(torch.randn(4, generator=gen), gold["next_draw"]), f"{what}: the generator is not where the reference leaves it"
    assert not pok
    assert ok, (what, cos, err)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", list(PC.CASES))
def test_brushnet_pipeline_against_the_reference_call(case, dtype):
    pipe, call = _pipeline(dtype, case)
    out, g = call(PC.case_prompt(case), True)
    unet_names = [c[2] for c in pipe._loop.rt.step_plan.calls]
    setup_names = [c[2] for c in pipe._loop.rt.setup_plan.calls]
    n_x = len(pipe.unet.net._attn_specs())
    assert unet_names.count("ip_attn_add") == n_x * len(PC.CASES[case]["kinds"]) and "perceiver_attn" not in unet_names
    assert setup_names.count("perceiver_attn") == PC.FIX["depth"]
    gold = _fixture()[case]
    _against(out, g, gold, f"BrushNet pipeline, case {case}, graph, {str(dtype)[6:]}")
    if case == "plus_image":
        # zeros in place of the zero image's hidden states are another call: the output is on the truth's side
        d_truth = float((out - gold["latents"]).abs().max())
        d_zero = float((out - gold["latents_zero_negative"]).abs().max())
        assert d_truth < 0.5 * d_zero, (d_truth, d_zero)
    if dtype == torch.bfloat16:
        eager, g2 = call(PC.case_prompt(case), False)
        _against(eager, g2, gold, f"BrushNet pipeline, case {case}, eager, bf16")


def test_second_call_with_other_embeds_matches_its_own_reference():
    pipe, call = _pipeline(torch.bfloat16, "plus")
    out, g = call(PC.case_prompt("plus", 0))
    _against(out, g, _fixture()["plus"], "per-call state, first call")
    out2, g2 = call(PC.case_prompt("plus", 1))
    _against(out2, g2, _fixture()["plus_b"], "per-call state, second call (other embeds)")
    assert not IC.loop_gate(out2, _fixture()["plus"]["latents"])[2]


def test_scale_zero_on_the_plus_adapter_is_the_base_adapter_alone():
    """Case `mixed` with the Plus adapter's scale at 0: the result of the base adapter alone at its 0.7, bit for bit."""
    pipe, call = _pipeline(torch.bfloat16, "mixed")
    prompt = PC.case_prompt("mixed")
    full, _ = call(prompt)
    pipe.set_ip_adapter_scale([0.7, 0.0])
    base_only, _ = call(prompt)
    pipe2, call2 = _pipeline(torch.bfloat16, adapters=lambda u4: PC.case_adapters(u4, "mixed")[:1], scales=[0.7])
    want, _ = call2(dict(ip_adapter_image_embeds=prompt["ip_adapter_image_embeds"][:1]))
    assert torch.equal(base_only, want) and not torch.equal(full, base_only)


def test_image_prompt_from_pixels_through_the_hip_tower_is_the_embeds_call():
    """`ip_adapter_image=<pixel tensor>` through the HIP CLIP vision tower equals, bit for bit, the call with
    `ip_adapter_image_embeds` built by hand from the tower's hidden_states[-2] of the image and of zeros; the host-side
    projection module is never evaluated on the way."""
    import vit_cases as VC
    cfg = dict(VC.TINY)
    S = (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1
    sizes = dict(PC.FIX, E=cfg["hidden_size"])
    pipe, call = _pipeline(torch.bfloat16, adapters=lambda u4: [PC.plus_state_dict(u4, 31, **sizes)], scales=[1.0])
    hf = VC.hf_vision(seed=11, **cfg)
    enc = PM.CLIPVisionModelWithProjection(device=DEV, **cfg)
    enc.load_state_dict(hf.state_dict())
    pipe.image_encoder = enc

    def no_host_projection(*a, **k):
        raise AssertionError("the host-side image projection ran on the call path")

    pipe.unet.encoder_hid_proj.forward = no_host_projection
    img = torch.randn(1, 3, cfg["image_size"], cfg["image_size"], generator=torch.Generator().manual_seed(8))
    out_img, _ = call(dict(ip_adapter_image=img))
    assert "vit_embed_ln" in [c[2] for c in enc._rt.plan.calls]
    assert "perceiver_attn" in [c[2] for c in pipe._loop.rt.setup_plan.calls]
    pos = enc(img.to(DEV), output_hidden_states=True).hidden_states[-2].clone()
    neg = enc(torch.zeros_like(img).to(DEV), output_hidden_states=True).hidden_states[-2].clone()
    assert pos.shape == (1, S, cfg["hidden_size"]) and float(neg.abs().max()) > 0 and not torch.equal(pos, neg)
    with torch.no_grad():
        want = hf(pixel_values=img, output_hidden_states=True).hidden_states[-2]
    cos, err, ok = _tower_gate(pos, want)
    assert ok, (cos, err)
    out_emb, _ = call(dict(ip_adapter_image_embeds=[torch.stack([neg, pos])]))
    assert torch.equal(out_img, out_emb)
    pipe.unload_ip_adapter()
    out_plain, _ = call()
    assert bool(torch.isfinite(out_img).all()) and not torch.equal(out_img, out_plain)
