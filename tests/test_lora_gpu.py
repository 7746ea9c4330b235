"""GPU: LoRA adapters merged into the packed weights on the device (pp_lora_merge, SDNet.repack, the models' and pipelines'
adapter surface).

References: float64 torch for the merge itself (W + sum c U D, the permutation functions of engine.py for the layouts),
oracle/sd_modules.py loaded with the float64-merged weights for the networks.  The adapter key conventions are restated
from the published form of diffusers / PEFT and kohya-ss files: neither library is importable here, so they are NOT
pinned against the libraries (as for the other unpinned parts, tests/golden/README.md); the adapters are generated from
seeds and go through `.safetensors` files in tmp_path.

Elementwise bound of the fp32 merge: (R + 3) * 2^-24 * (|W| + sum |c_a| |U_a| |D_a|) * |gamma|, R the summed rank -- the
standard bound of an fp32 dot product of that length; side vectors (K + R + 3) * 2^-24 * sum_k |term_k|.
"""
import copy
import ctypes as C
import hashlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lora_cases import diffusers_keys, kohya_keys, make_factors, merged_weights_f64  # noqa: E402
from test_models_gpu import TINY, close, gen  # noqa: E402

from oracle import loops as OL  # noqa: E402
from oracle import schedulers as OS  # noqa: E402
from oracle import sd_modules as OM  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import engine as E  # noqa: E402
from powerpaint_amd import models as PM  # noqa: E402
from powerpaint_amd import pipelines as PP  # noqa: E402
from powerpaint_amd import schedulers as PS  # noqa: E402
from powerpaint_amd.lora import LoraAdapter, read_lora, unet_targets  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24
RANKS = (1, 4, 7, 16, 64, 128)
T16 = {torch.bfloat16: L.PP_DT_BF16, torch.float16: L.PP_DT_F16}


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ the kernel
def run_merge(W, ads, out_dtype, lay, gamma=None, beta=None, badd=None, mapped=True, sides=False):
    """One pp_lora_merge call.  W [N][K] fp32 (source order); ads [(U, D, c)]; lay: the layout (dict).  mapped=False: plain
    row / column order at offset 0 into an [N][K] destination.  -> (destination matrix incl. what surrounds the block,
    colsum, bias)."""
    N, K = W.shape
    a = L.PPLoraMergeArgs()
    a.N, a.K, a.w, a.ldw, a.n_adapters = N, K, W.data_ptr(), K, len(ads)
    for i, (U, D, c) in enumerate(ads):
        a.rank[i], a.coef[i], a.up[i], a.down[i] = D.shape[0], c, U.data_ptr(), D.data_ptr()
    ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    a.gamma, a.beta, a.badd = ptr(gamma), ptr(beta), ptr(badd)
    if mapped:
        rows, cols = lay["out_rows"], lay["out_cols"]
        a.row_mode = L.PP_LORA_ROWS_GEGLU if lay.get("rows") == "geglu" else L.PP_LORA_ROWS_PLAIN
        a.col_mode = {"plain": 0, "igemm": 1, "kperm": 2, "kperm_geglu": 3}[lay.get("cols", "plain")]
        a.row_off, a.col_off, a.taps, a.cin_pad = lay.get("row_off", 0), lay.get("col_off", 0), lay.get("taps", 0), lay.get("cin_pad", 0)
    else:
        rows, cols = N, K
    tdt = torch.float32 if out_dtype == L.PP_DT_F32 else {v: k for k, v in T16.items()}[out_dtype]
    out = torch.full((rows, cols), 7.0, dtype=tdt, device=DEV)           # (7.0: what must survive around the block)
    a.out, a.ldo, a.out_rows, a.out_cols, a.out_dtype = out.data_ptr(), cols, rows, cols, out_dtype
    cs = bi = None
    if sides:
        cs = torch.full((rows,), float("nan"), device=DEV)
        bi = torch.full((rows,), float("nan"), device=DEV)
        a.colsum, a.bias = cs.data_ptr(), bi.data_ptr()
    L.check(L.lib().pp_lora_merge(C.byref(a), _stream()), "pp_lora_merge")
    torch.cuda.synchronize()
    return out, cs, bi


def host_place(X, lay, fill=7.0):
    """A plain-order [N][K] matrix moved to its place in the destination by the permutation functions of engine.py."""
    N, K = X.shape
    cols = lay.get("cols", "plain")
    if cols == "igemm":
        t = lay["taps"]
        k = int(round(t ** 0.5))
        Y = E._conv_igemm_cpad(X.reshape(N, K // t, k, k), lay["cin_pad"])
    elif cols == "kperm":
        Y = E._kperm(X)
    elif cols == "kperm_geglu":
        Y = E._kperm_geglu(X)
    else:
        Y = X
    if lay.get("rows") == "geglu":
        Y = E._geglu_interleave(Y)
    out = torch.full((lay["out_rows"], lay["out_cols"]), fill, dtype=X.dtype, device=X.device)
    r0, c0 = lay.get("row_off", 0), lay.get("col_off", 0)
    out[r0:r0 + N, c0:c0 + Y.shape[1]] = Y
    return out


def host_rows(v, lay, fill=float("nan")):
    y = E._geglu_interleave(v) if lay.get("rows") == "geglu" else v
    out = torch.full((lay["out_rows"],), fill, dtype=v.dtype, device=v.device)
    out[lay.get("row_off", 0):lay.get("row_off", 0) + v.shape[0]] = y
    return out


# every row / column order and block offset of the packing table, on shapes of the real SD-1.5 table
LAYOUTS = [
    dict(id="to_q_320", N=320, K=320, out_rows=320, out_cols=320),
    dict(id="attn2_kv_rowblock", N=320, K=768, row_off=320, out_rows=640, out_cols=768),
    dict(id="temb_all_rowblock", N=640, K=1280, row_off=960, out_rows=2240, out_cols=1280),
    dict(id="ff1_geglu_2560x320", N=2560, K=320, rows="geglu", out_rows=2560, out_cols=320, sides=True),
    dict(id="qkv_fold_rowblock", N=320, K=320, row_off=640, out_rows=960, out_cols=320, sides=True),
    dict(id="qkv_kperm", N=320, K=320, cols="kperm", row_off=320, out_rows=960, out_cols=320),
    dict(id="conv_1280x11520", N=1280, K=11520, cols="igemm", taps=9, cin_pad=1280, out_rows=1280, out_cols=11520),
    dict(id="conv2_with_k_tail", N=640, K=5760, cols="igemm", taps=9, cin_pad=640, out_rows=640, out_cols=5760 + 320),
    dict(id="shortcut_k_tail", N=640, K=320, col_off=5760, out_rows=640, out_cols=5760 + 320),
    dict(id="conv_in_9ch_padded", N=320, K=81, cols="igemm", taps=9, cin_pad=64, out_rows=320, out_cols=576),
    dict(id="conv_in_4ch_padded", N=320, K=36, cols="igemm", taps=9, cin_pad=64, out_rows=320, out_cols=576),
    dict(id="ff2_proj_out_kperm_geglu", N=320, K=1280, cols="kperm_geglu", out_rows=320, out_cols=1600),
    dict(id="ff2_proj_out_tail", N=320, K=320, col_off=1280, out_rows=320, out_cols=1600),
    dict(id="proj_out_1x1_1280", N=1280, K=1280, out_rows=1280, out_cols=1280),
]


def _case(lay, rank, n_ad, with_gamma, seed):
    g = torch.Generator("cpu").manual_seed(seed)
    N, K = lay["N"], lay["K"]
    W = (torch.randn(N, K, generator=g) * K ** -0.5).to(DEV)
    ranks = [rank, (rank + 1) // 2, 1][:n_ad]
    ads = []
    for i, r in enumerate(ranks):
        U = (torch.randn(N, r, generator=g) * 0.3).to(DEV)
        D = (torch.randn(r, K, generator=g) * K ** -0.5).to(DEV)
        ads.append((U, D, (0.75, -0.5, 1.25)[i]))      # (exact in fp32)
    gamma = (1.0 + 0.3 * torch.randn(K, generator=g)).to(DEV) if with_gamma else None
    beta = (0.2 * torch.randn(K, generator=g)).to(DEV)
    badd = (0.1 * torch.randn(N, generator=g)).to(DEV)
    Wd = W.double()
    ref, base = Wd.clone(), Wd.abs()
    for U, D, c in ads:
        ref += c * (U.double() @ D.double())
        base += abs(c) * (U.double().abs() @ D.double().abs())
    return W, ads, gamma, beta, badd, ref, base, sum(ranks)


@pytest.mark.parametrize("lay", LAYOUTS, ids=[l["id"] for l in LAYOUTS])
def test_merge_kernel_fp32_and_16bit(lay):
    """Checks 4 and 5: the fp32 destination against float64 within the dot-product bound; every layout bitwise equal to the
    plain result moved by the host permutation functions; the 16-bit destinations bitwise round16 of the fp32 result; the
    side vectors within their bounds (colsum against the float64 sum of the ROUNDED values)."""
    N, K = lay["N"], lay["K"]
    sides = bool(lay.get("sides"))
    worst = 0.0
    for rank in RANKS:
        for n_ad in (1, 3):
            for with_gamma in (False, True):
                W, ads, gamma, beta, badd, ref, base, R = _case(lay, rank, n_ad, with_gamma, seed=rank * 10 + n_ad)
                what = f"{lay['id']} rank {rank} x{n_ad} gamma={with_gamma}"
                gd = gamma.double() if with_gamma else torch.ones(K, dtype=torch.float64, device=DEV)
                kw = dict(gamma=gamma, beta=beta if sides else None, badd=badd if sides else None, sides=sides)
                plain, cs, bi = run_merge(W, ads, L.PP_DT_F32, lay, mapped=False, **kw)
                bound = (R + 3) * EPS * base * gd.abs()[None, :]
                err = (plain.double() - ref * gd[None, :]).abs()
                worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
                assert (err <= bound).all(), f"{what}: fp32 result outside the dot-product bound ({worst:.3f} of it)"
                if sides:
                    sb = (K + R + 3) * EPS * (base * gd.abs()[None, :]).sum(1)
                    assert ((cs.double() - (ref * gd[None, :]).sum(1)).abs() <= sb).all(), f"{what}: fp32 colsum"
                    bb = (K + R + 3) * EPS * ((base * beta.double().abs()[None, :]).sum(1) + badd.double().abs())
                    assert ((bi.double() - ((ref * beta.double()[None, :]).sum(1) + badd.double())).abs() <= bb).all(), f"{what}: bias"
                mapped, cs_m, bi_m = run_merge(W, ads, L.PP_DT_F32, lay, **kw)
                assert torch.equal(mapped, host_place(plain, lay)), f"{what}: fp32 layout differs from the host permutation"
                if sides:
                    assert torch.equal(torch.nan_to_num(cs_m, nan=-1.0), torch.nan_to_num(host_rows(cs, lay), nan=-1.0)), f"{what}: colsum row order"
                    assert torch.equal(torch.nan_to_num(bi_m, nan=-1.0), torch.nan_to_num(host_rows(bi, lay), nan=-1.0)), f"{what}: bias row order"
                for dt, code in T16.items():
                    out16, cs16, _ = run_merge(W, ads, code, lay, **kw)
                    want = host_place(plain.to(dt), lay, fill=7.0)
                    assert torch.equal(out16.view(torch.int16), want.view(torch.int16)), f"{what}: {dt} is not round16 of the fp32 result"
                    if sides:
                        v = plain.to(dt).double()
                        cb = K * EPS * v.abs().sum(1)
                        got = cs16[lay.get("row_off", 0):lay.get("row_off", 0) + N].double()
                        wantcs = host_rows(v.sum(1), lay)[lay.get("row_off", 0):lay.get("row_off", 0) + N]
                        assert ((got - wantcs).abs() <= host_rows(cb, lay)[lay.get("row_off", 0):lay.get("row_off", 0) + N]).all(), \
                            f"{what}: {dt} colsum is not the sum of the rounded values"
    print(f"{lay['id']}: worst fp32 error {worst:.3f} of the bound")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_colsum_is_of_the_rounded_values(dt):
    """A case where the sum of the fp32 values and the sum of the rounded values differ by far more than the colsum bound:
    every value sits a little above a 16-bit grid point, so every rounding error has the same sign."""
    N, K = 64, 320
    g = torch.Generator("cpu").manual_seed(3)
    W = (1.0 + 2.0 ** -13 * (1.0 + torch.rand(N, K, generator=g))).to(DEV)
    lay = dict(N=N, K=K, out_rows=N, out_cols=K)
    out, cs, _ = run_merge(W, [], T16[dt], lay, beta=torch.zeros(K, device=DEV), sides=True)
    v = out.double()
    bound = K * EPS * v.abs().sum(1)
    assert ((W.double().sum(1) - v.sum(1)).abs() > 4 * bound).all()          # the two candidates are far apart
    assert ((cs.double() - v.sum(1)).abs() <= bound).all()


# ------------------------------------------------------------------------------------------------ networks (built once)
_NETS = {}


def tiny(cin, dt):
    """(oracle with seed-0 weights rounded to bf16 as in test_models_gpu.make_tiny, HIP model, state dict)."""
    key = (cin, dt)
    if key not in _NETS:
        torch.manual_seed(0)
        o = OM.UNet2DConditionModel(in_channels=cin, **TINY)
        with torch.no_grad():
            for p in o.parameters():
                if p.dim() >= 2:
                    p.copy_(p.to(torch.bfloat16).float())
        o.eval()
        sd = {k: v.detach().clone() for k, v in o.state_dict().items()}
        h = PM.UNet2DConditionModel(in_channels=cin, device=DEV, dtype=dt, **TINY).load_state_dict(sd, keep_state_dict=True)
        _NETS[key] = (o, h, sd)
    return _NETS[key]


def digest(h):
    torch.cuda.synchronize()
    return hashlib.sha256(h.param_buffer().cpu().numpy().tobytes()).hexdigest()


def oracle_with(o, sd, adapters, scale=1.0):
    m = copy.deepcopy(o)
    w = {k: v.float() for k, v in merged_weights_f64(sd, adapters, scale).items()}
    m.load_state_dict({**sd, **w})
    return m.eval()


def write_adapter(tmp_path, name, fac, style="peft"):
    from safetensors.torch import save_file
    f = os.path.join(str(tmp_path), name + ".safetensors")
    ad = LoraAdapter(unet=fac)
    save_file({k: v.contiguous() for k, v in (kohya_keys(ad) if style == "kohya" else diffusers_keys(ad, style)).items()}, f)
    return f


def matters(ref, ref0, what, rel=3e-2, loop_cos_min=None):
    """The adapter moves the ORACLE by far more than the gate allows: a merge that does nothing cannot pass.
    Network forwards: cosine <= 0.99 and max-abs >= 3 x the gate's bound.  Free-running loops (loop_cos_min: the cosine gate
    of the loop tests, the tight one of the two there): a result within the gate of the adapter-less oracle is at most
    acos(loop_cos_min) away from it, so it fails the gate against the adapted oracle as soon as the two oracles are more
    than twice that angle apart; asked for here: three times."""
    import math
    cos = torch.nn.functional.cosine_similarity(ref.flatten(), ref0.flatten(), dim=0).item()
    d = (ref - ref0).abs().max().item()
    bound = rel * max(1.0, ref.abs().max().item())
    print(f"{what}: oracle with against without the adapter: cosine {cos:.4f}, max-abs {d:.3f} (gate bound {bound:.3f})")
    if loop_cos_min is not None:
        assert math.acos(min(1.0, cos)) >= 3 * math.acos(loop_cos_min), \
            f"{what}: the adapter is too weak to be seen (cosine {cos:.5f} between the two oracles)"
        return
    assert cos <= 0.99 and d >= 3 * bound, f"{what}: the adapter is too weak to be seen (cosine {cos:.5f}, max-abs {d:.4g})"


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_repack_without_adapters_reproduces_the_loaded_buffer(dt):
    """Check 6 on the TINY network (every kind of entry occurs in it: row blocks, GEGLU rows, both K permutations, the padded
    conv_in, conv2 with its K tail, the composed ff2_proj_out family)."""
    o, h, sd = tiny(9, dt)
    net, pk = h.net, h.net.params
    before = {n: pk.tensor(n).clone() for n in pk.offsets}
    targets = unet_targets(net)
    recipes = net.recipes_of(targets)
    assert {r.name for r in recipes} == {n for n, (_, d) in pk.shapes.items() if d == dt}
    for r in recipes:                                   # what is about to be rebuilt is wiped first
        for e in (r.name, r.colsum, r.bias):
            if e:
                pk.tensor(e).view(torch.uint8).fill_(0xFF)
    src = {k: v.to(DEV, torch.float32).contiguous() for k, v in sd.items()}
    comp = {}
    v0 = pk.version
    net.repack(list(targets), {}, src, _stream(), composed_out=comp)
    torch.cuda.synchronize()
    assert pk.version == v0 + 1
    for r in recipes:
        got, want = pk.tensor(r.name), before[r.name]
        if r.compose:
            t1, prod = comp[r.name]
            w_po, w_f2 = src[r.rows[0] + ".weight"].reshape(t1.shape).double(), src[r.compose + ".weight"].double()
            Cc = w_po.shape[0]
            assert torch.equal(t1, w_po.float())
            assert ((prod.double() - w_po @ w_f2).abs() <= (4 * Cc + 3) * EPS * (w_po.abs() @ w_f2.abs())).all(), r.name
            p16 = prod.to(dt)
            if r.cols == "kperm_geglu":
                p16 = E._kperm_geglu(p16)
            assert torch.equal(got.view(torch.int16), torch.cat([p16, t1.to(dt)], 1).view(torch.int16)), r.name
            if r.bias:
                b = w_po @ src[r.compose + ".bias"].double() + src[r.badd].double()
                bb = (Cc + 3) * EPS * ((w_po.abs() @ src[r.compose + ".bias"].double().abs()) + src[r.badd].double().abs())
                assert ((pk.tensor(r.bias).double() - b).abs() <= bb).all(), r.bias
            continue
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{r.name}: repack differs from load_state_dict"
        if r.colsum:
            ws = [src[m + ".weight"].double() for m in r.rows]
            w = torch.cat(ws, 0)
            gm, bt = src[r.gamma + ".weight"].double(), src[r.gamma + ".bias"].double()
            K = w.shape[1]
            v = (w.float() * gm.float()[None, :]).to(dt).double()
            cs, cb = v.sum(1), K * EPS * v.abs().sum(1)
            bi = w @ bt + (src[r.badd].double() if r.badd else 0.0)
            bb = (K + 3) * EPS * ((w.abs() @ bt.abs()) + (src[r.badd].double().abs() if r.badd else 0.0))
            if r.row_order == "geglu":
                cs, cb, bi, bb = (E._geglu_interleave(x) for x in (cs, cb, bi, bb))
            assert ((pk.tensor(r.colsum).double() - cs).abs() <= cb).all(), r.colsum
            assert ((pk.tensor(r.bias).double() - bi).abs() <= bb).all(), r.bias
    # fp32 entries that are not side vectors are not touched at all
    sidev = {e for r in recipes for e in (r.colsum, r.bias) if e}
    for n, (_, d) in pk.shapes.items():
        if d == torch.float32 and n not in sidev:
            assert torch.equal(pk.tensor(n), before[n]), n
    for n, t in before.items():                         # leave the shared model as it was loaded
        pk.tensor(n).copy_(t)
    h.params_changed()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("cin", [9, 4])
def test_tiny_unet_parity_with_adapters(cin, dt, tmp_path):
    """Check 7: an adapter over ALL target kinds (convs included), rank 8, rms(delta) = 0.1 rms(W): (a) scale 1, (b) scale 0.6
    through cross_attention_kwargs, (c) two adapters with weights (1.0, -0.5)."""
    o, h, sd = tiny(cin, dt)
    targets = unet_targets(h.net)
    f1 = make_factors(targets, sd, 8, seed=11)
    f2 = make_factors(targets, sd, 8, seed=12)
    a1 = read_lora(write_adapter(tmp_path, "a1", f1, "peft"), unet_modules=targets, text_modules={})
    a2 = read_lora(write_adapter(tmp_path, "a2", f2, "kohya"), unet_modules=targets, text_modules={})
    x, e = gen(2, cin, 16, 16, seed=1), gen(2, 77, 768, seed=2)
    with torch.no_grad():
        ref0 = o(x, 500, e)[0]
    d0 = digest(h)
    try:
        h.load_lora_adapter(a1, "a1")
        assert h.active_adapters() == ["a1"]
        for what, ads, scale, kw in (("a: s = 1", [(f1, 1.0)], 1.0, {}),
                                     ("b: s = 0.6", [(f1, 1.0)], 0.6, {"cross_attention_kwargs": {"scale": 0.6}}),
                                     ("c: two adapters (1.0, -0.5)", [(f1, 1.0), (f2, -0.5)], 1.0, {})):
            if len(ads) == 2:
                h.load_lora_adapter(a2, "a2")
                h.set_adapters(["a1", "a2"], [1.0, -0.5])
            with torch.no_grad():
                ref = oracle_with(o, sd, ads, scale)(x, 500, e)[0]
            tag = f"lora tiny unet cin {cin} {dt} ({what})"
            matters(ref, ref0, tag)
            out = h(x.to(DEV), 500, e.to(DEV), return_dict=False, **kw)[0]
            close(out, ref, tag)
    finally:
        h.delete_adapters(h.list_adapters())
    assert digest(h) == d0
    close(h(x.to(DEV), 500, e.to(DEV), return_dict=False)[0], ref0, "lora tiny unet: adapters gone")


def test_set_adapters_keeps_plan_and_graph():
    """Check 9: new adapter weights reach a captured step without a new plan or graph; the hoisted cross-attention K / V are
    refreshed although the encoder_hidden_states tensor object is the same."""
    o, h, sd = tiny(9, torch.bfloat16)
    targets = unet_targets(h.net)
    fac = make_factors(targets, sd, 8, seed=21)
    x, e = gen(2, 9, 16, 16, seed=1).to(DEV), gen(2, 77, 768, seed=2).to(DEV)
    never = PM.UNet2DConditionModel(in_channels=9, device=DEV, **TINY).load_state_dict(sd)
    never.prepare(tuple(x.shape), e)

    def step():
        rt = h.prepare(tuple(x.shape), e)
        rt.load_input([(x, 0)])
        rt.set_timestep(500)
        rt.run_step(use_graph=True)
        return rt, rt.eps_tensor().float().cpu()

    try:
        h.load_lora_adapter(fac, "a")
        h.merge_adapters(1.0)
        rt, out1 = step()
        plan, graph, ncalls = rt.step_plan, rt.graph, len(rt.step_plan.calls)
        assert graph is not None
        with torch.no_grad():
            close(out1, oracle_with(o, sd, [(fac, 1.0)])(x.cpu(), 500, e.cpu())[0], "lora captured step, weight 1.0")
        h.set_adapters(["a"], [-0.7])
        h.merge_adapters(1.0)
        rt2, out2 = step()
        assert rt2 is rt and rt.step_plan is plan and rt.graph is graph and len(rt.step_plan.calls) == ncalls
        assert ncalls == len(never.rt.step_plan.calls)
        with torch.no_grad():
            ref2 = oracle_with(o, sd, [(fac, -0.7)])(x.cpu(), 500, e.cpu())[0]
        close(out2, ref2, "lora captured step, weight -0.7 (same plan, same graph)")
        assert not torch.equal(out1, out2)
    finally:
        h.delete_adapters(h.list_adapters())


def test_round_trip_restores_the_buffer(tmp_path):
    """Check 10."""
    o, h, sd = tiny(4, torch.bfloat16)
    targets = unet_targets(h.net)
    fac = make_factors(targets, sd, 8, seed=31)
    f = write_adapter(tmp_path, "rt", fac, "old")
    pipe = PP.StableDiffusionInpaintPipeline(unet=h, scheduler=PS.DDIMScheduler())
    d0 = digest(h)
    pipe.load_lora_weights(f, adapter_name="rt")
    h.merge_adapters(1.0)
    d1 = digest(h)
    assert d1 != d0
    for w, s in ((0.5, 1.0), (1.0, 0.3), (-1.0, 0.8)):
        pipe.set_adapters(["rt"], [w])
        h.merge_adapters(s)
        assert digest(h) not in (d0, d1)
    pipe.unload_lora_weights()
    assert digest(h) == d0 and pipe.get_active_adapters() == [] and pipe.get_list_adapters() == {}
    pipe.load_lora_weights(f, adapter_name="rt")
    h.merge_adapters(1.0)
    assert digest(h) == d1, "the same adapter merged again gives other bytes"
    pipe.set_adapters(["rt"], [0.25])
    h.merge_adapters(1.0)
    pipe.delete_adapters("rt")                          # the last adapter goes: back to the loaded bytes
    assert digest(h) == d0


def test_an_adapter_swapped_under_a_kept_name_is_merged_anew(tmp_path):
    """`delete_adapters("style")` then `load_lora_weights(other file, adapter_name="style")` while another adapter stays
    active: the merged state is keyed on the LOAD, not on the name, so the new file reaches the weights (same digest as a
    model that only ever saw the new pair) and the old one leaves them."""
    o, h, sd = tiny(4, torch.bfloat16)
    targets = unet_targets(h.net)
    fb, fa1, fa2 = (make_factors(targets, sd, 8, seed=s) for s in (61, 62, 63))
    pipe = PP.StableDiffusionInpaintPipeline(unet=h, scheduler=PS.DDIMScheduler())
    d0 = digest(h)
    try:
        pipe.load_lora_weights(write_adapter(tmp_path, "subject", fb), adapter_name="subject")
        pipe.load_lora_weights(write_adapter(tmp_path, "style1", fa1), adapter_name="style")
        pipe._merge_lora(None)
        d_old = digest(h)
        pipe.delete_adapters("style")
        pipe.load_lora_weights(write_adapter(tmp_path, "style2", fa2, "kohya"), adapter_name="style")
        assert pipe.get_active_adapters() == ["subject", "style"]
        pipe._merge_lora(None)
        d_new = digest(h)
        assert d_new != d_old, "the adapter loaded under the old name never reached the weights"
        pipe.unload_lora_weights()
        assert digest(h) == d0
        h.load_lora_adapter(fb, "subject")
        h.load_lora_adapter(fa2, "style")
        h.merge_adapters(1.0)
        assert digest(h) == d_new
        x, e = gen(2, 4, 16, 16, seed=1), gen(2, 77, 768, seed=2)
        with torch.no_grad():
            ref = oracle_with(o, sd, [(fb, 1.0), (fa2, 1.0)])(x, 500, e)[0]
        close(h(x.to(DEV), 500, e.to(DEV), return_dict=False)[0], ref, "lora tiny unet: adapter swapped under a kept name")
    finally:
        h.delete_adapters(h.list_adapters())
        pipe.__dict__.pop("_lora_names", None)
    assert digest(h) == d0


def test_merge_without_a_kept_state_dict_says_what_to_do():
    o, _, sd = tiny(4, torch.bfloat16)
    h = PM.UNet2DConditionModel(in_channels=4, device=DEV, **TINY).load_state_dict(sd)
    h.load_lora_adapter(make_factors(unet_targets(h.net), sd, 4, seed=71, modules=["conv_out"]), "a")
    with pytest.raises(L.PPError, match="keep_state_dict=True"):
        h.merge_adapters(1.0)


# ------------------------------------------------------------------------------------------------ pipelines
def _clip(tmp_path):
    import json
    import transformers
    from powerpaint_amd.utils import TokenizerWrapper
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_task_tokens.json")) as f:
        G = json.load(f)
    tok = TokenizerWrapper(tokenizer=transformers.CLIPTokenizer(
        vocab={t: i for i, t in enumerate(G["vocab"])}, merges=[tuple(m) for m in G["merges"]], model_max_length=77))
    torch.manual_seed(5)
    enc = PM.CLIPTextModel(device=DEV, vocab_size=G["n_base"], num_hidden_layers=2, eos_token_id=G["n_base"] - 1)
    with torch.no_grad():
        for p in enc.parameters():
            if p.dim() >= 2:
                p.mul_(2.0)
    return tok, enc


@pytest.mark.parametrize("kind", ["v1", "brushnet"])
def test_pipeline_with_unet_and_text_encoder_adapter(kind, tmp_path):
    """Check 11: 4 DDIM steps to latents with a UNet + text-encoder adapter at cross_attention_kwargs scale 0.7 against the
    oracle loop on merged weights.  The text tower has no oracle of its own in this suite: its merge is checked against
    float64 on the parameters, and the prompt embeddings the oracle loop is fed are the tower's own output for the merged
    weights (the tower itself is held to transformers in tests/test_clip.py)."""
    from safetensors.torch import save_file
    from powerpaint_amd.lora import text_targets
    tok, enc = _clip(tmp_path)
    cin = 9 if kind == "v1" else 4
    o, h, sd = tiny(cin, torch.bfloat16)
    targets, tt = unet_targets(h.net), text_targets(enc)
    assert len(tt) == 12
    tsd = {n + ".weight": m.weight.detach().float().cpu() for n, m in enc.named_modules() if n in tt}
    fu, ft = make_factors(targets, sd, 8, seed=41, rel=0.2), make_factors(tt, tsd, 4, seed=42, rel=0.3)
    ad = LoraAdapter(unet=fu, text_encoder=ft)
    f = os.path.join(str(tmp_path), "both.safetensors")
    save_file({k: v.contiguous() for k, v in kohya_keys(ad).items()}, f)
    B, hh, N, s = 2, 16, 4, 0.7
    lat = gen(B, 4, hh, hh, seed=0)
    mask = torch.zeros(B, 1, hh, hh)
    mask[:, :, 4:12, 4:12] = 1.0
    mil = gen(B, 4, hh, hh, seed=1, scale=0.5)
    prompts, negs = ["a photo of a cat", "the sea"], ["", ""]
    if kind == "v1":
        pipe = PP.StableDiffusionInpaintPipeline(unet=h, text_encoder=enc, tokenizer=tok, scheduler=PS.DDIMScheduler())
        kw = dict(promptA=prompts, promptB=prompts, negative_promptA=negs, negative_promptB=negs, height=hh * 8, width=hh * 8,
                  mask_latents=mask.to(DEV), masked_image_latents=mil.to(DEV))
    else:
        torch.manual_seed(0)
        ob = OM.randomize_zero_convs(OM.BrushNetModel(in_channels=4, conditioning_channels=5, **TINY))
        with torch.no_grad():
            for p in ob.parameters():
                if p.dim() >= 2:
                    p.copy_(p.to(torch.bfloat16).float())
        ob.eval()
        hb = PM.BrushNetModel(in_channels=4, conditioning_channels=5, device=DEV, **TINY).load_state_dict(ob.state_dict())
        cl = torch.cat([mil, mask], 1)
        pe_b = gen(2 * B, 77, 768, seed=2)
        pipe = PP.StableDiffusionPowerPaintBrushNetPipeline(unet=h, brushnet=hb, text_encoder=enc, tokenizer=tok,
                                                            text_encoder_brushnet=None, scheduler=PS.DDIMScheduler())
        kw = dict(prompt_embeds=pe_b[B:].to(DEV), negative_prompt_embeds=pe_b[:B].to(DEV), promptU=prompts,
                  negative_promptU=negs, conditioning_latents=cl.to(DEV))
    kw.update(num_inference_steps=N, guidance_scale=7.5, latents=lat.to(DEV), output_type="latent", return_dict=False)

    def emb(p):
        ids = tok(p, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
        return enc(ids.to(DEV))[0].float().cpu()

    def oracle_run(scale, pe):
        ou = oracle_with(o, sd, [(fu, 1.0)], scale)
        if kind == "v1":
            return OL.loop_v1(ou, OS.DDIMScheduler(), lat, torch.cat([mask] * 2), torch.cat([mil] * 2), pe, N, 7.5)
        return OL.loop_v2(ou, ob, OS.DDIMScheduler(), lat, torch.cat([cl] * 2), pe_b, pe, N, 7.5, 1.0)

    try:
        pe_plain = torch.cat([emb(negs), emb(prompts)])
        pipe.load_lora_weights(f, adapter_name="both")
        assert pipe.get_list_adapters() == {"unet": ["both"], "text_encoder": ["both"]}
        out = pipe(cross_attention_kwargs={"scale": s}, **kw)[0]
        # the tower's parameters are the float64 merge, rounded once
        mods = dict(enc.named_modules())
        for m, w in merged_weights_f64(tsd, [(ft, 1.0)], s).items():
            p = mods[m[:-len(".weight")]].weight
            assert ((p.detach().cpu().double() - w).abs() <= 2.0 ** -24 * w.abs() + 1e-30).all(), m    # one rounding to fp32
        pe = torch.cat([emb(negs), emb(prompts)])           # (the tower is at scale 0.7 now)
        assert (pe - pe_plain).abs().max().item() > 0.05, "the text-encoder adapter does not reach the embeddings"
        ref = oracle_run(s, pe)
        if kind == "v1":
            ref0 = OL.loop_v1(o, OS.DDIMScheduler(), lat, torch.cat([mask] * 2), torch.cat([mil] * 2), pe_plain, N, 7.5)
        else:
            ref0 = OL.loop_v2(o, ob, OS.DDIMScheduler(), lat, torch.cat([cl] * 2), pe_b, pe_plain, N, 7.5, 1.0)
        matters(ref, ref0, f"lora pipeline {kind}", rel=4.5e-2, loop_cos_min=0.9997)
        close(out, ref, f"lora pipeline {kind} free-running, scale {s}", cos_min=0.9997, rel=4.5e-2)
        # two scales, two results, one plan
        rt = h.rt
        plan = rt.step_plan
        out_b = pipe(cross_attention_kwargs={"scale": 0.2}, **kw)[0]
        assert rt.step_plan is plan and not torch.equal(out, out_b)
        pe_b2 = torch.cat([emb(negs), emb(prompts)])
        close(out_b, oracle_run(0.2, pe_b2), f"lora pipeline {kind} free-running, scale 0.2", cos_min=0.9997, rel=4.5e-2)
        again = pipe(cross_attention_kwargs={"scale": s}, **kw)[0]
        assert rt.step_plan is plan and torch.equal(again, out)
    finally:
        pipe.unload_lora_weights()


# ------------------------------------------------------------------------------------------------ full width
def test_full_sd15_unet_attention_adapter():
    """Check 8: SD-1.5 UNet, 64x64, batch 2, rank 16 on the attention projections only (the common file shape),
    rms(delta) = 0.5 rms(W); and check 6 once more at full width (zero adapters reproduce the 16-bit entries)."""
    torch.manual_seed(0)
    o = OM.UNet2DConditionModel(in_channels=4)
    with torch.no_grad():
        for p in o.parameters():
            if p.dim() >= 2:
                p.copy_(p.to(torch.bfloat16).float())
    o.eval()
    sd = {k: v.detach().clone() for k, v in o.state_dict().items()}
    h = PM.UNet2DConditionModel(in_channels=4, device=DEV).load_state_dict(sd, keep_state_dict=True)
    targets = unet_targets(h.net)
    attn = [m for m in targets if ".attn1." in m or ".attn2." in m]
    assert len(attn) == 16 * 8
    fac = make_factors(targets, sd, 16, seed=51, rel=0.5, modules=attn)
    x, e = gen(2, 4, 64, 64, seed=1), gen(2, 77, 768, seed=2)
    with torch.no_grad():
        ref0 = o(x, 500, e)[0]
        ref = oracle_with(o, sd, [(fac, 1.0)])(x, 500, e)[0]
    matters(ref, ref0, "lora full SD-1.5 unet")
    d0 = digest(h)
    h.load_lora_adapter(fac, "attn")
    out = h(x.to(DEV), 500, e.to(DEV), return_dict=False)[0]
    close(out, ref, "lora full SD-1.5 unet 64x64, rank 16 attention adapter")
    h.delete_adapters("attn")
    assert digest(h) == d0
    close(h(x.to(DEV), 500, e.to(DEV), return_dict=False)[0], ref0, "lora full SD-1.5 unet: adapter gone")
    # zero adapters, every target, full width
    pk = h.net.params
    recipes = h.net.recipes_of(targets)
    before = {r.name: pk.tensor(r.name).clone() for r in recipes}
    src = {k: v.to(DEV, torch.float32).contiguous() for k, v in sd.items()}
    h.net.repack(list(targets), {}, src, _stream())
    torch.cuda.synchronize()
    for r in recipes:
        if not r.compose:
            assert torch.equal(pk.tensor(r.name).view(torch.int16), before[r.name].view(torch.int16)), r.name
