"""-m gpu: every normalisation path against its fp64 reference under the derived gates of tests/norm_cases.py (derivations:
that module's docstring; proof that the gates notice a wrong kernel: tests/test_norm_probes.py), at the smallest shapes at
which each of its code paths exists, in bf16 and fp16, over the data regimes zero / offset16 / edge / constant / outlier /
tiny.

The only gates:  |out - ref| <= u |ref| + (1 + u) d   with d the propagated statistics, fp32 and SiLU terms of the path;
accumulators and row moments against the exact sums of the stored output within (adds) half quanta + the fp32 column sums.

Outputs of the norm kernels go into the middle of a sentinel-filled buffer (the kernels take no row stride, so the padding
lies in front of the first and behind the last row): every element outside the result is bit-for-bit unchanged after the
launch and the result is finite.

The worst error / gate per (path, format, regime) is printed, and profiles/norm_exact_achieved.txt is rewritten with them
when the whole module has run (every case has entered its figure before it asserts).
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import norm_cases as NC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import ops  # noqa: E402

DEV = "cuda"
SENTINEL = 0x5A5A
PAD = 64                     # 16-bit elements in front of and behind the result (keeps its 16-byte alignment)
WORST = {}


ACHIEVED_HEADER = ("# tests/test_norm_exact_gpu.py on one MI355X: the largest achieved error / gate per (path, format, regime or input).\n"
                   "# Gates: tests/norm_cases.py (derived, not fitted).  No ratio may exceed 1.\n")
ACHIEVED_KEYS = 82           # the (path, format, regime) keys of a whole run of this file


@pytest.fixture(scope="module", autouse=True)
def _achieved():
    """After a WHOLE run of the file profiles/norm_exact_achieved.txt is rewritten (never appended to): the figures are
    deterministic, so the tracked file stays as committed unless a kernel or a gate changed."""
    yield
    if len(WORST) != ACHIEVED_KEYS:
        return
    try:
        with open(os.path.join(ROOT, "profiles", "norm_exact_achieved.txt"), "w") as f:
            f.write(ACHIEVED_HEADER)
            for (path, fmt, regime), (r, where) in sorted(WORST.items()):
                f.write(f"[norm exact] {path} {fmt} {regime}: worst error / gate {r:.3f} at {where}\n")
    except OSError:
        pass


def _note(path, fmt, regime, ratio, where):
    print(f"[norm exact] {path} {fmt} {regime} {where}: error / gate {ratio:.3f}")
    if ratio > WORST.get((path, fmt, regime), (-1.0, None))[0]:
        WORST[(path, fmt, regime)] = (ratio, where)


def _guarded(shape, dtype, launch_into, what):
    """Run one launch into the middle of a sentinel-filled buffer; -> the result (a copy)."""
    n = 1
    for s in shape:
        n *= s
    full = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.int16, device=DEV)
    view = full[PAD:PAD + n].view(dtype).view(*shape)
    launch_into(view)
    torch.cuda.synchronize()
    out = view.clone()
    assert bool((full[:PAD] == SENTINEL).all()) and bool((full[PAD + n:] == SENTINEL).all()), \
        ("bytes outside the output were written", what)
    assert bool(torch.isfinite(out.float()).all()), ("non-finite output", what)
    return out


def _dev(t):
    return t.to(DEV) if t is not None else None


# ------------------------------------------------------------------------------------------------ GroupNorm
@pytest.mark.parametrize("path", ["stats", "acc"])
@pytest.mark.parametrize("shape", NC.GN_SHAPES, ids=lambda s: "c%d+%d_g%d_hw%d_b%d" % tuple(s))
def test_groupnorm_paths(shape, path):
    """path "stats": pp_groupnorm_stats + pp_groupnorm_apply; "acc": pp_groupnorm_apply_acc from accumulators rounded once
    from the exact sums (its contract, no producer).  What each shape reaches: NC.GN_SHAPES."""
    c1, c2, groups, hw, B = shape
    C = c1 + c2
    failures = []
    for dtype, fmt in NC.DTYPES:
        for regime in NC.gn_regimes(shape):
            k = NC.build_gn_case(shape, regime, dtype, path)
            x1, x2, gamma, beta = _dev(k["x1"]), _dev(k["x2"]), _dev(k["gamma"]), _dev(k["beta"])
            x1v = x1.view(B, hw, 1, c1)
            x2v = x2.view(B, hw, 1, c2) if x2 is not None else None
            acc = NC.build_acc(x1, x2, groups) if path == "acc" else None
            worst = 0.0
            for silu in (True, False):
                for eps in NC.gn_eps_list(regime, silu):
                    ref, gate = NC.gate_groupnorm(x1, x2, groups, gamma, beta, eps, silu, dtype, k["terms"], k["exact"])
                    assert bool(torch.isfinite(gate).all())

                    def go(o):
                        if path == "acc":
                            ops.groupnorm_apply_acc(x1v, acc, gamma, beta, eps, silu, groups=groups, x2=x2v, out=o)
                        else:
                            ops.groupnorm(x1v, gamma, beta, eps, silu, groups=groups, x2=x2v, out=o)

                    out = _guarded((B, hw, 1, C), dtype, go, (shape, path, fmt, regime, silu, eps))
                    worst = max(worst, NC.worst_ratio(out.view(B, hw, C), ref, gate))
            _note("groupnorm_" + path, fmt, regime, worst, "c%d+%d g%d hw%d" % (c1, c2, groups, hw))
            if not worst <= 1.0:
                failures.append((path, fmt, regime, worst))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("rows", NC.LN_ROWS)
@pytest.mark.parametrize("C", NC.LN_C)
def test_layernorm_kernel(C, rows):
    """C: one slot; 320; the S = 64 | 65, 128 | 129, 192 | 193 boundaries between the four instantiations; S = 256, the
    limit.  rows 1, 5, 7: the last block of four rows is ragged, the `row >= rows` guard fires."""
    failures = []
    for dtype, fmt in NC.DTYPES:
        for regime in NC.ln_regimes(C):
            k = NC.build_ln_case(C, rows, regime, dtype)
            x, gamma, beta = _dev(k["x"]), _dev(k["gamma"]), _dev(k["beta"])
            worst = 0.0
            for eps in ((1e-5, 1e-6) if regime == "constant" else (1e-5,)):
                ref, gate = NC.gate_layernorm(x, gamma, beta, eps, dtype, regime == "constant")
                out = _guarded((rows, C), dtype, lambda o: ops.layernorm(x, gamma, beta, eps, out=o), (C, rows, fmt, regime))
                worst = max(worst, NC.worst_ratio(out, ref, gate))
            _note("layernorm", fmt, regime, worst, f"C={C} rows={rows}")
            if not worst <= 1.0:
                failures.append((fmt, regime, worst))
    assert not failures, failures


def test_layernorm_refuses_more_than_2048_channels():
    x = torch.zeros(4, 2056, dtype=torch.bfloat16, device=DEV)
    g = torch.ones(2056, device=DEV)
    with pytest.raises(L.PPError, match="PP_ERR_UNSUPPORTED"):
        ops.layernorm(x, g, g)


# ------------------------------------------------------------------------------------------------ epilogue accumulators
def _acc_ratio(acc, out3, rpb, splitk, cg, c0, groups):
    S, Q, gS, gQ = NC.gate_epilogue_acc(out3, rpb, cg, c0, groups, NC.epilogue_block_rows(rpb, splitk))
    a = acc.double()
    return max(NC.worst_ratio(a[..., 0] / NC.SUM_SCALE, S, gS), NC.worst_ratio(a[..., 1] / NC.SQ_SCALE, Q, gQ))


@pytest.mark.parametrize("tile", NC.EPI_TILES)
@pytest.mark.parametrize("case", NC.EPI_CASES, ids=lambda c: c[0])
def test_gemm_epilogue_accumulators(case, tile):
    """rows_per_batch = 64: several batch items inside one 128- or 256-row tile (the batch index is per 64-row pass), an odd
    item count (the last tile is ragged in rows), a ragged last column tile (N 200), cg = 8 at a misaligned channel offset (21
    groups in one 160-column tile, GN_SLOTS = 24), two subscriptions, the split-K combine -- against the exact sums of the
    stored output.  A second run gives the same integers."""
    name, B, rpb, N, K, subs, splitk = case
    failures = []
    for dtype, fmt in NC.DTYPES:
        x, w, bias, res = (_dev(t) for t in NC.build_gemm_case(B * rpb, N, K, dtype))
        runs = []
        for _ in range(2):
            accs = [torch.zeros(B, groups, 2, dtype=torch.int64, device=DEV) for (_, _, groups) in subs]
            gn = [(a, cg, c0, groups) for a, (cg, c0, groups) in zip(accs, subs)]
            out = ops.gemm(x, w, bias=bias, res1=res, rows_per_batch=rpb, tile=tile, splitk=splitk, gn=gn)
            runs.append((out, accs))
        torch.cuda.synchronize()
        out, accs = runs[0]
        assert torch.equal(out, runs[1][0]) and all(torch.equal(a, b) for a, b in zip(accs, runs[1][1])), (name, tile, fmt)
        assert torch.equal(out, ops.gemm(x, w, bias=bias, res1=res, rows_per_batch=rpb, tile=tile, splitk=splitk)), (name, tile, fmt)
        worst = max(_acc_ratio(a, out.view(B, rpb, N), rpb, splitk, *sub) for a, sub in zip(accs, subs))
        _note("epilogue_acc_gemm", fmt, "gemm_output", worst, f"{name} tile={tile}")
        if not worst <= 1.0:
            failures.append((name, tile, fmt, worst))
    assert not failures, failures


@pytest.mark.parametrize("tile,splitk", [(0, 0), (53, 1), (31, 4)])
@pytest.mark.parametrize("B", [3, 5])
def test_conv_epilogue_accumulators_at_the_8x8_level(B, tile, splitk):
    H, Cin, Cout = 8, 320, 320
    subs = [(10, 0, 32), (20, 320, 32)]
    failures = []
    for dtype, fmt in NC.DTYPES:
        g = NC._gen(13, B, tile)
        x = torch.randn(B, H, H, Cin, generator=g).to(dtype).to(DEV)
        w = (torch.randn(Cout, 9 * Cin, generator=g) * (9 * Cin) ** -0.5).to(dtype).to(DEV)
        bias = torch.randn(Cout, generator=g).to(DEV)
        runs = []
        for _ in range(2):
            accs = [torch.zeros(B, groups, 2, dtype=torch.int64, device=DEV) for (_, _, groups) in subs]
            out = ops.conv3x3(x, w, bias, tile=tile, splitk=splitk, gn=[(a, *s) for a, s in zip(accs, subs)])
            runs.append((out, accs))
        out, accs = runs[0]
        assert torch.equal(out, runs[1][0]) and all(torch.equal(a, b) for a, b in zip(accs, runs[1][1])), (B, tile, fmt)
        worst = max(_acc_ratio(a, out.view(B, H * H, Cout), H * H, splitk, *sub) for a, sub in zip(accs, subs))
        _note("epilogue_acc_conv", fmt, "conv_output", worst, f"B={B} tile={tile} splitk={splitk}")
        if not worst <= 1.0:
            failures.append((B, tile, fmt, worst))
    assert not failures, failures


def test_epilogue_accumulators_refuse_four_channel_groups():
    """cg < 8 could put more than GN_SLOTS groups into one 160-column tile"""
    x, w, _, _ = (_dev(t) for t in NC.build_gemm_case(192, 160, 320, torch.bfloat16))
    acc = torch.zeros(3, 40, 2, dtype=torch.int64, device=DEV)
    with pytest.raises(L.PPError, match="PP_ERR_UNSUPPORTED"):
        ops.gemm(x, w, rows_per_batch=64, gn=[(acc, 4, 0, 40)])
    torch.cuda.synchronize()
    assert int(acc.abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ row moments, folded LayerNorm
@pytest.mark.parametrize("tile", [0, 53, 21])
@pytest.mark.parametrize("M", NC.ROWSTAT_M)
@pytest.mark.parametrize("N", NC.ROWSTAT_N)
def test_row_moments(N, M, tile):
    """row_stats_out against the exact sums of the stored output; N = 200: the last column tile holds 40 columns; M = 5:
    fewer rows than one pass."""
    failures = []
    for dtype, fmt in NC.DTYPES:
        x, w, bias, res = (_dev(t) for t in NC.build_gemm_case(M, N, 320, dtype))
        st = []
        out = _guarded((M, N), dtype, lambda o: st.append(ops.gemm(x, w, bias=bias, res1=res, tile=tile, row_stats=True, out=o)[1]),
                       (M, N, tile, fmt))
        st = st[0]
        S, Q, gS, gQ = NC.gate_row_stats(out)
        assert tuple(st.shape) == (M, (N + 159) // 160, 2)
        worst = max(NC.worst_ratio(st[..., 0], S, gS), NC.worst_ratio(st[..., 1], Q, gQ))
        _note("row_stats", fmt, "gemm_output", worst, f"M={M} N={N} tile={tile}")
        if not worst <= 1.0:
            failures.append((fmt, worst))
    assert not failures, failures


@pytest.mark.parametrize("tile", [0, 53])
@pytest.mark.parametrize("C", NC.FOLD_C)
@pytest.mark.parametrize("kind", NC.FOLD_KINDS)
def test_gemm_folded_layernorm_vs_layernorm_then_linear(kind, C, tile):
    """ops.gemm(ln_stats=...) against the fp64 LayerNorm -> Linear (with the 16-bit weights the kernel multiplies), not the
    one-pass formula: plain, GEGLU and V^T epilogues."""
    from powerpaint_amd.engine import _geglu_interleave
    B, hw = NC.FOLD_B, NC.FOLD_HW
    failures = []
    for dtype, fmt in NC.DTYPES:
        for regime in NC.FOLD_REGIMES:
            k = NC.build_fold_case(kind, C, regime, dtype)
            x, w16, cs, t, st = (_dev(k[n]) for n in ("x", "w16", "cs", "t", "st"))
            ref, gate = NC.gate_folded_ln(x, w16, cs, t, 1e-5, k["tiles"], dtype, kind == "geglu")
            assert bool(torch.isfinite(gate).all())
            kw = dict(ln_stats=st, ln_dim=C, ln_eps=1e-5, tile=tile)
            if kind == "plain":
                out = _guarded((k["M"], k["N"]), dtype, lambda o: ops.gemm(x, w16, bias=t, ln_colsum=cs, out=o, **kw), (kind, C, fmt))
            elif kind == "geglu":
                out = _guarded((k["M"], k["N"] // 2), dtype,
                               lambda o: ops.gemm(x, _geglu_interleave(w16).contiguous(), bias=_geglu_interleave(t).contiguous(),
                                                  ln_colsum=_geglu_interleave(cs).contiguous(), act=L.PP_ACT_GEGLU, out=o, **kw),
                               (kind, C, fmt))
            else:
                n_qk = k["N"] * 2 // 3
                qk, vt = ops.gemm(x, w16, bias=t, ln_colsum=cs, vt_col0=n_qk, rows_per_batch=hw, **kw)
                out = torch.cat([qk, vt.transpose(1, 2).reshape(B * hw, k["N"] - n_qk)], 1)
            assert bool(torch.isfinite(out.float()).all())
            worst = NC.worst_ratio(out, ref, gate)
            _note("folded_ln_" + kind, fmt, regime, worst, f"C={C} tile={tile}")
            if not worst <= 1.0:
                failures.append((fmt, regime, worst))
    assert not failures, failures


@pytest.mark.parametrize("w8", [True, False], ids=["8wave", "4wave"])
def test_ff_fused_folded_layernorm(w8):
    """pp_ff_fused at the smallest shape it accepts (M 128, C 320), hs in the offset16 and outlier regimes, against the fp64
    LayerNorm -> GEGLU feed-forward -> [FF2 . proj_out | proj_out] of the 16-bit weights."""
    from powerpaint_amd.engine import _geglu_interleave, _kperm_geglu
    C = NC.FF_C
    inv = torch.argsort(NC.quad_perm(8 * C))
    assert torch.equal(_geglu_interleave(torch.arange(8 * C)), inv)           # the layout build_ff_case assumes
    assert L.lib().pp_ff_fused_supported(NC.FF_M, C, NC.FF_M) == 1
    failures = []
    for dtype, fmt in NC.DTYPES:
        for regime in NC.FUSED_REGIMES:
            k = {n: _dev(t) for n, t in NC.build_ff_case(regime, dtype).items()}
            ref, gate = NC.gate_ff_fused(k["hs"], k["w1"], k["b1"], k["cs1"], k["w2"], k["bias2"], 1e-5, dtype)
            w2 = k["w2"] if w8 else torch.cat([_kperm_geglu(k["w2"][:, :4 * C]), k["w2"][:, 4 * C:]], 1).contiguous()
            out = ops.ff_fused(k["hs"], k["w1"], k["b1"], w2, bias2=k["bias2"], cs1=k["cs1"], ln_stats=k["st"], w2_kperm=not w8)
            worst = NC.worst_ratio(out, ref, gate)
            _note("ff_fused", fmt, regime, worst, "8-wave" if w8 else "4-wave")
            if not worst <= 1.0:
                failures.append((fmt, regime, worst))
    assert not failures, failures


def test_tfront_groupnorm_proj_in_layernorm_qkv():
    """pp_tfront at the smallest shape it accepts (M 128, C 320), offset16 and outlier (proj_in carries the regime into the
    rows LayerNorm1 sees): hs against the fp64 GroupNorm -> proj_in, then Q | K | V^T against the fp64 LayerNorm -> Linear of
    the hs the kernel stored, with the error terms of moments formed inside the kernel."""
    from powerpaint_amd.engine import _kperm
    B, hw, C = NC.TF_B, NC.TF_HW, NC.TF_C
    assert L.lib().pp_tfront_supported(B * hw, C, hw, 32) == 1
    failures = []
    for dtype, fmt in NC.DTYPES:
        for regime in NC.FUSED_REGIMES:
            k = {n: _dev(t) for n, t in NC.build_tfront_case(regime, dtype).items()}
            acc = NC.build_acc(k["x"], None, 32)
            hs, qk, vt = ops.tfront(k["x"].view(B * hw, C), acc, k["gg"], k["gb"], k["w1"], k["b1"], _kperm(k["wf"]).contiguous(),
                                    k["cs"], k["tb"], hw)
            r1, g1 = NC.gate_tfront_hs(k["x"], k["gg"], k["gb"], k["w1"], k["b1"], dtype)
            r2, g2 = NC.gate_tfront_qkv(hs, k["wf"], k["cs"], k["tb"], dtype)
            assert bool(torch.isfinite(g1).all()) and bool(torch.isfinite(g2).all())
            qkv = torch.cat([qk, vt.transpose(1, 2).reshape(B * hw, C)], 1)
            w_hs, w_qkv = NC.worst_ratio(hs, r1, g1), NC.worst_ratio(qkv, r2, g2)
            _note("tfront_hs", fmt, regime, w_hs, "M=128")
            _note("tfront_qkv", fmt, regime, w_qkv, "M=128")
            if not max(w_hs, w_qkv) <= 1.0:
                failures.append((fmt, regime, w_hs, w_qkv))
    assert not failures, failures


def test_xattn_block_folded_layernorm():
    """pp_xattn_block at the smallest shape it accepts (two batch items of one 128-row tile, C 320, 7 context tokens), x in
    the offset16 and outlier regimes, against the fp64 LayerNorm -> logits -> per-head softmax -> H^T + bias + residual of
    the folded 16-bit matrices."""
    B, hw, C = NC.XA_B, NC.XA_HW, NC.XA_C
    assert L.lib().pp_xattn_block_supported(B * hw, C, hw, NC.XA_NCTX, NC.XA_HEADS) == 1
    failures = []
    for dtype, fmt in NC.DTYPES:
        for regime in NC.FUSED_REGIMES:
            k = {n: _dev(t) for n, t in NC.build_xattn_case(regime, dtype).items()}
            folded = (k["gt"], k["gcs"], k["gb"], k["ht"])
            ref, gate = NC.gate_xattn_block(k["x"], 2, folded, k["bo"], k["x"], hw, 1e-5, dtype)
            assert bool(torch.isfinite(gate).all())
            out = ops.xattn_block(k["x"], folded, bias_o=k["bo"], res=k["x"], ln_stats=k["st"], rows_per_batch=hw)
            worst = NC.worst_ratio(out, ref, gate)
            _note("xattn_block", fmt, regime, worst, "M=256 nctx=7")
            if not worst <= 1.0:
                failures.append((fmt, regime, worst))
    assert not failures, failures
