"""CPU: the probes of tests/gemm_cases.py can fail, and only for a reason.

`tile_walk_emulate` restates on the CPU what the GEMM / conv kernels do structurally (tiles under the XCD remap in both tile
orders, the K walk and its split-K slices, slabs and combine, the conv geometry, the epilogue order with one rounding, stores
through the leading dimensions).  Here:

  * the faithful emulation passes every case of the GPU matrix -- equality for E and T, the derived gate for R, nothing stored
    outside a window;
  * every builder precondition (sum |x||w| < 2^24, expected values representable, no invisible 64 x 64 block, GroupNorm
    partials exact) holds for every case: `build` asserts them;
  * each named defect fails at least one case; the table names the probe and the smallest case that catches it;
  * slice starts of every kind, grids with tiles % 8 == 0, != 0 and tiles < 8, both tile orders with a ragged edge, and every
    tile id under every probe occur in the matrix;
  * the derived R gate beside the check(atol, rtol) tolerances of the older random tests, element by element on their shapes.

defect                                         probe  smallest case that catches it
---------------------------------------------  -----  ------------------------------------------------------------------------
drop_last_k_tile_of_slice                      E      plain-E-M40-N200-K64+64-t32-sk2-bias
slice_restart_in_x2_reads_x1                   E      plain-E-M40-N200-K64+64-t32-sk2-bias
slice_restart_in_tail_reads_x3_for_x4          E      conv-E-2x16x16-c128+64-t128+64-n160-t0-sk3-bias+rowvec+res1+res2+half
tail_uses_tap_geometry                         E      conv-E-3x8x8-c64+0-t128+64-n328-t33-sk3-bias+res2
ky_kx_swapped                                  E      conv-E-1x5x7-c64+0-t0+0-n160-s2-t32-sk1-bias
halo_crosses_batch_item                        E      conv-E-2x24x8-c64+0-t0+0-n160-s2-t1-sk2-bias+res2
stride2_odd_last_row_dropped                   E      conv-E-1x5x7-c64+0-t0+0-n160-s2-t32-sk1-bias
up_rounds_half_up                              E      conv-E-1x5x7-c192+0-t0+0-n200-up-t32-sk1-res1
rows_past_M_written                            E      plain-E-M40-N36-K64-t0-sk1                  (sentinel rows behind `out`)
cols_past_N_written                            E      plain-E-M40-N36-K64-t0-sk1                  (pad columns, next row)
pad_columns_of_ldo_written                     E      plain-E-M40-N36-K64-t0-sk1                  (pad columns)
n_major_tile_swap                              E      plain-E-M40-N200-K64-t22-sk1                (1 x 2 tiles, N-major)
xcd_remap_drops_tile_when_grid_not_mult_of_8   E      plain-E-M40-N200-K64-t22-sk1                (2 tiles)
x2_offset_uses_ldx1                            E      plain-E-M261-N160-K128+192-t0-sk1
res_uses_ldo                                   E      plain-E-M40-N160-K64-t62-sk1-bias+rowvec+res1+res2+half  (ldres2 != ldo)
rowvec_batch_from_tile_start                   E      plain-E-M261-N328-K64-t44-sk1-bias+rowvec+res1+res2+half
res1_wrap_off_by_rows                          E      plain-E-M256-N200-K192-t32-sk1-bias+res1+half-wrap       (poison row)
scale_after_residual                           E      plain-E-M40-N160-K64-t62-sk1-bias+rowvec+res1+res2+half
bias_after_scale                               T      plain-T:bias-M40-N36-K64-t1-sk1
store_truncates                                T      plain-T:rne-M40-N36-K64-t1-sk1
acc_rounded_before_residual                    T      plain-T:res-M40-N36-K64-t1-sk1
fp16_through_bf16                              T      plain-T:b256-M40-N36-K64-t1-sk1             (fp16)
combine_drops_last_slab                        E      plain-E-M40-N200-K64+64-t32-sk2-bias
vt_transposed_within_batch_only                E      plain-E-M256-N480-K192-t32-sk1-bias+half-vt
row_stats_count_pad_columns                    E      plain-E-M261-N328-K192-t32-sk1-bias+res1-stats
gn_acc_counts_rows_past_M                      E      plain-E-M192-N320-K192-t54-sk1-bias+rowvec+res1+res2+half-gn
subpix_parity_swapped                          E      subpix-E-3x8x8-c64+0-t0+0-n328-t2-sk1-bias+res2

The older tests' tolerances (`test_the_derived_gate_beside_the_older_tolerances`): the derived gate is below
atol + rtol |ref| at EVERY element of test_gemm_plain, test_gemm_splitk, test_conv3x3, test_conv3x3_with_1x1_tail and
test_gemm_fp16 (at most 0.46 of it).  On test_conv3x3_fp16 (K = 2880) it is not: the worst-case n_r 2^-24 A = 5.9e-3 exceeds
atol = 5e-3 where |ref| < 0.45 (a fifth of the elements, gate / tolerance up to 1.35).  Those tests therefore assert BOTH,
which is everywhere at least as tight as either.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gemm_cases as GC  # noqa: E402

BF, HF = torch.bfloat16, torch.float16
BY_ID = {c.id: c for c in GC.CASES}
DEFECT_TABLE = {
    "drop_last_k_tile_of_slice": "plain-E-M40-N200-K64+64-t32-sk2-bias",
    "slice_restart_in_x2_reads_x1": "plain-E-M40-N200-K64+64-t32-sk2-bias",
    "slice_restart_in_tail_reads_x3_for_x4": "conv-E-2x16x16-c128+64-t128+64-n160-t0-sk3-bias+rowvec+res1+res2+half",
    "tail_uses_tap_geometry": "conv-E-3x8x8-c64+0-t128+64-n328-t33-sk3-bias+res2",
    "ky_kx_swapped": "conv-E-1x5x7-c64+0-t0+0-n160-s2-t32-sk1-bias",
    "halo_crosses_batch_item": "conv-E-2x24x8-c64+0-t0+0-n160-s2-t1-sk2-bias+res2",
    "stride2_odd_last_row_dropped": "conv-E-1x5x7-c64+0-t0+0-n160-s2-t32-sk1-bias",
    "up_rounds_half_up": "conv-E-1x5x7-c192+0-t0+0-n200-up-t32-sk1-res1",
    "rows_past_M_written": "plain-E-M40-N36-K64-t0-sk1",
    "cols_past_N_written": "plain-E-M40-N36-K64-t0-sk1",
    "pad_columns_of_ldo_written": "plain-E-M40-N36-K64-t0-sk1",
    "n_major_tile_swap": "plain-E-M40-N200-K64-t22-sk1",
    "xcd_remap_drops_tile_when_grid_not_mult_of_8": "plain-E-M40-N200-K64-t22-sk1",
    "x2_offset_uses_ldx1": "plain-E-M261-N160-K128+192-t0-sk1",
    "res_uses_ldo": "plain-E-M40-N160-K64-t62-sk1-bias+rowvec+res1+res2+half",
    "rowvec_batch_from_tile_start": "plain-E-M261-N328-K64-t44-sk1-bias+rowvec+res1+res2+half",
    "res1_wrap_off_by_rows": "plain-E-M256-N200-K192-t32-sk1-bias+res1+half-wrap",
    "scale_after_residual": "plain-E-M40-N160-K64-t62-sk1-bias+rowvec+res1+res2+half",
    "bias_after_scale": "plain-T:bias-M40-N36-K64-t1-sk1",
    "store_truncates": "plain-T:rne-M40-N36-K64-t1-sk1",
    "acc_rounded_before_residual": "plain-T:res-M40-N36-K64-t1-sk1",
    "fp16_through_bf16": "plain-T:b256-M40-N36-K64-t1-sk1",
    "combine_drops_last_slab": "plain-E-M40-N200-K64+64-t32-sk2-bias",
    "vt_transposed_within_batch_only": "plain-E-M256-N480-K192-t32-sk1-bias+half-vt",
    "row_stats_count_pad_columns": "plain-E-M261-N328-K192-t32-sk1-bias+res1-stats",
    "gn_acc_counts_rows_past_M": "plain-E-M192-N320-K192-t54-sk1-bias+rowvec+res1+res2+half-gn",
    "subpix_parity_swapped": "subpix-E-3x8x8-c64+0-t0+0-n328-t2-sk1-bias+res2",
}
_built = {}


def _build(c, dtype):
    """built once, shared, never modified (the emulation writes into buffers of its own)"""
    if (c.id, dtype) not in _built:
        _built[(c.id, dtype)] = GC.build(c, dtype)
    return _built[(c.id, dtype)]


@pytest.mark.parametrize("c", GC.CASES, ids=lambda c: c.id)
def test_faithful_emulation_passes_and_preconditions_hold(c):
    for dtype, fmt in GC.case_dtypes(c):
        t = GC.build(c, dtype)                          # asserts the preconditions of E and T
        if c.probe.startswith("R"):
            assert bool((GC.gate(c, t, dtype) > 0).all()) or float(t["ref"].abs().min()) == 0.0
        if c.expect:
            continue                                    # the library refuses it: nothing to emulate
        assert GC.emulation_failures(c, t, dtype) == [], (c.id, fmt)


def test_the_defect_table_is_complete():
    assert set(DEFECT_TABLE) == set(GC.DEFECTS) and len(GC.DEFECTS) == 27
    assert all(v in BY_ID for v in DEFECT_TABLE.values()), [v for v in DEFECT_TABLE.values() if v not in BY_ID]
    doc = sys.modules[__name__].__doc__
    assert all(d in doc and DEFECT_TABLE[d] in doc for d in GC.DEFECTS)


@pytest.mark.parametrize("defect", GC.DEFECTS)
def test_each_defect_fails_its_case(defect):
    c = BY_ID[DEFECT_TABLE[defect]]
    caught = []
    for dtype, fmt in GC.case_dtypes(c):
        t = _build(c, dtype)
        assert GC.emulation_failures(c, t, dtype) == []
        if GC.emulation_failures(c, t, dtype, defect):
            caught.append(fmt)
    assert caught, (defect, c.id)
    if defect != "fp16_through_bf16":                   # a defect of the arithmetic shows in both formats
        assert len(caught) == len(GC.case_dtypes(c)), (defect, caught)


def test_probe_t_fails_on_half_the_elements_under_truncation():
    """the no-epilogue tie probe: a truncating store is wrong wherever the sum is odd and RNE rounds up -- a quarter of the
    elements --, and RNE itself is exercised on every odd sum: half of them"""
    c = BY_ID["plain-T:rne-M40-N36-K64-t1-sk1"]
    for dtype, _ in GC.case_dtypes(c):
        t = _build(c, dtype)
        odd = (t["ref"] % 2 == 1).double().mean()
        assert 0.45 < float(odd) < 0.55
        out, _ = GC.emu_result(c, t, dtype, "store_truncates")
        wrong = (out != GC.expected_out(c, t, dtype).double()).double().mean()
        assert float(wrong) > 0.2


def test_gate_is_as_tight_as_the_issue_states():
    """K = 2944, R+: the gate is 1.045 u (bf16) and 1.36 u (fp16) -- a 2 u error fails"""
    for dtype, want in ((BF, 1.045), (HF, 1.36)):
        ref = torch.ones(1, 1, dtype=torch.float64)
        g = GC.gate_rpm(ref, ref, 2944, 1, dtype) / GC.unit_roundoff(dtype)
        assert abs(float(g) - want) < 0.01, float(g)


def test_matrix_reaches_every_mechanism():
    live = [c for c in GC.CASES if not c.expect]
    print(f"[gemm probes] {len(GC.CASES)} cases ({len(live)} run, {len(GC.CASES) - len(live)} refusals), "
          f"{sum(len(GC.case_dtypes(c)) for c in GC.CASES)} (case, format) pairs")
    # every tile id (AUTO included) meets every probe and every ragged edge
    for tile in GC.TILE_IDS:
        mine = [c for c in live if c.tile == tile]
        assert {c.probe[0] for c in mine} == {"E", "T", "R"}, tile
        plain = [c for c in mine if c.kind == "plain"]
        assert any(c.M % GC.launch_form(c)[1] for c in plain) and any(c.N % 160 for c in plain), tile
        assert {c.M for c in GC.CASES if c.tile == tile and c.kind == "plain"} >= set(GC.PLAIN_M), tile
        assert {c.N for c in GC.CASES if c.tile == tile and c.kind == "plain"} >= set(GC.PLAIN_N), tile
    assert {c.splitk for c in live if c.kind == "plain" and c.K == 704} >= set(GC.SPLITS)
    assert {(c.K1, c.K2) for c in live if c.kind == "plain" and c.K2} == {(128, 192), (64, 64)}
    # N % 8 = 4: the register-staged kernel serves it, a v2 id is refused as v2_ok says
    n36 = [c for c in GC.CASES if c.kind == "plain" and c.N == 36]
    assert all((c.expect == GC.PP_ERR_BAD_ARG) == bool(c.tile and GC.TILES[c.tile][2]) for c in n36)
    assert any(c.expect for c in n36) and any(not c.expect for c in n36)
    # slice starts
    kinds = {k for c in live for k in GC.slice_start_kinds(c)}
    assert kinds >= {"in_x2", "tap", "in_tail", "x3x4", "in_x1", "tail", "empty"}, kinds
    # grids: tiles % 8 == 0, != 0, < 8; both tile orders with a ragged edge
    grids, orders = set(), set()
    for c in live:
        fam, bm, sk, _ = GC.launch_form(c)
        tm = c.rows // bm if fam == "halo" else -(-c.rows // bm)
        tn = (c.N + 159) // 160
        g = tm * tn
        grids.add("lt8" if g < 8 else "mult8" if g % 8 == 0 else "ragged8")
        if c.rows % bm or c.N % 160:
            orders.add("n_major" if (tm < tn and tm <= 8) else "m_major")
    assert grids == {"lt8", "mult8", "ragged8"} and orders == {"n_major", "m_major"}
    # the conv lists, the halo-tile loop with BM 64 / 128 / 256, plain / up / sub-pixel / split
    conv = [c for c in live if c.kind != "plain"]
    assert {(c.B, c.H, c.W) for c in conv} >= set(GC.CONV_SHAPES)
    assert {(c.K1, c.K2) for c in conv} >= set(GC.CONV_CH) and {(c.C3, c.C4) for c in conv} >= set(GC.CONV_TAILS)
    assert {c.N for c in conv} >= set(GC.CONV_COUT) and {c.stride for c in conv} == {1, 2} and any(c.up for c in conv)
    assert any(c.stride == 2 and c.H % 2 for c in conv)
    halo = [c for c in conv if c.halo]
    assert {GC.halo_form(c)[0] for c in halo if c.kind == "conv"} == {64, 128, 256}
    assert {GC.halo_form(c)[0] for c in halo if c.kind == "subpix"} == {64, 128, 256}
    assert any(c.up for c in halo) and any(GC.halo_form(c)[1] > 1 for c in halo)
    assert {c.probe for c in GC.CASES} >= {"E", "T:rne", "T:res", "T:bias", "T:b256", "R+", "R-"}
    # the epilogues that are not exactly predictable run under R-, the consumer norm of the combine on E data
    ln = [c for c in live if "ln" in c.epi]
    assert all(c.probe == "R-" for c in live if {"ln", "softmax", "geglu", "silu"} & set(c.epi))
    assert any("geglu" in c.epi for c in ln) and any(c.side == "vt" for c in ln) and any("softmax" in c.epi for c in ln)
    assert any(GC.launch_form(c)[2] > 1 for c in ln) and {GC.launch_form(c)[0] for c in ln} == {"v1", "v2"}
    assert {c.halo for c in live if c.side == "gnnext"} == {True, False}


def _rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator("cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _beside(ref, A, K, splits, dtype, atol, rtol):
    g, tol = GC.gate_rpm(ref, A, K, splits, dtype), atol + rtol * ref.abs()
    return float((g / tol).max()), float((g <= tol).double().mean())


def test_the_derived_gate_beside_the_older_tolerances():
    """on the data of tests/test_ops_gpu.py / test_fp16_gpu.py (same seeds), element by element"""
    def gemm(M, N, K, dtype, seed_scale=1.0):
        x, w = _rnd(M, K, seed=1).to(dtype).double(), _rnd(N, K, seed=2, scale=K ** -0.5).to(dtype).double()
        return x, w, _rnd(N, seed=3).double(), _rnd(M, N, seed=4).to(dtype).double()
    for M, N, K in [(256, 320, 320), (616, 640, 768), (1024, 960, 320), (2048, 320, 1280)]:          # test_gemm_plain
        x, w, b, r = gemm(M, N, K, BF)
        worst, frac = _beside(x @ w.T + b + r, x.abs() @ w.abs().T + b.abs() + r.abs(), K, 1, BF, 2e-2, 1e-2)
        assert frac == 1.0 and worst < 0.5
    x, w, b, r = gemm(512, 1280, 2560, BF)                                                            # test_gemm_splitk
    worst, frac = _beside((x @ w.T + b) * 0.5 + 2 * r, (x.abs() @ w.abs().T + b.abs()) * 0.5 + 2 * r.abs(), 2560, 4, BF, 2e-2, 1e-2)
    assert frac == 1.0 and worst < 0.5
    x, w, b, r = gemm(512, 640, 1280, HF)                                                             # test_gemm_fp16
    worst, frac = _beside(x @ w.T + b + r, x.abs() @ w.abs().T + b.abs() + r.abs(), 1280, 8, HF, 5e-3, 2.5e-3)
    assert frac == 1.0 and worst < 0.5
    for dtype, atol, rtol in ((BF, 2e-2, 1e-2), (HF, 5e-3, 2.5e-3)):                                  # test_conv3x3(_fp16)
        x = _rnd(2, 16, 16, 320, seed=1).to(dtype)
        w = _rnd(320, 2880, seed=2, scale=2880 ** -0.5).to(dtype)
        b = _rnd(320, seed=3).double()
        for stride, up in ((1, False), (2, False), (1, True)):
            worst, frac = _beside(GC.conv64(x, w, stride, up) + b, GC.conv64(x.abs(), w.abs(), stride, up) + b.abs(), 2880, 8,
                                  dtype, atol, rtol)
            if dtype == BF:
                assert frac == 1.0 and worst < 0.5
            else:
                # Reported, not pinned.  K = 2880 in fp16: the worst-case fp32 term (K + 13) 2^-24 A = 5.9e-3 alone exceeds
                # atol = 5e-3, so the derived gate is NOT the tighter one where |ref| < 0.45 (about a fifth of the elements).
                # test_conv3x3_fp16 therefore asserts both bounds; a tighter n_r would only raise `frac`.
                print(f"[gemm probes] fp16 conv s{stride} up{up}: derived gate <= check() tolerance on {frac:.3f} of the "
                      f"elements, worst gate / tolerance {worst:.3f}")
    h, x = _rnd(2, 16, 16, 320, seed=1).to(BF), _rnd(2, 16, 16, 640, seed=2).to(BF)                   # ..._with_1x1_tail
    w2, wsc = _rnd(320, 2880, seed=4, scale=2880 ** -0.5).to(BF), _rnd(320, 640, seed=5, scale=640 ** -0.5).to(BF)
    b = _rnd(320, seed=6).double()
    xin = x.double().reshape(-1, 640)
    ref = GC.conv64(h, w2).reshape(-1, 320) + xin @ wsc.double().T + b
    A = GC.conv64(h.abs(), w2.abs()).reshape(-1, 320) + xin.abs() @ wsc.double().abs().T + b.abs()
    worst, frac = _beside(ref, A, 2880 + 640, 8, BF, 3e-2, 1e-2)
    assert frac == 1.0 and worst < 0.5
