"""CPU self-test of the normalisation probes (tests/norm_cases.py): the gates are only worth their GPU time if a correct
kernel meets them and a subtly wrong one does not.  On the WHOLE GPU matrix of tests/test_norm_exact_gpu.py, in both
formats, the faithful emulation of every path stays within its gate; every named defect fails at least one case; in the
`zero` regime every gate is tighter, element for element, than the `2e-2 + 1e-2 |ref|` it replaces; and the regime builders
meet their preconditions.

Where each defect shows (KILLS below is this table; the test asserts that it is what the gates do):

    defect                              path that carries it                    first case that fails
    last_chunk_dropped                  gn_stats_kernel                         hw = 47: chunk 1 of 2
    per_floor                           gn_stats_kernel                         hw = 47: per 23, pixel 46 lost
    n_counts_c1_only                    gn_fold / gn_fold_acc                   8 + 56 and 640 + 320 channels
    x2_read_with_c1_stride              stats and apply                         8 + 56 and 640 + 320 channels
    slot_group_from_first_channel       gn_apply_kernel                         cg = 10, 30, 257, 2
    tail_loop_rows_skipped              gn_apply_kernel                         C 1280, hw 2065: rows 2048 ..
    fourth_prefetched_row_dropped       gn_apply_kernel                         every shape with >= 4 row passes
    batch_from_tile_start               epilogue accumulators                   rows_per_batch 64 on a 128- / 256-row tile
    acc_scales_swapped                  gn_fold_acc, epilogue accumulators      everywhere
    ragged_column_tile_dropped          epilogue accumulators, row moments      N = 200
    ln_last_block_skipped               layernorm_kernel                        rows 1, 5, 7
    np_one_too_small                    layernorm_kernel                        C 520, 1032, 1544 (and every C > 512)
    folded_cs_mean_dropped              every fp32 one-pass consumer            everywhere (largest in offset16 / edge)
    folded_ln_dim_is_one_tile           every fp32 one-pass consumer            everywhere
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_cases as NC  # noqa: E402

KILLS = {
    "last_chunk_dropped": {"gn_stats"},
    "per_floor": {"gn_stats"},
    "n_counts_c1_only": {"gn_stats", "gn_acc"},
    "x2_read_with_c1_stride": {"gn_stats", "gn_acc"},
    "slot_group_from_first_channel": {"gn_stats", "gn_acc"},
    "tail_loop_rows_skipped": {"gn_stats", "gn_acc"},
    "fourth_prefetched_row_dropped": {"gn_stats", "gn_acc"},
    "batch_from_tile_start": {"epilogue_acc"},
    "acc_scales_swapped": {"gn_acc", "epilogue_acc"},
    "ragged_column_tile_dropped": {"epilogue_acc", "row_stats"},
    "ln_last_block_skipped": {"layernorm"},
    "np_one_too_small": {"layernorm"},
    "folded_cs_mean_dropped": {"folded_ln", "ff_fused", "tfront", "xattn_block"},
    "folded_ln_dim_is_one_tile": {"folded_ln", "ff_fused", "tfront", "xattn_block"},
}
OLD_ATOL, OLD_RTOL = 2e-2, 1e-2

_cache = {}


def _memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


# ------------------------------------------------------------------------------------------------ the cases, one list per path
def _gn_cases(path):
    for shape in NC.GN_SHAPES:
        for dtype, _ in NC.DTYPES:
            for regime in NC.gn_regimes(shape):
                for silu in (True, False):
                    for eps in NC.gn_eps_list(regime, silu):
                        yield (path, shape, dtype, regime, silu, eps)


def _gn_setup(case):
    path, shape, dtype, regime, silu, eps = case

    def make():
        k = _memo(("gn", path, shape, dtype, regime), lambda: NC.build_gn_case(shape, regime, dtype, path))
        ref, gate = NC.gate_groupnorm(k["x1"], k["x2"], shape[2], k["gamma"], k["beta"], eps, silu, dtype, k["terms"], k["exact"])
        return k, ref, gate
    return _memo(("gn_gate",) + case, make)


def _gn_ratio(case, defect):
    path, shape, dtype, regime, silu, eps = case
    k, ref, gate = _gn_setup(case)
    x1 = NC._np(k["x1"])
    x2 = NC._np(k["x2"]) if k["x2"] is not None else None
    g, b = k["gamma"].numpy(), k["beta"].numpy()
    if path == "stats":
        partial = _memo(("partial", shape, dtype, regime, defect), lambda: NC.emu_gn_stats(x1, x2, shape[2], defect))
        out = NC.emu_gn_apply(x1, x2, shape[2], g, b, eps, silu, dtype, partial=partial, defect=defect)
    else:
        acc = NC.build_acc(k["x1"], k["x2"], shape[2]).numpy()
        out = NC.emu_gn_apply(x1, x2, shape[2], g, b, eps, silu, dtype, acc=acc, defect=defect)
    return NC.worst_ratio(out, ref, gate)


def _ln_cases():
    for C in NC.LN_C:
        for rows in NC.LN_ROWS:
            for dtype, _ in NC.DTYPES:
                for regime in NC.ln_regimes(C):
                    for eps in ((1e-5, 1e-6) if regime == "constant" else (1e-5,)):
                        yield (C, rows, dtype, regime, eps)


def _ln_setup(case):
    C, rows, dtype, regime, eps = case

    def make():
        k = NC.build_ln_case(C, rows, regime, dtype)
        return (k,) + NC.gate_layernorm(k["x"], k["gamma"], k["beta"], eps, dtype, regime == "constant")
    return _memo(("ln",) + case, make)


def _ln_ratio(case, defect):
    k, ref, gate = _ln_setup(case)
    out = NC.emu_layernorm(NC._np(k["x"]), k["gamma"].numpy(), k["beta"].numpy(), case[4], case[2], defect)
    return NC.worst_ratio(out, ref, gate)


def _stored(M, N, K, dtype):
    """a GEMM's stored 16-bit output, as the epilogue statistics see it"""
    def make():
        x, w, bias, res = NC.build_gemm_case(M, N, K, dtype)
        return (x.double() @ w.double().t() + bias.double() + res.double()).to(dtype)
    return _memo(("stored", M, N, K, dtype), make)


def _epi_cases():
    for case in NC.EPI_CASES:
        for tile in NC.EPI_TILES:
            for dtype, _ in NC.DTYPES:
                yield case + (tile, dtype)


def _epi_ratio(case, defect):
    name, B, rpb, N, K, subs, splitk, tile, dtype = case
    out = _stored(B * rpb, N, K, dtype)
    tile_rows = {53: 256, 44: 128, 22: 64, 0: 128}[tile]
    block = NC.epilogue_block_rows(rpb, splitk)
    accs = NC.emu_epilogue_acc(NC._np(out), rpb, subs, block, 16 if splitk > 1 else tile_rows, defect)
    worst = 0.0
    for acc, (cg, c0, groups) in zip(accs, subs):
        S, Q, gS, gQ = NC.gate_epilogue_acc(out.reshape(B, rpb, N), rpb, cg, c0, groups, NC.epilogue_block_rows(rpb, splitk))
        a = torch.from_numpy(acc).double()
        worst = max(worst, NC.worst_ratio(a[..., 0] / NC.SUM_SCALE, S, gS), NC.worst_ratio(a[..., 1] / NC.SQ_SCALE, Q, gQ))
    return worst


def _rs_cases():
    for N in NC.ROWSTAT_N:
        for M in NC.ROWSTAT_M:
            for dtype, _ in NC.DTYPES:
                yield (M, N, dtype)


def _rs_ratio(case, defect):
    M, N, dtype = case
    out = _stored(M, N, 320, dtype)
    st = torch.from_numpy(NC.emu_row_stats(NC._np(out), defect)).double()
    S, Q, gS, gQ = NC.gate_row_stats(out)
    return max(NC.worst_ratio(st[..., 0], S, gS), NC.worst_ratio(st[..., 1], Q, gQ))


def _fold_cases():
    for kind in NC.FOLD_KINDS:
        for C in NC.FOLD_C:
            for regime in NC.FOLD_REGIMES:
                for dtype, _ in NC.DTYPES:
                    yield (kind, C, regime, dtype)


def _fold_setup(case):
    kind, C, regime, dtype = case

    def make():
        k = NC.build_fold_case(kind, C, regime, dtype)
        return (k,) + NC.gate_folded_ln(k["x"], k["w16"], k["cs"], k["t"], 1e-5, k["tiles"], dtype, kind == "geglu")
    return _memo(("fold",) + case, make)


def _fold_ratio(case, defect):
    k, ref, gate = _fold_setup(case)
    out = NC.emu_folded_ln(k["x"], k["w16"], k["cs"], k["t"], k["st"], 1e-5, case[1], case[3], case[0] == "geglu", defect)
    return NC.worst_ratio(out, ref, gate)


def _ff_cases():
    for regime in NC.FUSED_REGIMES:
        for dtype, _ in NC.DTYPES:
            yield (regime, dtype)


def _ff_ratio(case, defect):
    k = NC.build_ff_case(*case)
    ref, gate = NC.gate_ff_fused(k["hs"], k["w1"], k["b1"], k["cs1"], k["w2"], k["bias2"], 1e-5, case[1])
    return NC.worst_ratio(NC.emu_ff_fused(k, 1e-5, case[1], defect), ref, gate)


def _tf_ratio(case, defect):
    k = _memo(("tf",) + case, lambda: NC.build_tfront_case(*case))
    hs, qkv = NC.emu_tfront(k, case[1], defect)
    r1, g1 = NC.gate_tfront_hs(k["x"], k["gg"], k["gb"], k["w1"], k["b1"], case[1])
    r2, g2 = NC.gate_tfront_qkv(hs, k["wf"], k["cs"], k["tb"], case[1])
    return max(NC.worst_ratio(hs, r1, g1), NC.worst_ratio(qkv, r2, g2))


def _xa_ratio(case, defect):
    def make():
        k = NC.build_xattn_case(*case)
        return (k,) + NC.gate_xattn_block(k["x"], 2, (k["gt"], k["gcs"], k["gb"], k["ht"]), k["bo"], k["x"], NC.XA_HW, 1e-5, case[1])
    k, ref, gate = _memo(("xa",) + case, make)
    assert bool(torch.isfinite(gate).all())
    return NC.worst_ratio(NC.emu_xattn_block(k, case[1], defect), ref, gate)


PATHS = {
    "gn_stats": (lambda: _gn_cases("stats"), _gn_ratio),
    "gn_acc": (lambda: _gn_cases("acc"), _gn_ratio),
    "layernorm": (_ln_cases, _ln_ratio),
    "epilogue_acc": (_epi_cases, _epi_ratio),
    "row_stats": (_rs_cases, _rs_ratio),
    "folded_ln": (_fold_cases, _fold_ratio),
    "ff_fused": (_ff_cases, _ff_ratio),
    "tfront": (_ff_cases, _tf_ratio),
    "xattn_block": (_ff_cases, _xa_ratio),
}


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("path", sorted(PATHS))
def test_faithful_emulation_meets_every_gate_of_the_gpu_matrix(path):
    cases, ratio = PATHS[path]
    worst, where, n = 0.0, None, 0
    for case in cases():
        r = ratio(case, None)
        n += 1
        if r > worst:
            worst, where = r, case
        assert r <= 1.0, (path, case, r)
    print(f"[norm probes] {path}: {n} cases, faithful emulation worst error / gate {worst:.3f} at {where}")


def test_every_defect_fails_a_case_and_the_kill_table_is_true():
    assert set(KILLS) == set(NC.DEFECTS)
    for defect in NC.DEFECTS:
        killed = set()
        for path in sorted(PATHS):
            cases, ratio = PATHS[path]
            for case in cases():
                if ratio(case, defect) > 1.0:
                    killed.add(path)
                    break
        print(f"[norm probes] {defect}: fails {sorted(killed)}")
        assert killed, f"{defect} survives every case: a hole in the matrix"
        assert killed == KILLS[defect], (defect, sorted(killed), sorted(KILLS[defect]))


def test_the_gates_are_tighter_than_the_tolerance_they_replace():
    """Against a vacuous bound: in the `zero` regime every gate is below 2e-2 + 1e-2 |ref| at every element."""
    n = 0
    for path in ("stats", "acc"):
        for case in _gn_cases(path):
            if case[3] == "zero":
                _, ref, gate = _gn_setup(case)
                assert bool((gate < OLD_ATOL + OLD_RTOL * ref.abs()).all()), case
                n += 1
    for case in _ln_cases():
        if case[3] == "zero":
            _, ref, gate = _ln_setup(case)
            assert bool((gate < OLD_ATOL + OLD_RTOL * ref.abs()).all()), case
            n += 1
    for case in _fold_cases():
        if case[2] == "zero":
            _, ref, gate = _fold_setup(case)
            assert bool((gate < 3e-2 + 1e-2 * ref.abs()).all()), case          # (test_gemm_folded_layernorm's tolerance)
            n += 1
    for case in _epi_cases():
        name, B, rpb, N, K, subs, splitk, tile, dtype = case
        for cg, c0, groups in subs:
            S, Q, gS, gQ = NC.gate_epilogue_acc(_stored(B * rpb, N, K, dtype).reshape(B, rpb, N), rpb, cg, c0, groups,
                                                NC.epilogue_block_rows(rpb, splitk))
            assert bool((gS < 1e-2 + 1e-4 * S.abs()).all()) and bool((gQ < 1e-2 + 1e-4 * Q.abs()).all()), case
    for case in _rs_cases():
        S, Q, gS, gQ = NC.gate_row_stats(_stored(case[0], case[1], 320, case[2]))
        assert bool((gS < 1e-3 + 1e-5 * S.abs()).all()) and bool((gQ < 1e-3 + 1e-5 * Q.abs()).all()), case
    assert n >= 2 * 12 * 2 * 2 + 9 * 3 * 2 + 3 * 2 * 2


def test_the_regime_builders_meet_their_preconditions():
    """On the whole matrix: `edge` keeps a standard deviation of at least two quanta of the format at its mean and sits at
    the envelope (or at the format's limit); `constant` is exactly representable and has zero variance."""
    seen_edge = 0
    for path in ("stats", "acc"):
        for shape in NC.GN_SHAPES:
            for dtype, _ in NC.DTYPES:
                for regime in NC.gn_regimes(shape):
                    k = _memo(("gn", path, shape, dtype, regime), lambda: NC.build_gn_case(shape, regime, dtype, path))
                    x = torch.cat([k["x1"], k["x2"]], -1) if k["x2"] is not None else k["x1"]
                    _check_regime(regime, x.double(), shape[2], dtype, k["ratio"], k["terms"])
                    seen_edge += regime == "edge"
    for C in NC.LN_C:
        for regime in NC.ln_regimes(C):
            for dtype, _ in NC.DTYPES:
                k = NC.build_ln_case(C, 7, regime, dtype)
                _check_regime(regime, k["x"].double()[:, None, :].reshape(7, 1, C), 1, dtype, k["ratio"], None)
                seen_edge += regime == "edge"
    for case in _fold_cases():
        k, _, _ = _fold_setup(case)
        _check_regime(case[2], k["x"].double().reshape(k["M"], 1, case[1]), 1, case[3], k["ratio"], NC.folded_ln_eps(k["tiles"]))
        seen_edge += case[2] == "edge"
    assert seen_edge >= 4 + 2 + 12


def _check_regime(regime, x, groups, dtype, ratio, terms):
    n, _, _, mean, var = NC._pop(x, groups)
    if regime == "edge":
        assert ratio >= 1.0
        assert 2.0 * NC.quantum(ratio + 4.0, dtype) <= 1.0, (ratio, dtype)          # std 1 >= two quanta up to mean + 4 std
        if terms is not None:
            assert ratio == min(np.sqrt(NC.kappa_envelope(terms[0], terms[1], dtype) - 1.0), NC.max_ratio_of_format(dtype))
        if n >= 100:
            assert bool(((mean.abs() - ratio).abs() < 0.5).all()) and bool((var > 0.5).all()) and bool((var < 2.0).all())
    if regime == "constant":
        assert bool((var == 0).all())
        assert bool((x * 2 == torch.round(x * 2)).all()) and float(x.abs().max()) <= 7.5 and float(x.abs().min()) >= 0.5
    if regime == "offset16" and n >= 100:
        assert bool(((mean.abs() - 16).abs() < 0.5).all())
