"""CPU: the probes of tests/small_cases.py can fail.  The torch restatement of every kernel's index walk (`small_cases.walk`)
meets every case of the matrix -- E cases bit for bit, R cases under the derived gate, every guard untouched, the ticket
re-armed and the counter moved by exactly one per launch -- and each named defect fails at least one case.  The GPU twin,
tests/test_small_exact_gpu.py, applies the same checks (`small_cases.compare`) to the kernels themselves."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import small_cases as SC  # noqa: E402

BIG = 300000            # work items above which a case is emulated in one format only


def _size(c):
    p = c.p
    if c.kernel == "mask" and p["mode"] == 2:
        return p["B"] * p["ho"] * p["wo"]
    return max(p.get("n", 0), p.get("hw", 0) * p.get("B", 1) * p.get("c", p.get("C", 1)), p.get("h", 0) * p.get("w", 0) * p.get("B", 1),
               p.get("H", 0) * p.get("W", 0) * p.get("cout", 0), p.get("nz", 0))


def _dtypes(c):
    d = SC.case_dtypes(c)
    return d[:1] if _size(c) > BIG else d


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(c, dtype):
        key = (c.id, dtype)
        if key not in cache:
            cache[key] = SC.build(c, dtype)
        return cache[key]
    return get


def test_ids_are_unique_and_the_matrix_is_whole():
    ids = [c.id for c in SC.CASES]
    assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1][:5]
    kernels = {c.kernel for c in SC.CASES}
    assert kernels == set(SC.BUILD), kernels ^ set(SC.BUILD)
    big = [c for c in SC.CASES if _size(c) > 4096 * 256]
    assert {c.kernel for c in big} >= {"conv_direct", "to_nhwc", "to_nchw", "add", "step", "blend", "mask"}, "capped-grid cases"
    print(f"[small probes] {len(SC.CASES)} cases, {sum(len(SC.case_dtypes(c)) for c in SC.CASES)} (case, format) runs")


@pytest.mark.parametrize("c", SC.CASES, ids=lambda c: c.id)
def test_faithful_walk_meets_the_case(c, built):
    for dtype, fmt in _dtypes(c):
        assert SC.failures(c, built(c, dtype), dtype) == [], (c.id, fmt)


def _candidates(defect):
    """the cases a defect can show on: by kernel, small ones first (the capped-grid defect needs the large ones)"""
    fam = {"hin_win_swapped": "conv_direct", "stride2_odd_last_row_dropped": "conv_direct", "clamped_pixel_not_masked": "conv_out",
           "group_crosses_batch_item": "conv_out", "third_load_round_dropped": "conv_out", "scalar_last_block_dropped": "conv_out",
           "blend": "blend", "mask": "mask", "skinny": "skinny", "softmax": "softmax", "splice": "splice", "temb": "temb",
           "ticket_not_rearmed": "step", "counter_moved_without_ticket": "step", "ksampler_push_before_read": "step",
           "pndm_save_after_update": "step", "z_read_on_quiet_row": "step", "zero_tail_dropped": ("zero", "step_head"),
           "nchw_channel_stride_from_ldc": "to_nhwc", "nchw_batch_item_ignored": "to_nchw", "direct": "conv_direct", "pack": "add", "bmod_ignored": ("to_nhwc", "step_head"), "c0_ignored": ("to_nhwc", "step_head")}
    k = fam.get(defect) or fam.get(defect.split("_")[0])
    ks = (k,) if isinstance(k, str) else k
    cs = [c for c in SC.CASES if c.probe != "X" and (ks is None or c.kernel in ks)]
    if defect == "stride_loop_second_pass_dropped":
        return [c for c in cs if _size(c) > 65536]
    return [c for c in cs if _size(c) <= BIG]


@pytest.mark.parametrize("defect", SC.DEFECTS)
def test_every_defect_fails_a_named_case(defect, built):
    hits = []
    cands = _candidates(defect)
    assert cands, defect
    seen = set()
    for c in cands:
        dtype, fmt = _dtypes(c)[0]
        f = SC.failures(c, built(c, dtype), dtype, defect)
        if f:
            hits.append((c.id, f[0]))
            seen.add(c.kernel)
            if defect != "stride_loop_second_pass_dropped" and len(hits) >= 3:
                break
    assert hits, f"no case of the matrix notices the defect {defect}"
    print(f"[small probes] {defect}: {len(hits)} cases, e.g. {hits[0][0]}: {hits[0][1][:120]}")
    if defect == "stride_loop_second_pass_dropped":      # every capped grid of the family has a case that strides
        assert seen >= {"conv_direct", "to_nhwc", "to_nchw", "add", "step", "blend", "mask", "zero", "step_head"}, seen


def test_every_case_is_failed_by_a_defect(built):
    """a probe that no defect can fail is dropped or sharpened: every runnable case of the matrix is failed by at least one of
    the named defects of its kernel (the capped-grid cases by the dropped second pass)"""
    by = {}
    for d in SC.DEFECTS:
        for c in _candidates(d):
            by.setdefault(c.id, []).append(d)
    idle = []
    for c in SC.CASES:
        if c.probe == "X":
            continue
        dtype, _ = _dtypes(c)[0]
        if not any(SC.failures(c, built(c, dtype), dtype, d) for d in by.get(c.id, [])):
            idle.append(c.id)
    assert not idle, idle


def test_refusals_are_the_host_checks():
    for c in SC.CASES:
        if c.probe == "X":
            assert SC.refuses(c) == c.expect != 0, c.id
        else:
            assert SC.refuses(c) == 0, c.id


def test_gates_are_tight_where_it_matters():
    """where the output is 16 bits wide the derived gate is the rounding of the format and little more: two units on the
    elements that carry the result (the fp32 outputs keep their worst-case n_r 2^-24 A, which no rounding hides)"""
    for c in SC.CASES:
        if c.probe != "R" or _size(c) > 20000:
            continue
        dtype, _ = SC.case_dtypes(c)[-1]
        t = SC.build(c, dtype)
        for name, g in t["gate"].items():
            ref = t["ref"][name]
            big = ref.abs() > 0.25 * ref.abs().max()
            rel = (g / ref.abs().clamp_min(1e-300))[big]
            if t["out"][name].full.dtype == torch.float32:
                continue
            assert float(rel.median()) < 2 * SC.unit_roundoff(dtype), (c.id, name, float(rel.median()))
