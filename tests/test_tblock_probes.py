"""CPU: the probes of tests/test_tblock_exact_gpu.py can fail, and a faithful kernel passes them.

tests/tblock_cases.py restates the index walk of pp_ff_fused (both forms), pp_tfront, pp_xattn_block (plain, pre_w, wrapped, the
wide kernel) and pp_xattn_fold in NumPy and carries the defects of tblock_cases.DEFECTS by name.  Shown here, without a GPU:
  1. the faithful walk meets every case of the matrix: E cases bit for bit, R cases inside their gate, nothing stored outside a
     window;
  2. each named defect fails at least one case;
  3. every case is failed by at least one defect;
  4. every precondition of a probe holds on the reference alone (exactness, the one-hot margin, the open-unit pattern: asserted
     by the builders; the spread of the winning keys and the pack-time permutations against powerpaint_amd.engine here).
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import norm_cases as NC  # noqa: E402
import tblock_cases as TC  # noqa: E402
from powerpaint_amd import engine  # noqa: E402

BF16 = torch.bfloat16
_BUILT = {}


def built(c, dtype):
    key = (c.id, dtype)
    if key not in _BUILT:
        _BUILT[key] = TC.build(c, dtype)
    return _BUILT[key]


def fails(c, defect, dtype=BF16):
    return any(TC.walk_failures(c, built(c, dtype), dtype, f, defect)[0] for f in TC.forms(c))


# where each defect is expected to show first (any other case may be tried after these)
FIRST = {
    "stale_ring_stage": ["ff-E-open-all", "tfront-E-groups32", "xattn-E-nctx77"],
    "drop_t2_chunk37": ["ff-E-open-single"], "dup_t2_chunk38": ["ff-E-open-single"], "drop_t2_chunk39": ["ff-E-open-single"],
    "drop_tail0": ["ff-E-open-chunk"], "dup_tail4": ["ff-E-open-chunk"], "drop_tail5": ["ff-E-open-chunk"], "drop_tail9": ["ff-E-open-chunk"],
    "last_geglu_other_parity": ["ff-E-open-ends"], "kperm_geglu_identity": ["ff-E-open-chunk"],
    "geglu_interleave_identity": ["ff-E-open-chunk"], "geglu_interleave_inverse": ["ff-E-open-chunk"],
    "kperm_identity": ["tfront-E-groups32", "xattn-E-pre-w", "fold-E-c320-kperm1"],
    "kperm_inverse": ["tfront-E-groups32", "xattn-E-pre-w", "fold-E-c320-kperm1"],
    "quad_h_g_swapped": ["ff-E-open-chunk"], "wpo_offset_32": ["ff-E-open-chunk"],
    "remap_q_off_by_one": ["ff-E-grid8", "tfront-E-grid8", "xattn-E-grid8"],
    "remap_r_off_by_one": ["ff-E-grid9", "tfront-E-grid9", "xattn-E-grid9"],
    "batch_of_tile_end": ["tfront-E-rpb384-b2", "xattn-E-rpb384-b2", "ff-E-gn-rpb384-wrap"],
    "gn_stats_of_item0": ["tfront-E-groups32"], "groups_as_c_over_10": ["tfront-E-groups16"], "q_scale_on_k": ["tfront-E-groups20"],
    "vt_at_p0_zero": ["tfront-E-rpb256-b3"], "res1_wrap_per_tile": ["ff-E-wrap64"], "scale_after_residuals": ["ff-E-scale2-res12"],
    "gn_halves_not_split": ["ff-E-gn-cg40-c020"], "ff8_exchange_halves_swapped": ["ff-E-open-chunk"],
    "heads47_tables_of_03": ["xattn-E-nctx77"], "padded_not_masked": ["xattn-E-nctx7"], "wrap_on_parked_h": ["xattn-E-pre-wrap"],
    "row_stats_split_128": ["xattn-E-nctx77"], "wide_ht_group_offset_dropped": ["xattn-E-wide640-grid3"],
    "fold_ht_layout_natural": ["fold-E-c320-kperm0"], "fold_padded_not_masked": ["fold-E-nctx7"],
}
# the defects tried, in this order, on a case until one fails it
KILLERS = {"ff": ("drop_tail0", "stale_ring_stage"), "tfront": ("stale_ring_stage", "kperm_identity"),
           "xattn": ("stale_ring_stage", "heads47_tables_of_03", "padded_not_masked"),
           "fold": ("fold_ht_layout_natural", "fold_padded_not_masked")}


@pytest.mark.parametrize("kernel", ["ff", "tfront", "xattn", "fold"])
def test_the_faithful_walk_meets_every_case_and_every_case_can_fail(kernel):
    """1. and 3.: both formats and both forms through the faithful walk; then, per case, one defect that fails it"""
    n = 0
    for c in TC.CASES:
        if c.kernel != kernel:
            continue
        for dtype, fmt in TC.DTYPES:
            if dtype != BF16 and c.p.get("M", 0) > 384:             # (the format changes the rounding, not the walk)
                continue
            t = built(c, dtype)
            for f in TC.forms(c):
                bad, worst = TC.walk_failures(c, t, dtype, f)
                assert not bad, (c.id, fmt, f, bad)
                assert worst is None or worst <= 1.0, (c.id, fmt, f, worst)
                n += 1
        assert any(fails(c, d) for d in KILLERS[kernel]), (c.id, "no defect fails this case")
        _BUILT.pop((c.id, torch.float16), None)
    assert n


@pytest.mark.parametrize("defect", TC.DEFECTS)
def test_each_defect_fails_a_case(defect):
    """2.: at the case where it should show; `fails` judges exactly as the GPU file does"""
    assert set(FIRST) == set(TC.DEFECTS)
    hit = [cid for cid in FIRST[defect] if fails(TC.BY_ID[cid], defect)]
    assert hit, (defect, "passes", FIRST[defect])
    if defect in ("stale_ring_stage", "kperm_identity", "kperm_inverse", "remap_q_off_by_one", "remap_r_off_by_one", "batch_of_tile_end"):
        assert hit == FIRST[defect], (defect, "every kernel that has this structure must notice it", hit)


def test_preconditions_on_the_reference_alone():
    """4.  The builders assert exactness, the open-unit pattern and the one-hot margin for every case (a violated one raises
    here); on top: the winning keys cover key 0, nctx - 1, 79 and every 16-column block of a head, in every batch item."""
    seen = {}
    for c in TC.CASES:
        for dtype, _ in TC.DTYPES:
            t = built(c, dtype)
            if c.kernel == "xattn" and c.probe == "E" and dtype == BF16:
                w = t["winners"]                                  # [M, heads, 80]
                assert bool(w.any(-1).all())
                keys = w.any(0).any(0).nonzero().flatten().tolist()
                seen.setdefault(c.p["nctx"], set()).update(keys)
                nb = c.p["M"] // c.p["rpb"]
                if nb > 1:                                         # the items' tables differ
                    i = t["inp"]
                    assert not torch.equal(i["ht"][0], i["ht"][1])
                    if c.p["nctx"] > 1:                            # (one key: one winner, one bias)
                        assert not torch.equal(i["gt"][0], i["gt"][1]) and not torch.equal(i["gb"][0], i["gb"][1])
            _BUILT.pop((c.id, torch.float16), None)
    for nctx, keys in seen.items():
        assert 0 in keys and nctx - 1 in keys, (nctx, sorted(keys))
        assert {k // 16 for k in keys} == set(range((nctx + 15) // 16)), (nctx, sorted(keys))
    assert 79 in seen[80]


def test_the_pack_time_permutations_are_the_engines():
    w = torch.arange(4 * 1280, dtype=torch.float32).reshape(4, 1280)
    assert torch.equal(engine._kperm(w), w[:, TC.kperm_idx(1280)])
    assert torch.equal(engine._kperm_geglu(w), w[:, TC.kperm_geglu_idx(1280)])
    r = torch.arange(2560, dtype=torch.float32)[:, None].expand(2560, 3).contiguous()
    il = TC.geglu_interleave_idx(2560)
    assert torch.equal(engine._geglu_interleave(r), r[il])
    assert torch.equal(torch.argsort(il), NC.quad_perm(2560))        # interleaved quads -> [values | gates]
    assert torch.equal(TC.kperm_idx(640), NC.xattn_kk())
    kg = TC.kperm_geglu_idx(32)
    assert torch.equal(kg[kg], torch.arange(32))                       # an involution: its inverse is no separate defect
    kp = TC.kperm_idx(32)
    assert not torch.equal(kp[kp], torch.arange(32)) and not torch.equal(kp, torch.arange(32))


def test_the_remap_is_a_bijection_only_when_all_four_pieces_are_right():
    for nwg in range(1, 73):
        assert sorted(TC.remap(b, nwg) for b in range(nwg)) == list(range(nwg)), nwg
        # consecutive tiles share an XCD: the tiles of XCD x are one contiguous run
        for x in range(min(8, nwg)):
            run = [TC.remap(b, nwg) for b in range(x, nwg, 8)]
            assert run == list(range(run[0], run[0] + len(run)))
    for d, grids in (("remap_q_off_by_one", (8, 9, 17)), ("remap_r_off_by_one", (9, 17))):
        for nwg in grids:
            assert sorted(TC.remap(b, nwg, d) for b in range(nwg)) != list(range(nwg)), (d, nwg)


def test_the_piece_sequence_of_ff_fused():
    """130 pieces; every step refills the stage read one step before; T2(c - 1) follows the chunk pair that carries its GEGLU;
    the K tail sits between T2(38) and T2(39)"""
    P = TC.FF_PIECES
    assert len(P) == 130 and len(set(P)) == 130
    assert P.index(("T2", 39, 0)) == 129 and P.index(("TAIL", 0, 0)) == P.index(("T2", 38, 0)) + 1
    for c in range(1, 40):
        assert P.index(("T1", c, 1)) + 1 == P.index(("T2", c - 1, 0))
    for step in range(5, 130):                                          # piece `step` is issued at step - 5 into stage (step - 6) % 6
        assert step % TC.FF_NS == (step - 5 - 1) % TC.FF_NS


def test_matrix_size():
    kinds = {}
    for c in TC.CASES:
        kinds[(c.kernel, c.probe)] = kinds.get((c.kernel, c.probe), 0) + 1
    print(kinds, len(TC.REFUSALS), "refusals", len(TC.DEFECTS), "defects")
    assert len(TC.CASES) >= 120 and len(TC.REFUSALS) >= 65 and len(TC.DEFECTS) >= 34
    assert all(kinds.get((k, "E"), 0) >= 15 for k in ("ff", "tfront", "xattn", "fold"))
    assert all(kinds.get((k, "R"), 0) >= 7 for k in ("ff", "tfront", "xattn"))
