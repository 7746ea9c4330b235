"""CPU self-test of the attention probes (tests/attention_cases.py): the probes are only worth their GPU time if a subtly
wrong kernel fails them.  On a few-second subset of the GPU matrix the faithful emulation passes P1, P2 and P3 in both
formats, and every named defect fails at least one probe at at least one case.

Which probe kills which mutant (KILLS below is this table; the test asserts that it is what the probes do):

    mutant                              P1   P2   P3   where it first shows
    drop_last_key                        x    x    x   any nk (P2: one key of <= 129; P3: flat softmax of few keys)
    mask_lets_key_nk_in                  x    x    x   nk % 64 != 0: key nk of item 0 is key 0 of item 1, its V the poison
    tail_half_skipped_at_33              x    x    x   nk % 64 == 33 only
    v_keys_swapped_in_16_block           x    x    x   any nk > 4
    k_batch_stride_uses_nq               x    .    x   nq != nk, batch item 1 (P2: q = 0 does not look at K)
    b_h_swapped                          x    .    x   B = 2, heads = 3 (P2: V is the same for every (b, h))
    no_rescale_on_max_jump               x    .    .   >= 2 tiles and a target beyond the first (N(0, 1) scores never jump by 2^8)
    second_query_block_keeps_state       x    .    x   the K / V-reuse form (qrep = 2), second block of a pair (P2: both
                                                       blocks hold the same uniform average)
    ring_slot_off_by_one                 x    x    x   >= 2 tiles
    causal_lt                            x    x    x   pp_attention_small, causal (query 0 has no key left: not finite)
    p_rounded_to_bf16_in_fp16_mode       .    .    x   fp16 (P1 / P2 probabilities are powers of two)

It also asserts the P1 precondition (off-target mass <= 2^-20, inside build_p1) and full key coverage for EVERY case of
the GPU matrix, so that the GPU tests never skip or soften a case.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_cases as AC  # noqa: E402

DTYPES = [torch.bfloat16, torch.float16]
PROBES = ("P1", "P2", "P3")

# (d, nq, nk, qrep, causal, small): a subset of the GPU matrix that reaches every path the mutants live on
SUBSET = [
    (40, 33, 4, 1, False, False),         # below one 16-key block
    (80, 33, 13, 1, False, False),
    (40, 4, 33, 1, False, False),         # the <= 32-live-keys tail, one key past its edge; nq < nk: 9 launches of P1
    (40, 33, 77, 1, False, False),        # one tile + a 13-key tail
    (160, 33, 97, 1, False, False),       # 64 + 33
    (40, 130, 129, 1, False, False),      # three tiles, the last one with one key
    (40, 200, 320, 1, False, False),      # five tiles (the pipelined kernels' shapes)
    (40, 300, 77, 2, False, False),       # K / V reuse over two query blocks, ragged second block
    (64, 5, 5, 1, True, True),            # pp_attention_small
    (64, 77, 77, 1, True, True),
    (64, 77, 5, 1, False, True),
]

KILLS = {
    "drop_last_key": {"P1", "P2", "P3"},
    "mask_lets_key_nk_in": {"P1", "P2", "P3"},
    "tail_half_skipped_at_33": {"P1", "P2", "P3"},
    "v_keys_swapped_in_16_block": {"P1", "P2", "P3"},
    "k_batch_stride_uses_nq": {"P1", "P3"},
    "b_h_swapped": {"P1", "P3"},
    "no_rescale_on_max_jump": {"P1"},
    "second_query_block_keeps_state": {"P1", "P3"},
    "ring_slot_off_by_one": {"P1", "P2", "P3"},
    "causal_lt": {"P1", "P2", "P3"},
    "p_rounded_to_bf16_in_fp16_mode": {"P3"},
}

_setups = {}


def _setup(probe, case, dtype):
    """Built once, shared by the faithful run and every mutant; the emulation never writes to it."""
    key = (probe, case, dtype)
    if key not in _setups:
        d, nq, nk, qrep, causal, small = case
        kw = dict(p_fp32=True) if (small and probe == "P3") else {}
        s = AC.BUILDERS[probe](AC.B_, AC.H_, nq, nk, d, dtype, causal=causal, **kw)
        _setups[key] = (s, s.vt_torch())
    return _setups[key]


def _ratio(probe, case, dtype, mutant):
    d, nq, nk, qrep, causal, small = case
    s, vt = _setup(probe, case, dtype)
    worst = 0.0
    for launch in range(len(s.q)):
        o = AC.flash_emulate(s.q_view(launch), s.k_view(), vt, s.B, s.H, nq, nk, d, s.scale, dtype, mutant=mutant,
                             causal=causal, qrep=qrep, round_p=not small)
        worst = max(worst, AC.worst_ratio(o, s.expected[launch], s.gate[launch]))
    return worst


def _probes_of(case):
    return [p for p in PROBES if p != "P2" or case[2] <= 129]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_faithful_emulation_passes_every_probe(dtype):
    worst = {}
    for case in SUBSET:
        for probe in _probes_of(case):
            r = _ratio(probe, case, dtype, None)
            worst[probe] = max(worst.get(probe, 0.0), r)
            assert r <= 1.0, (probe, case, dtype, r)
    print(f"[attention probes] faithful emulation {dtype}: worst error / gate {worst}")
    assert worst["P3"] > 0.2, "the P3 gate is more than 5x what a correct kernel needs: not the derived bound"


def test_every_mutant_fails_a_probe_and_the_kill_table_is_true():
    assert set(KILLS) == set(AC.MUTANTS)
    for mutant in AC.MUTANTS:
        killed = set()
        for case in SUBSET:
            if mutant == "causal_lt" and not case[4]:
                continue                                  # (no causal mask in this case: the mutant is the faithful code)
            for dtype in DTYPES:
                for probe in _probes_of(case):
                    if probe not in killed and _ratio(probe, case, dtype, mutant) > 1.0:
                        killed.add(probe)
        print(f"[attention probes] {mutant}: killed by {sorted(killed)}")
        assert killed, f"{mutant} survives every probe: a hole in the probes"
        assert killed == KILLS[mutant], (mutant, sorted(killed), sorted(KILLS[mutant]))


def _matrix():
    for d in AC.PHASED_D:
        for nk in AC.PHASED_NK:
            for nq in AC.PHASED_NQ:
                yield AC.B_, AC.H_, nq, nk, d, False, False
    for nq, nk in AC.QR_CASES:
        yield AC.QR_B, AC.QR_H, nq, nk, 40, False, False
    for nq, nk in AC.PIPE_CASES:
        yield AC.B_, AC.H_, nq, nk, 40, False, False
        yield AC.B_, AC.H_, nq, nk, 40, False, True
    for n in AC.SMALL_N:
        yield AC.B_, AC.H_, n, n, AC.SMALL_D, True, False
        yield AC.B_, AC.H_, n, n, AC.SMALL_D, False, False
    for nq, nk in AC.SMALL_RECT:
        yield AC.B_, AC.H_, nq, nk, AC.SMALL_D, False, False


def test_p1_precondition_and_coverage_hold_on_the_whole_gpu_matrix():
    """build_p1 asserts off-target mass <= 2^-20 for every query of every launch; the keys are +-1 in either format, so one
    format decides for both except for the rounded LOG2 multiplier, which is tried in both."""
    n = 0
    for B, H, nq, nk, d, causal, log2 in _matrix():
        assert AC.p1_covers_every_key(B, H, nq, nk, causal), (B, H, nq, nk, causal)
        for dtype in (DTYPES if log2 else DTYPES[:1]):
            AC.build_p1(B, H, nq, nk, d, dtype, causal=causal, log2=log2)
            n += 1
    assert n >= 3 * 12 * 3 + 6 + 11 * 3 + 16 + 3
