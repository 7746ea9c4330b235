"""CPU: the probes of tests/test_unet_blocks_gpu.py can fail, and the faithful arithmetic passes them.

The emulation of tests/unet_cases.py (torch float32, the plans' rounding points) takes the place of the GPU in the teacher-forced
chain, at the configurations and shapes of the GPU file (`unet_cases.CASES`):
  * the faithful emulation meets the derived gate at every gated tap of every network of every case, and the free-running
    float64 chain built from the same segments agrees with it end to end under the gate of the existing network tests (cosine
    >= 0.999, max-abs <= 3e-2 max(1, max|ref|)); every resnet of the free-running chain equals oracle/sd_modules.py's ResnetBlock2D in
    float64 (unet_cases.CROSS_RTOL);
  * every defect of `unet_cases.DEFECTS` breaks the gate of one tap at least.  A defect sits in one segment, and in a
    teacher-forced chain only that segment's tap can see it: the segment is re-run with the defect on the faithful emulation's
    taps, at every segment of the cases that can carry it, and its tap is held to the gate the faithful tap met;
  * every network of every case is compiled on a host arena (no launch): the forms its shape must select are the ones in the
    plan (`unet_cases.FORMS`: a silent fallback to the chain fails here and in the GPU file), the tap names equal the list
    derived from SDNet._resnet_specs / _attn_specs / _zero_conv_specs and the form table, every block-output tap keeps its bytes
    to the end of the plan, every tensor recorded inside a block is written by the call it names.
Every segment is gated, both attention segments of a transformer in each of the four cross-attention forms included; every packed
tensor they read is compared with its composition from the checkpoint tensors.
"""
import math

import pytest
import torch

import unet_cases as UC
import vae_cases as VC

_CHAIN = {}


def chain(c):
    """The faithful emulation of a case and the (ref, gate) results of each of its networks, computed once."""
    if c.id not in _CHAIN:
        out = {}
        for kind, (n, sd, taps, io) in UC.emulate(c).items():
            t64, i64 = {k: v.double() for k, v in taps.items()}, UC.io64(io)
            out[kind] = (n, sd, taps, io, t64, i64, UC.check_chain(n, c, sd, t64, i64))
        _CHAIN[c.id] = out
    return _CHAIN[c.id]


@pytest.mark.parametrize("c", UC.CASES, ids=lambda c: c.id)
def test_faithful_emulation_meets_every_gate(c):
    for kind, (n, sd, taps, io, t64, i64, res) in chain(c).items():
        gated = [s.name for s in UC.steps(n, c.H, c.W)]
        assert not UC.pack_violations(sd, io.packed, [(p, C) for p, C in UC.make_net(n)._attn_specs()], UC.FMT[c.fmt])
        assert [r[0] for r in res] == gated and len(set(gated)) == len(gated)
        bad = [(kind, nm, k, r, w) for nm, k, r, w in res if not r <= 1.0]
        assert not bad, bad
        # end to end: the free-running float64 chain against the emulation's outputs, the gate of the existing network tests
        want = UC.free_run(n, c, sd, i64)
        for got, ref in zip(UC.outputs_of(n, t64), UC.outputs_of(n, want)):
            cos, rel = UC.e2e(got, ref)
            assert cos >= 0.999 and rel <= 1.0, (kind, cos, rel)


def _carriers(defect):
    kind, pred = UC.DEFECT_AT[defect]
    for c in UC.CASES:
        for n in c.nets:
            for st in UC.steps(n, c.H, c.W):
                if st.kind == kind and pred(st):
                    yield c, n, st


@pytest.mark.parametrize("defect", UC.DEFECTS)
def test_every_defect_breaks_a_gate(defect):
    seen, broke = 0, []
    for c, n, st in _carriers(defect):
        _, sd, taps, io, t64, i64, res = chain(c)[n.kind]
        out = UC.emu_step(sd, n, st, taps, io, UC.FMT[c.fmt], defect)
        if torch.equal(out, taps[st.name]):
            continue                                             # the defect cannot show here (an even target, no residual, ...)
        seen += 1
        ratio = UC.check_chain(n, c, sd, dict(t64, **{st.name: out.double()}), i64, only=(st.name,))[0][2]
        if ratio > 1.0:
            broke.append((c.id, st.name, ratio))
            break
    assert seen, "no segment of any case carries the defect"
    assert broke, f"{defect}: passes every gate it meets ({seen} segments): the bound is too loose"


@pytest.mark.parametrize("form", ["CHAIN", "BLOCK", "BLOCK_PRE", "TWO_GEMM"])
@pytest.mark.parametrize("defect", ["second_item_reads_first_items_context", "pad_context_keys_enter_softmax", "attn2_out_bias_dropped"])
def test_cross_attention_defects_break_in_every_form(defect, form):
    """the first .attn2 segment of each cross-attention form (the 16x64 case has all four) catches each of its defects"""
    c = UC.CASES[0]
    n, sd, taps, io, t64, i64, res = chain(c)["unet"]
    st = [s for s in UC.steps(n, c.H, c.W) if s.kind == "t_attn2" and io.forms[s.opt["pre"]] == form][0]
    out = UC.emu_step(sd, n, st, taps, io, UC.FMT[c.fmt], defect)
    ratio = UC.check_chain(n, c, sd, dict(t64, **{st.name: out.double()}), i64, only=(st.name,))[0][2]
    assert ratio > 1.0, (st.name, form, ratio)


def test_defect_table_is_complete():
    assert set(UC.DEFECT_AT) == set(UC.DEFECTS) and len(UC.DEFECTS) == 24
    assert UC.LAMBDA == VC.LAMBDA and 2.0 * math.exp(-UC.LAMBDA ** 2 / 2.0) < 1e-13


@pytest.mark.parametrize("c", UC.CASES, ids=lambda c: c.id)
def test_dry_build_forms_tap_names_and_layout(c):
    for n in c.nets:
        rt, log = UC.dry_runtime(n, c)
        assert not UC.form_violations(rt, c), UC.form_violations(rt, c)
        taps = rt.lay["taps"]
        assert [t[0] for t in taps] == UC.tap_names(rt.net, UC.forms_of(rt, c), n.wiring)
        # the wiring by name (unet_cases.steps) names the same block outputs, in the same order
        assert [t[0] for t in taps if not t[0].rsplit(".", 1)[-1] in ("proj_in", "attn1", "attn1_out", "attn2")] == \
            [s.name for s in UC.steps(n, c.H, c.W) if s.kind not in UC.INNER]
        assert not VC.tap_layout_violations(UC.block_taps(taps), log)
        assert not UC.inner_tap_violations(rt), UC.inner_tap_violations(rt)
        if c.twin:
            half = {t[0]: t[1].B for t in taps if hasattr(t[1], "B")}
            assert half["conv_in"] == c.B and half["down_blocks.0.resnets.0"] == c.B // 2 and \
                half["down_blocks.0.attentions.0.attn1"] == c.B // 2 and half["down_blocks.0.attentions.0"] == c.B
