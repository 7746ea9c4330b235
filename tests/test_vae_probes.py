"""CPU: the probes of tests/test_vae_blocks_gpu.py can fail, and the faithful arithmetic passes them.

The emulation of tests/vae_cases.py (torch float32, the plans' rounding points) takes the place of the GPU in the teacher-forced
chain, at the configurations and shapes of the GPU file (`vae_cases.CASES`: the checkpoints' widths, both formats of the
asymmetric VAE):
  * the faithful emulation meets the derived gate at every tap of every case, and the free-running float64 chain built from the
    same blocks agrees with it end to end under the gate of the existing parity tests (cosine 0.999, max-abs 5 %);
  * every defect of `vae_cases.DEFECTS` breaks the gate of one tap at least.  A defect sits in one block, and in a
    teacher-forced chain only that block's tap can see it: the block is re-run with the defect on the faithful emulation's
    taps, at every block of the case that can carry it, and its tap is held to the gate the faithful tap met.
The defects run at the checkpoints' widths and layer counts, like the faithful chain (the whole file takes about a minute).
"""
import math

import pytest
import torch
import torch.nn.functional as F

import vae_cases as VC

_CHAIN = {}


def chain(c):
    """The faithful emulation of a case, its float64 view and the (ref, gate) results, computed once."""
    if c.id not in _CHAIN:
        cfg, sd = VC.CFG[c.model], VC.state_dict(c.model)
        taps, extra = VC.emulate(c, cfg, sd, VC.inputs(c))
        t64, e64 = VC.as64(taps, extra)
        _CHAIN[c.id] = (cfg, sd, taps, extra, t64, e64, VC.check_chain(c, cfg, sd, t64, e64))
    return _CHAIN[c.id]


@pytest.mark.parametrize("c", VC.CASES, ids=lambda c: c.id)
def test_faithful_emulation_meets_every_gate(c):
    cfg, sd, taps, extra, t64, e64, res = chain(c)
    names = [s.name for s in VC.steps(cfg, c.direction, c.cond, c.model == "asym")]
    assert [r[0] for r in res] == names and len(set(names)) == len(names)
    bad = [(n, k, r, w) for n, k, r, w in res if not r <= 1.0]
    assert not bad, bad
    # end to end: the free-running float64 chain against the emulation's last tap, the gate of the existing parity tests
    want = VC.free_run(c, cfg, sd, e64)
    got = t64["decoder.conv_out"][:, :3] if c.direction == "decode" else t64["quant_conv"].flip(2, 3)
    cos = F.cosine_similarity(got.flatten(), want.flatten(), dim=0).item()
    rel = ((got - want).abs().max() / want.abs().max()).item()
    assert cos >= 0.999 and rel <= 0.05, (cos, rel)


def _carriers(defect):
    kind, pred = VC.DEFECT_AT[defect]
    for c in VC.CASES:
        cfg = VC.CFG[c.model]
        for st in VC.steps(cfg, c.direction, c.cond, c.model == "asym"):
            if st.kind == kind and pred(st):
                yield c, st


@pytest.mark.parametrize("defect", VC.DEFECTS)
def test_every_defect_breaks_a_gate(defect):
    seen, broke = 0, []
    for c, st in _carriers(defect):
        cfg, sd, taps, extra, t64, e64, res = chain(c)
        out = VC.emu_step(sd, st, taps, extra, VC.FMT[c.fmt], cfg["groups"], defect)
        if torch.equal(out, taps[st.name]):
            continue                                             # the defect cannot show here (no pad keys, mask of one size, ...)
        seen += 1
        ratio = VC.check_chain(c, cfg, sd, dict(t64, **{st.name: out.double()}), e64, only=(st.name,))[0][2]
        if ratio > 1.0:
            broke.append((c.id, st.name, ratio))
        if broke:
            break
    assert seen, "no block of any case carries the defect"
    assert broke, f"{defect}: passes every gate it meets ({seen} blocks): the bound is too loose"


def test_defect_table_is_complete():
    assert set(VC.DEFECT_AT) == set(VC.DEFECTS) and len(VC.DEFECTS) == 15
    assert 2.0 * math.exp(-VC.LAMBDA ** 2 / 2.0) < 1e-13                  # the confidence the quadrature terms are carried at
