"""-m gpu: the UNet, BrushNet and ControlNet step plans block by block at the checkpoint's widths (tests/unet_cases.py: the cases,
the wiring by name, the teacher-forced float64 references, the derived gates; proof that the probes can fail:
tests/test_unet_probes.py).

Every network of every case runs through the product entry point (NetRuntime.ensure / load_input / set_cond / set_context /
set_timestep / load_residual / run_step), eager and as a captured graph (same bits), and its recorded taps (`rt.lay["taps"]`)
are read.  A side network runs first; its outputs reach the UNet through load_residual.  The CONDITION of a case: the
cross-attention forms and launches its shape must select are the ones in the plan (unet_cases.FORMS); a silent fallback fails.

  1. every tap: one eager walk of plan.calls copies each tensor recorded inside a block right after the call that completes
     it; the block-output taps of that walk must equal the product run's, bit for bit.  Then every tap, every element, against its segment evaluated in float64 on
     the HIP path's own bits of the inputs the reference's wiring names, under the segment's derived gate.  Under the twin
     prefix a tensor stored for one half stands for both.
  2. whole-plan poison: every byte of the arena is filled with 16-bit NaN patterns except the regions of EXEMPT below, each with
     the comment in the source that makes it one; the walk and the graph run again: the outputs and every tap, the ones inside
     the blocks included, must keep their bits.
  3. identical batch items (items equal, contexts equal): every tap's items are bit-identical.  A twin case is also rebuilt
     without the twin prefix on the same inputs.  Bit equality between the two plans does NOT hold by design (DESIGN.md section 5,
     tests/test_twin_gpu.py: the prefix runs half the rows per launch, which may change a split-K factor and with it the fp32
     summation order; it was met on one set of inputs here and missed at down_blocks.0.resnets.0 on another): temb_all, which no
     row count touches, and conv_in (single-pass in both plans, stored for the full batch) must be bit-equal, the two halves
     of conv_in must be equal in the main run of a twin case, and the two plans must record the same taps; for the others the number of
     bit-equal taps is written to the profile, no threshold on it (a 16-bit rounding that flips in the prefix moves every tap
     behind it, so no per-tap bound follows from 'a few values differ by one rounding'); each plan is itself held to the float64
     gates of probe 1 (this case, and the same shape without the twin prefix in the case before it).
  4. end to end: the outputs against the free-running float64 chain under the gate of tests/test_models_gpu.py (cosine >= 0.999,
     max-abs <= 3e-2 max(1, max|ref|)), printed next to the per-segment figures.

After a whole run of the file profiles/unet_blocks_achieved.txt is rewritten: per (network, format, segment kind and, for
a transformer's segments, form, width and size) the worst achieved / gate and where, per case the forms and launches that ran, the number of bit-equal poison and identical-item runs and
the end-to-end figures, and the wall time; no threshold is pinned on the ratios.
"""
import os
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import unet_cases as UC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402

DEV = "cuda"
NAN16 = 0x7FC1                      # a NaN in bf16 and fp16; two of them a NaN in fp32
WORST, EQUAL, E2E, FORMS_MET, TWIN_EQUAL, DONE, T0 = {}, {}, {}, {}, {}, set(), [None]
_NETS = {}
# What the poison leaves alone, and why each may be left alone (everything else in the arena is filled with NaN patterns):
EXEMPT = (
    ("t_dev", "the timestep, an input (NetRuntime.set_timestep)"),
    ("gn_acc", "runtime.py, _build: 'int64 accumulators of the GroupNorm statistics the GEMM epilogues produce ...; zeroed by the first "
               "launch of every step' (and the split-K tile counters, engine.py, _gemm: 'persistent words of the pool the step's "
               "first launch zeroes')"),
    ("fault", "runtime.py, _build: 'placement violations seen by the in-kernel split-K combines (check_faults)': a counter the "
              "plan only ever adds to and check_faults reads"),
    ("x_in", "the network input; its pad channels -- runtime.py, _build: 'The arena is zero-filled and nothing else ever writes "
             "the pad channels'"),
    ("ehs", "the context, an input (NetRuntime.set_context)"),
    ("cond", "the ControlNet conditioning image, an input (NetRuntime.set_cond)"),
    ("slots", "runtime.py, _build: 'slots for foreign residual tensors (copied in at forward time)': inputs"),
    # the setup plan's outputs, one by one (its scratch and every gap between them ARE poisoned):
    ("kv", "engine.py, SDNet.__init__: 'transformer -> hoisted cross-attention (K, ldk, V^T, ldvt)' (net.kv), build_setup: K "
           "[B nctx][C] and V^T [B][C][ldvt]; the V^T row padding nctx..ldvt is the arena's zeros -- build_setup: 'ldvt = "
           "_align(nctx, 8)', the GEMM's out_vt store writes nctx columns"),
    ("xa", "engine.py, XAttnFold: 'Folded cross-attention operands of one transformer (written by pp_xattn_fold in the setup "
           "plan)': gt, gcs, gb, ht (net.xa)"),
    ("upfold", "engine.py, build_setup: 'Upsample2D convs in their sub-pixel form ...: the folded weights are a cache derived "
               "from the packed conv weight, rebuilt with everything else here' (net.upfold)"),
    ("cond_emb", "engine.py, SDNet.__init__: '(controlnet) the conditioning embedding' (net.cond_emb), conv_in's res2"),
)
ACHIEVED_HEADER = (
    "# tests/test_unet_blocks_gpu.py on one MI355X: per (network, format, segment kind) the largest achieved error / gate over every\n"
    "# element of every tap of that kind (gates: tests/unet_cases.py, derived, not fitted: the ratio shows the slack, no threshold is\n"
    "# pinned on it) and the case and tap it was met at; per (network, wiring, format) the number of bit-equal whole-plan poison\n"
    "# runs and identical-item runs and the end-to-end figures of the same runs against the free-running float64 chain (gate\n"
    "# 0.999 / 3e-2 max(1, max|ref|)); per case the cross-attention forms that ran.  The wall time is rounded to 30 s, at least\n"
    "# 30 s, so that this tracked file is the same after every run.\n")


@pytest.fixture(scope="module", autouse=True)
def _achieved():
    T0[0] = time.time()
    yield
    _NETS.clear()
    if DONE != {c.id for c in UC.CASES}:
        return
    try:
        with open(os.path.join(ROOT, "profiles", "unet_blocks_achieved.txt"), "w") as f:
            f.write(ACHIEVED_HEADER)
            for key in sorted(WORST):
                r, where = WORST[key]
                f.write(f"[unet blocks] {key[0]} {key[1]} {key[2]}: worst error / gate {r:.3f} at {where}\n")
            for key in sorted(EQUAL):
                p, b = EQUAL[key]
                cos, rel = E2E[key]
                f.write(f"[unet blocks] {key[0]} {key[1]} {key[2]}: {p} poison runs bit-equal, {b} identical-item runs bit-equal; "
                        f"end to end worst cosine {cos:.6f}, max-abs / bound {rel:.4f}\n")
            for key in sorted(TWIN_EQUAL):
                f.write(f"[unet blocks] {key}: {TWIN_EQUAL[key][0]} of {TWIN_EQUAL[key][1]} taps bit-equal to the plan without the twin prefix\n")
            for key in sorted(FORMS_MET):
                f.write(f"[unet blocks] {key}: {FORMS_MET[key]}\n")
            wall = max(30, 30 * round((time.time() - T0[0]) / 30))
            f.write(f"# {len(UC.CASES)} cases; wall time of the file about {wall} s\n")
    except OSError:
        pass


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _runtime(n, c):
    """one NetRuntime per (network, format), its weights loaded once; one set of device weights per kind at a time"""
    key = (n, c.fmt)
    if key not in _NETS:
        for k in [k for k in _NETS if k[0].kind == n.kind]:
            del _NETS[k]
        from powerpaint_amd.runtime import NetRuntime
        net = UC.make_net(n, UC.FMT[c.fmt])
        net.load_state_dict(UC.state_dict(n), DEV)
        _NETS[key] = NetRuntime(net, DEV)
    return _NETS[key]


def _ensure(rt, n, c, twin):
    wiring = ("plain",)
    if n.wiring != "plain":
        sh = rt._residual_shapes(c.B, c.H, c.W, with_up=n.wiring == "brushnet")
        wiring = (n.wiring, {k: [0] * len(v) for k, v in sh.items()})
    rt.ensure(c.B, c.H, c.W, UC.NCTX, rt.net.cin0, wiring, cond_hw=(8 * c.H, 8 * c.W) if n.kind == "controlnet" else None,
              scale=UC.SCALE if n.kind != "unet" else 1.0, twin=twin)


def _load(rt, n, c, inp, side):
    """the inputs through the product entry points; side: the runtime of the side network whose outputs feed this UNet"""
    rt.load_input([(inp["x_" + n.kind].to(DEV), 0)])
    if n.kind == "controlnet":
        rt.set_cond(inp["cond"].to(DEV))
    rt.set_context(inp["ctx"].to(DEV), force=True)
    rt.set_timestep(UC.TIMESTEP)
    if side is not None:
        o = side.outputs
        for group in ("down", "up"):
            for i, a in enumerate(o.get(group, [])):
                rt.load_residual(group, i, side.act_as_nchw(a))
        rt.load_residual("mid", 0, side.act_as_nchw(o["mid"]))
    torch.cuda.synchronize()


def _bytes(rt, t):
    return rt.arena.view(t.ptr, (t.nbytes,), torch.uint8).clone()


def _value(rt, t, dtype):
    """a tap as float64 on the host: an Act as NCHW, a TapF32 in its stored shape"""
    if hasattr(t, "shape"):
        return rt.arena.view(t.ptr, tuple(t.shape), torch.float32).double().cpu()
    return rt.arena.view(t.ptr, (t.B, t.H, t.W, t.C), dtype).permute(0, 3, 1, 2).double().cpu()


def _walk(rt, dtype):
    """plan.calls one by one; every tensor recorded inside a block is copied right after the call that completes it ->
    ({name: bytes}, {name: value}) of those tensors"""
    inner = [t for t in rt.lay["taps"] if len(t) == 3]
    bits, val = {}, {}
    for call in rt.step_plan.calls:
        fn, args, name = call
        L.check(fn(*args, _stream()), name)
        for t in inner:
            if t[2] is call:
                torch.cuda.synchronize()
                bits[t[0]], val[t[0]] = _bytes(rt, t[1]), _value(rt, t[1], dtype)
    torch.cuda.synchronize()
    assert len(bits) == len(inner), "a tensor recorded inside a block names a call that is not in the plan"
    return bits, val


def _block_bits(rt):
    return {t[0]: _bytes(rt, t[1]) for t in rt.lay["taps"] if len(t) == 2}


def _keep_regions(rt):
    """[(lo, hi)] byte ranges of EXEMPT in this arena"""
    lay, keep = rt.lay, []
    span = lambda a: (a.ptr, a.ptr + a.nbytes)      # noqa: E731
    keep += [(lay["t_dev"], lay["t_dev"] + 256), (lay["gn_acc"], lay["fault"]), (lay["fault"], lay["fault"] + 256), span(lay["x_in"])]
    keep.append((lay["ehs"], lay["ehs"] + rt.B * rt.nctx * rt.net.ctx_dim * 2))
    if "cond" in lay:
        keep.append(span(lay["cond"]))
    last = max(hi for _, hi in keep)
    for group in lay["slots"].values():
        keep += [span(a) for a in group]
    net, B = rt.net, rt.B
    for k, c, vt, ldvt in net.kv.values():
        keep += [(k, k + B * rt.nctx * c * 2), (vt, vt + B * c * ldvt * 2)]
    S = net.heads * 80
    for pre, xa in net.xa.items():
        c = dict(net._attn_specs())[pre]
        keep += [(xa.gt, xa.gt + B * S * c * 2), (xa.ht, xa.ht + B * c * S * 2), (xa.gcs, xa.gcs + B * S * 4), (xa.gb, xa.gb + B * S * 4)]
    rev = list(reversed(net.boc))
    for pre, ptr in net.upfold.items():
        c = rev[int(pre.split(".")[1])]
        keep.append((ptr, ptr + 16 * c * c * 2))
    if net.cond_emb is not None:
        keep.append(span(net.cond_emb))
    return keep


def _poison(rt):
    keep = _keep_regions(rt)
    saved = [(lo, hi, rt.arena.view(lo, (hi - lo,), torch.uint8).clone()) for lo, hi in keep if hi > lo]
    rt.arena.buf.view(torch.int16).fill_(NAN16)
    for lo, hi, b in saved:
        rt.arena.view(lo, (hi - lo,), torch.uint8).copy_(b)
    torch.cuda.synchronize()


def _io(rt, n, c, dtype, subpix):
    """the segments' inputs as the HIP path holds them, by name (float64)"""
    lay = rt.lay
    named = {}
    if n.kind == "controlnet":
        named["cond_emb"] = _value(rt, rt.net.cond_emb, dtype)
    pre = {"brushnet": "add", "controlnet": "ctrl"}.get(n.wiring)
    for group, acts in lay["slots"].items():
        for i, a in enumerate(acts):
            named[f"{pre}_mid" if group == "mid" else f"{pre}_{group}.{i}"] = _value(rt, a, dtype)
    ctx = rt.arena.view(lay["ehs"], (c.B, UC.NCTX, UC.CTX_DIM), dtype).double().cpu()
    packed = lambda name: rt.net.params.tensor(name).cpu()      # noqa: E731  (the ParamPack's tensors, by name)
    return UC.NetIO(_value(rt, lay["x_in"], dtype), named, ctx, scale=UC.SCALE if n.kind != "unet" else 1.0, subpix=subpix,
                    packed=packed, twin=c.twin, forms=UC.forms_of(rt, c))


def _full(v, B):
    """a tensor the twin prefix stored for one half stands for both"""
    return torch.cat([v, v]) if v.dim() == 4 and v.shape[0] * 2 == B else v


def _form(name, kind, forms, c):
    """what tells two runs of a segment kind apart: a transformer's segments by its cross-attention form and level width (the
    fused front end, pp_ff_fused and the unfused pp_transpose_v path follow from the two and the case's size)"""
    if not kind.startswith("t_"):
        return kind
    pre = name
    while pre not in forms:
        pre = pre.rsplit(".", 1)[0]
    lvl = {"down_blocks.0": 320, "down_blocks.1": 640, "down_blocks.2": 1280, "mid_block": 1280, "up_blocks.1": 1280,
           "up_blocks.2": 640, "up_blocks.3": 320}[pre.rsplit(".attentions", 1)[0]]
    return f"{kind}[{forms[pre]},C={lvl},{c.H}x{c.W}]"


def _record(n, c, res, forms):
    for name, kind, r, where in res:
        key = (f"{n.kind}({n.wiring})", c.fmt, _form(name, kind, forms, c))
        if key not in WORST or r > WORST[key][0]:
            WORST[key] = (r, f"{c.id} {name} {where}")


def _outputs(rt, n):
    o = rt.outputs
    if n.kind == "unet":
        return [rt.eps_tensor().clone()]
    return [rt.act_as_nchw(a).clone() for a in list(o["down"]) + [o["mid"]] + list(o.get("up", []))]


def _same(a, b):
    """finite and equal (every output is also a tap, and those are compared byte for byte)"""
    return all(bool(torch.isfinite(x).all()) and torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("c", UC.CASES, ids=lambda c: c.id)
def test_case(c):
    dtype, inp, fails, side = UC.FMT[c.fmt], UC.inputs(c), [], None
    for n in c.nets:
        sd, rt = UC.state_dict(n), _runtime(n, c)
        _ensure(rt, n, c, c.twin)
        assert rt.twin == c.twin
        tag = f"{c.id} {n.kind}"

        # ---- the condition: the forms this shape must select ran
        bad = UC.form_violations(rt, c)
        assert not bad, f"{tag}: the plan does not run the forms the case is about: {bad}"
        forms = UC.forms_of(rt, c)
        taps = rt.lay["taps"]
        assert [t[0] for t in taps] == UC.tap_names(rt.net, forms, n.wiring)
        assert not UC.inner_tap_violations(rt)
        FORMS_MET[f"{c.id} {n.kind}({n.wiring})"] = " ".join(f"{k}={v}" for k, v in sorted(forms.items()))      # what xattn_forms answered
        launches = {call[2] for call in rt.step_plan.calls}
        FORMS_MET[f"{c.id} {n.kind}({n.wiring}) launches"] = " ".join(sorted(launches))

        # ---- the product run, eager and graph
        _load(rt, n, c, inp, side)
        rt.run_step(use_graph=False)
        torch.cuda.synchronize()
        out, bits = _outputs(rt, n), _block_bits(rt)
        rt.run_step(use_graph=True)
        torch.cuda.synchronize()
        if not (_same(_outputs(rt, n), out) and all(torch.equal(v, bits[k]) for k, v in _block_bits(rt).items())):
            fails.append(f"{tag}: the captured graph and the eager run differ")
        rt.check_faults()

        # ---- 1. every tap against its teacher-forced reference
        ibits, ival = _walk(rt, dtype)
        moved = [k for k, v in _block_bits(rt).items() if not torch.equal(v, bits[k])]
        assert not moved, f"{tag}: the launch-by-launch walk differs from the run, first at {moved[:1]}"
        val = {t[0]: _full(_value(rt, t[1], dtype), c.B) for t in taps if len(t) == 2}
        val.update({k: _full(v, c.B) for k, v in ival.items()})
        subpix = {t[0] for t in taps if len(t) == 2 and ".upsamplers." in t[0] and t[1].producer.subpix}
        io = _io(rt, n, c, dtype, subpix)
        bad = UC.pack_violations(sd, io.packed, rt.net._attn_specs(), dtype)
        assert not bad, f"{tag}: packed tensors differ from their composition from the checkpoint tensors: {bad[:3]}"
        res = UC.check_chain(n, c, sd, val, io)
        _record(n, c, res, forms)
        for name, kind, r, where in res:
            print(f"[unet blocks] {tag} {kind:8s} {name}: error / gate {r:.3f} at {where}")
            if not r <= 1.0:
                fails.append(f"{tag}: tap {name} ({kind}): error / gate {r:.3f} at {where}")

        if c.twin:                                                 # the twice-stored tensor: each half against the other
            ci = bits["conv_in"]
            if not torch.equal(ci[:ci.numel() // 2], ci[ci.numel() // 2:]):
                fails.append(f"{tag}: the two halves of the twin prefix's conv_in differ")

        # ---- 2. whole-plan poison
        _poison(rt)
        assert all(bool(torch.isnan(rt.arena.view(t[1].ptr, (t[1].nbytes // 2,), dtype)).all()) for t in taps), "the poison did not land"
        pbits, _ = _walk(rt, dtype)
        differ = [k for k, v in _block_bits(rt).items() if not torch.equal(v, bits[k])] + \
                 [k for k, v in pbits.items() if not torch.equal(v, ibits[k])]
        poison_ok = _same(_outputs(rt, n), out) and not differ
        _poison(rt)                                                # (the graph captured above: a replay, no warm-up run in front)
        rt.run_step(use_graph=True)
        torch.cuda.synchronize()
        gdiffer = [k for k, v in _block_bits(rt).items() if not torch.equal(v, bits[k])]
        poison_ok = poison_ok and _same(_outputs(rt, n), out) and not gdiffer
        if not poison_ok:
            fails.append(f"{tag}: poisoned arena: the output or taps differ, first {(differ + gdiffer)[:1]}: the plan reads memory "
                         f"it did not write")

        # ---- 4. end to end, the same run
        want = UC.outputs_of(n, UC.free_run(n, c, sd, io))
        got = [o.double().cpu() for o in out]
        cos, rel = 1.0, 0.0
        for g_, w_ in zip(got, want):
            cs, rl = UC.e2e(g_, w_)
            cos, rel = min(cos, cs), max(rel, rl)
        print(f"[unet blocks] {tag} end to end: cosine {cos:.6f}, max-abs / bound {rel:.4f}; worst segment {max(r[2] for r in res):.3f}")
        if not (cos >= 0.999 and rel <= 1.0):
            fails.append(f"{tag}: end to end: cosine {cos:.6f} (>= 0.999), max-abs / bound {rel:.4f} (<= 1)")

        # ---- 3. identical batch items; a twin case also against the plan without the twin prefix
        same_inp = UC.inputs(c, same_items=True)
        side_same = None
        if side is not None:                                       # the side network again on the equal items: its outputs feed this one
            sn = c.nets[0]
            _load(side, sn, c, same_inp, None)
            side.run_step(use_graph=False)
            side_same = side
        _load(rt, n, c, same_inp, side_same)
        w_bits, _ = _walk(rt, dtype)
        all_bits = dict(_block_bits(rt), **w_bits)
        items = {t[0]: t[1].B if hasattr(t[1], "B") else (t[1].shape[0] if len(t[1].shape) == 4 else 1) for t in taps}
        uneven = [k for k, v in all_bits.items() if items[k] > 1 and not bool((v.view(items[k], -1) == v.view(items[k], -1)[:1]).all())]
        batch_ok = not uneven
        if c.twin:
            _ensure(rt, n, c, False)
            assert not rt.twin
            _load(rt, n, c, same_inp, side_same)
            p_bits, _ = _walk(rt, dtype)
            plain = dict(_block_bits(rt), **p_bits)
            # conv_in runs single-pass in both plans (the twin store takes no split-K; asserted for the plain one): the K walk of a
            # row does not depend on the row count, so the full, twice-stored tensor must have the plain plan's bits
            conv_in = [t[1] for t in rt.lay["taps"] if t[0] == "conv_in"][0]
            assert not conv_in.producer.workspace, "the plain plan's conv_in runs split-K: its bits need not be the twin plan's"
            off = [k for k in ("temb_all", "conv_in") if not torch.equal(all_bits[k], plain[k])]
            TWIN_EQUAL[c.id] = (sum(int(torch.equal(v, plain[k][:v.numel()])) for k, v in all_bits.items()), len(all_bits))
            batch_ok = batch_ok and set(plain) == set(all_bits) and not off
            if off:
                uneven += off
        if not batch_ok:
            fails.append(f"{tag}: identical batch items give different bits, first at {uneven[:1]}")

        key = (f"{n.kind}({n.wiring})", c.fmt, "twin" if c.twin else "plain")
        p, b = EQUAL.get(key, (0, 0))
        EQUAL[key] = (p + int(poison_ok), b + int(batch_ok))
        e = E2E.get(key, (1.0, 0.0))
        E2E[key] = (min(e[0], cos), max(e[1], rel))

        # the side network's outputs of the case's own inputs feed the next network
        if n.kind != "unet":
            _load(rt, n, c, inp, None)
            rt.run_step(use_graph=False)
            torch.cuda.synchronize()
            assert _same(_outputs(rt, n), out)
            side = rt
    assert not fails, "\n".join(fails)
    DONE.add(c.id)
