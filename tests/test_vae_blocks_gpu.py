"""-m gpu: both VAEs block by block at the checkpoints' widths (tests/vae_cases.py: the cases, the teacher-forced float64
references, the derived gates; proof that the probes can fail: tests/test_vae_probes.py).

Every case (model, direction, shape, format) runs the product entry point (`vae.decode` / `vae.encode`) and reads the taps the
plan recorded (`rt.lay["taps"]`):

  1. every tap, every element, against the block evaluated in float64 on the HIP path's own bits of its input taps, under the
     block's derived gate.  Encoder taps are compared in the plan's rotated frame (the reference is rotated).  The tensor in
     front of a conditioned blend is overwritten in place: the plan is replayed launch by launch and the sample is copied in
     front of every pp_mask_blend (the replay's taps must equal the product run's bit for bit).  conv_out: channel 3 of the
     buffer is exactly 0 and only [:, :3] is returned; the moments after the flip-back: mean and logvar gated separately.
     Inside the attention: the plan's prefix up to its last pp_softmax_rows leaves S and P of the last image; P against the
     float64 softmax of that S over the n real columns under the softmax gate, rows summing to 1 within the gates' sum, pad
     columns exact zeros.
  2. whole-plan poison: every byte of the arena except the input buffers (x_in; img8 and the mask planes of the conditioned
     decode) is filled with NaN bit patterns; the run is repeated: the output and every tap must have the same bits.
  3. identical batch items: a batch of equal items must give bit-identical items in every tap: the order in which an element
     is accumulated does not depend on its row's position, the statistics are per item in a fixed order, pp_mask_blend's
     accumulators are integers.  (Held on the MI355X in every case; a difference would be a batch offset, a pad-row read or
     an accumulator slot.)
  4. end to end: the image / the moments against the free-running float64 chain under the gate of the existing parity tests
     (cosine >= 0.999, max-abs <= 5 % of max|ref|), printed next to the per-block figures.

After a whole run of the file profiles/vae_blocks_achieved.txt is rewritten: per (model, direction, format, block kind) the
worst achieved / gate and where, the number of bit-equal poison and batch checks, the wall time; no threshold is pinned on it.
"""
import os
import sys
import time

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import vae_cases as VC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402

DEV = "cuda"
NAN16 = 0x7FC1                      # a NaN in bf16 and fp16; two of them a NaN in fp32
WORST, EQUAL, E2E, DONE, T0 = {}, {}, {}, set(), [None]
_MODELS = {}
ACHIEVED_HEADER = (
    "# tests/test_vae_blocks_gpu.py on one MI355X: per (model, direction, format, block kind) the largest achieved error / gate over\n"
    "# every element of every tap of that kind (gates: tests/vae_cases.py, derived, not fitted: the ratio shows the slack, no\n"
    "# threshold is pinned on it) and the case and tap it was met at; per (model, direction, format) the number of bit-equal\n"
    "# whole-plan poison runs and identical-item runs, and the end-to-end figures of the same runs against the free-running\n"
    "# float64 chain (gate 0.999 / 0.05).  The wall time is rounded to 30 s, at least 30 s, so that this tracked file is the same\n"
    "# after every run.\n")


@pytest.fixture(scope="module", autouse=True)
def _achieved():
    T0[0] = time.time()
    yield
    _MODELS.clear()
    if DONE != {c.id for c in VC.CASES}:
        return
    try:
        with open(os.path.join(ROOT, "profiles", "vae_blocks_achieved.txt"), "w") as f:
            f.write(ACHIEVED_HEADER)
            for key in sorted(WORST):
                r, where = WORST[key]
                f.write(f"[vae blocks] {key[0]} {key[1]} {key[2]} {key[3]}: worst error / gate {r:.3f} at {where}\n")
            for key in sorted(EQUAL):
                p, b = EQUAL[key]
                cos, rel = E2E[key]
                f.write(f"[vae blocks] {key[0]} {key[1]} {key[2]}: {p} poison runs bit-equal, {b} identical-item runs bit-equal; "
                        f"end to end worst cosine {cos:.6f}, max-abs / max {rel:.4f}\n")
            wall = max(30, 30 * round((time.time() - T0[0]) / 30))
            f.write(f"# {len(VC.CASES)} cases; wall time of the file about {wall} s\n")
    except OSError:
        pass


def _model(c):
    key = (c.model, c.fmt)
    if key not in _MODELS:
        _MODELS.clear()                                               # one set of device weights at a time
        from powerpaint_amd import models as PM
        cfg = VC.CFG[c.model]
        if c.model == "kl":
            vae = PM.AutoencoderKL(device=DEV)
        else:
            t = ("DownEncoderBlock2D",) * 4, ("UpDecoderBlock2D",) * 4
            vae = PM.AsymmetricAutoencoderKL(down_block_types=t[0], down_block_out_channels=cfg["down"],
                                             layers_per_down_block=cfg["layers_down"], up_block_types=t[1],
                                             up_block_out_channels=cfg["up"], layers_per_up_block=cfg["layers_up"], device=DEV,
                                             dtype=VC.FMT[c.fmt])
        vae.load_state_dict(VC.state_dict(c.model))
        _MODELS[key] = vae
    return _MODELS[key]


def _rt(vae, c):
    return vae._enc if c.direction == "encode" else (vae._dec_cond if c.cond else vae._dec)


def _run(vae, c, inp):
    """The product entry point -> the image [B, 3, H, W] or cat(mean, logvar) [B, 8, h, w], a copy."""
    if c.direction == "encode":
        d = vae.encode(inp["img"].to(DEV)).latent_dist
        out = torch.cat([d.mean, d.logvar], 1)
    elif c.cond:
        out = vae.decode(inp["z"].to(DEV), image=inp["image"].to(DEV), mask=inp["mask"].to(DEV), return_dict=False)[0]
    else:
        out = vae.decode(inp["z"].to(DEV), return_dict=False)[0]
    torch.cuda.synchronize()
    return out.clone()


def _bytes(rt, t):
    return rt.arena.view(t.ptr, (t.B, t.nbytes // t.B), torch.uint8).clone()


def _value(rt, t, dtype):
    """a tap as NCHW float64 on the host"""
    if not hasattr(t, "rows"):                                        # the decoder's fp32 NCHW image
        return rt.arena.view(t.ptr, (t.B, t.C, t.H, t.W), torch.float32).double().cpu()
    return rt.arena.view(t.ptr, (t.B, t.H, t.W, t.C), dtype).permute(0, 3, 1, 2).double().cpu()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _replay(rt, upto=None, before=None):
    """the plan launch by launch; before(i, name): called in front of launch i"""
    for i, (fn, args, name) in enumerate(rt.plan.calls[:upto]):
        if before is not None:
            before(i, name)
        L.check(fn(*args, _stream()), name)
    torch.cuda.synchronize()


def _poison(rt, c):
    keep = [rt.lay["x_in"]] + ([rt.lay["img8"]] if c.cond else [])
    saved = [(t, rt.arena.view(t.ptr, (t.nbytes,), torch.uint8).clone()) for t in keep]
    if c.cond:
        B, H, W = rt.key
        mask = rt.arena.view(rt.lay["mask"], (B * 64 * H * W,), torch.float32)
        msaved = mask.clone()
    rt.arena.buf.view(torch.int16).fill_(NAN16)
    for t, b in saved:
        rt.arena.view(t.ptr, (t.nbytes,), torch.uint8).copy_(b)
    if c.cond:
        mask.copy_(msaved)
    torch.cuda.synchronize()


def _record(c, res):
    for name, kind, r, where in res:
        key = (c.model, c.direction, c.fmt, kind)
        if key not in WORST or r > WORST[key][0]:
            WORST[key] = (r, f"{c.id} {name} {where}")


@pytest.mark.parametrize("c", VC.CASES, ids=lambda c: c.id)
def test_case(c):
    cfg, sd, dtype = VC.CFG[c.model], VC.state_dict(c.model), VC.FMT[c.fmt]
    vae = _model(c)
    rt = _rt(vae, c)
    inp = VC.inputs(c)
    out = _run(vae, c, inp)
    taps = rt.lay["taps"]
    names = [s.name for s in VC.steps(cfg, c.direction, c.cond, c.model == "asym")]
    assert [t[0] for t in taps] == names
    bits = {t[0]: _bytes(rt, t[1]) for t in taps}
    val = {t[0]: _value(rt, t[1], dtype) for t in taps}
    extra = dict(x_in=_value(rt, rt.lay["x_in"], dtype), pre_blend={})
    fails = []

    # ---- 1. every tap against its teacher-forced reference
    if c.model == "asym" and c.direction == "decode":
        blends = [t for t in taps if len(t) == 3]
        at = [i for i, call in enumerate(rt.plan.calls) if call[2] == "mask_blend"]
        assert len(at) == len(blends) == 5
        front = {}

        def before(i, name):
            if name == "mask_blend":
                front[blends[at.index(i)][0]] = _value(rt, blends[at.index(i)][1], dtype)

        _replay(rt, before=before)
        assert all(torch.equal(_bytes(rt, t[1]), bits[t[0]]) for t in taps), "the launch-by-launch replay differs from the run"
        extra["pre_blend"] = front
        if c.cond:
            B, H, W = rt.key
            extra["img8"] = _value(rt, rt.lay["img8"], dtype)
            extra["mask"] = rt.arena.view(rt.lay["mask"], (B, 1, 8 * H, 8 * W), torch.float32).double().cpu()
            for st in VC.steps(cfg, c.direction, c.cond, True):
                if st.kind == "blend":
                    val[st.src] = front[st.name]                       # the tap in front of a blend, before it was overwritten
        else:
            assert all(torch.equal(front[t[0]], val[t[0]]) for t in blends), "a statistics-only blend wrote its tensor"
    res = VC.check_chain(c, cfg, sd, val, extra)
    _record(c, res)
    for name, kind, r, where in res:
        print(f"[vae blocks] {c.id} {kind:10s} {name}: error / gate {r:.3f} at {where}")
        if not r <= 1.0:
            fails.append(f"tap {name} ({kind}): error / gate {r:.3f} at {where}")
    if c.direction == "decode":
        img = val["decoder.conv_out"]
        assert out.shape == (c.B, 3, 8 * c.H, 8 * c.W) and torch.equal(out.double().cpu(), img[:, :3])
        assert torch.count_nonzero(img[:, 3]) == 0, "channel 3 of the conv_out buffer is not exactly 0"
    else:
        st = [s for s in VC.steps(cfg, c.direction) if s.name == "quant_conv"][0]
        ref, gate = VC.gate_step(VC.Ctx(dtype, cfg["groups"]), sd, st, val, extra)
        ref, gate, got = ref.flip(2, 3), gate.flip(2, 3), out.double().cpu()
        assert torch.equal(got[:, :4], val["quant_conv"].flip(2, 3)[:, :4])
        r_mean = VC.where_worst(got[:, :4], ref[:, :4], gate[:, :4])
        r_logvar = VC.where_worst(got[:, 4:], ref[:, 4:].clamp(-30.0, 20.0), gate[:, 4:])
        _record(c, [("mean", "moments-mean") + r_mean, ("logvar", "moments-logvar") + r_logvar])
        print(f"[vae blocks] {c.id} moments: mean error / gate {r_mean[0]:.3f}, logvar {r_logvar[0]:.3f}")
        if not (r_mean[0] <= 1.0 and r_logvar[0] <= 1.0):
            fails.append(f"moments after the flip-back: mean {r_mean}, logvar {r_logvar}")

    # ---- inside the attention: S and P of the last image
    last = max(i for i, call in enumerate(rt.plan.calls) if call[2] == "softmax_rows")
    s_ptr, npad, n, _, scale, p_ptr = rt.plan.calls[last][1][:6]
    assert n == (c.H * c.W if c.direction == "decode" else c.H * c.W // 64) and npad == -(-n // 64) * 64
    _replay(rt, upto=last + 1)
    S = rt.arena.view(s_ptr, (n, npad), torch.float32).double().cpu()
    P = rt.arena.view(p_ptr, (n, npad), dtype).double().cpu()
    width = cfg["down" if c.direction == "encode" else "up"][-1]
    assert abs(scale - width ** -0.5) < 1e-12
    p64, gate = VC.softmax_own(VC.Ctx(dtype), S[:, :n], width ** -0.5, n)
    r_p = VC.where_worst(P[:, :n], p64, gate)
    r_sum = float(((P[:, :n].sum(1) - 1.0).abs() / gate.sum(1)).max())
    _record(c, [("P", "softmax") + r_p])
    print(f"[vae blocks] {c.id} softmax interior: error / gate {r_p[0]:.3f}, row sums {r_sum:.3f}, {npad - n} pad columns")
    if not (r_p[0] <= 1.0 and r_sum <= 1.0):
        fails.append(f"P of the last image: error / gate {r_p}, row sums {r_sum}")
    if torch.count_nonzero(P[:, n:]) != 0:
        fails.append("pad columns of P are not exact zeros")

    # ---- 2. whole-plan poison
    _poison(rt, c)
    assert all(bool(torch.isnan(rt.arena.view(t[1].ptr, (t[1].nbytes // 2,), dtype)).all()) for t in taps), "the poison did not land"
    assert torch.equal(_value(rt, rt.lay["x_in"], dtype), extra["x_in"])
    again = _run(vae, c, inp)
    differ = [t[0] for t in taps if not torch.equal(_bytes(rt, t[1]), bits[t[0]])]
    poison_ok = torch.equal(again.view(torch.int32), out.view(torch.int32)) and not differ
    if not poison_ok:
        fails.append(f"poisoned arena: the output or taps differ, first {differ[:1]}: the plan reads memory it did not write")

    # ---- 3. identical batch items
    same = _run(vae, c, VC.inputs(c, same_items=True))
    uneven = [t[0] for t in taps if not bool((_bytes(rt, t[1]) == _bytes(rt, t[1])[:1]).all())]
    batch_ok = not uneven and bool((same == same[:1]).all())
    if not batch_ok:
        fails.append(f"identical batch items give different bits, first at {uneven[:1]}")

    # ---- 4. end to end, the same run
    want = VC.free_run(c, cfg, sd, extra)
    if c.direction == "encode":
        want = torch.cat([want[:, :4], want[:, 4:].clamp(-30.0, 20.0)], 1)
    got = out.double().cpu()
    cos = F.cosine_similarity(got.flatten(), want.flatten(), dim=0).item()
    rel = ((got - want).abs().max() / want.abs().max()).item()
    print(f"[vae blocks] {c.id} end to end: cosine {cos:.6f}, max-abs / max {rel:.4f}; worst block {max(r[2] for r in res):.3f}")
    if not (cos >= 0.999 and rel <= 0.05):
        fails.append(f"end to end: cosine {cos:.6f} (>= 0.999), max-abs / max {rel:.4f} (<= 0.05)")

    key = (c.model, c.direction + ("-cond" if c.cond else ""), c.fmt)
    p, b = EQUAL.get(key, (0, 0))
    EQUAL[key] = (p + int(poison_ok), b + int(batch_ok))
    e = E2E.get(key, (1.0, 0.0))
    E2E[key] = (min(e[0], cos), max(e[1], rel))
    assert not fails, "\n".join(fails)
    DONE.add(c.id)
