"""GPU: AutoencoderTiny on the HIP path against its float64 restatement (tests/taesd_cases.py), synthetic weights, bf16 and
fp16, batch 2; decode at 8 x 12 and 5 x 7 latents, encode at 64 x 96 and 24 x 40 images.

Per launch.  Every tap (the output of every launch) is compared with the float64 value e recomputed from that launch's STORED
inputs (the taps in front of it, the parameters as packed).  A conv sums 576 products, a bias and a residual in fp32: whatever
the order, |r32 - e| <= E32 = 578 * 2^-24 * (sum |w||x| + |b| + |res|) (577 additions at most and one rounding per product,
(1 + u)^578 - 1 to first order); ReLU is 1-Lipschitz and exact; the stored value is r32 rounded to nearest in the 16-bit format
(unit roundoff u16 = 2^-8 bf16, 2^-11 fp16; fp16 subnormal spacing 2^-24):
        |stored - e| <= E32 + u16 (|e| + E32) + 2^-25.
The two last convs store fp32 (u16 -> 2^-24).  The ReLU launch must reproduce max(x, 0) exactly.  The pack launch rounds
(x + 1) / 2 (two exact-or-once-rounded fp32 operations) or 3 tanh(z / 3) (a division, tanhf, a product: E32 = 8 * 2^-24 |e|
covers tanhf's few-ulp error; t sech^2 t <= tanh t keeps the division's rounding below one more ulp of the result).

End to end.  The GPU's max-abs error against the PURE float64 model is at most twice that of the rounded restatement (the
same model with every stored tensor rounded to the format, computed on the CPU in the same test): the plan rounds where the
restatement rounds, and a tie that falls the other way propagates as an independent error of the same size.  The achieved
values and cosines are printed and appended to profiles/taesd_parity_achieved.txt before anything is asserted.
"""
import os

import pytest
import torch
import torch.nn.functional as F

import taesd_cases as TC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
U16 = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
U32 = 2.0 ** -24
CFG = TC.DEFAULT


def record(line: str):
    print(line)
    try:
        with open(os.path.join(ROOT, "profiles", "taesd_parity_achieved.txt"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


_MODELS = {}


def model(dt):
    """(AutoencoderTiny on the GPU, its fp32 state dict) -- one per format for the whole file."""
    if dt not in _MODELS:
        from powerpaint_amd.models import AutoencoderTiny
        vae = AutoencoderTiny(device="cuda", dtype=DT[dt])
        sd = vae.net.synthetic_state_dict(seed=11)
        vae.load_state_dict(sd)
        _MODELS[dt] = (vae, sd)
    return _MODELS[dt]


def _inputs(direction, h, w, B=2, seed=5):
    g = torch.Generator().manual_seed(seed + h)
    if direction == "decode":
        return torch.randn(B, 4, h, w, generator=g) * 3.0
    return torch.rand(B, 3, h, w, generator=g) * 2 - 1


def _runtime(vae, direction):
    return vae._dec if direction == "decode" else vae._enc


def _stored(rt, tap, dtype):
    """A tap's bytes as float64 NCHW."""
    t = tap[1]
    if hasattr(t, "rows"):
        return rt.arena.view(t.ptr, (t.B, t.H, t.W, t.C), dtype).cpu().double().permute(0, 3, 1, 2).contiguous()
    return rt.arena.view(t.ptr, (t.B, t.C, t.H, t.W), torch.float32).cpu().double()


def _bound(e, e32, u16):
    return e32 + u16 * (e.abs() + e32) + 2.0 ** -25


def _conv_case(sdr, pre, a, stride=1, up=False, res=None, relu=False, scale_out=False):
    """float64 value and E32 of one conv launch on the stored input `a`; scale_out: the decoder's folded last conv."""
    w, b = sdr[pre + ".weight"], sdr.get(pre + ".bias")
    if scale_out:
        w, b = 2 * w, (2 * b.float() - 1).double()
    if up:
        a = F.interpolate(a, scale_factor=2, mode="nearest")
    a = a[:, :w.shape[1]]
    e = F.conv2d(a, w, b, stride=stride, padding=1)
    s = F.conv2d(a.abs(), w.abs(), None if b is None else b.abs(), stride=stride, padding=1)
    if res is not None:
        e, s = e + res, s + res.abs()
    return (F.relu(e) if relu else e), 578 * U32 * s


def check_taps(rt, side, dt, sd, x):
    """Walk the taps of the run that just finished; returns the worst achieved error / bound."""
    dtype, u16 = DT[dt], U16[dt]
    sdr = TC.rounded_weights(sd, dtype)
    taps = list(rt.lay["taps"])
    assert len(taps) == len(rt.plan.calls)
    worst = [0.0, ""]

    def within(name, got, e, e32, u):
        ratio = ((got - e).abs() / _bound(e, e32, u)).max().item()
        if ratio > worst[0]:
            worst[:] = [ratio, name]
        assert ratio <= 1.0, f"{name}: error / bound {ratio:.3f}"

    name, tap = taps[0][0], _stored(rt, taps[0], dtype)
    assert name == "pack" and tap.shape[1] == 8 and bool((tap[:, x.shape[1]:] == 0).all())
    xd = x.double()
    if side == "encoder":
        within(name, tap[:, :3], (xd + 1) / 2, U32 * ((xd + 1) / 2).abs(), u16)
    else:
        e = 3 * torch.tanh(xd / 3)
        within(name, tap[:, :4], e, 8 * U32 * e.abs(), u16)
    cur, i = tap, 1
    for kind, idx in TC.layers(side, CFG):
        pre = f"{side}.layers.{idx}"
        if kind == "up":
            continue
        if kind == "block":
            blk_in = cur
            for c, res in ((0, None), (2, None), (4, blk_in)):
                assert taps[i][0] == f"{pre}.conv.{c}"
                got = _stored(rt, taps[i], dtype)
                e, e32 = _conv_case(sdr, taps[i][0], cur, res=res, relu=True)
                within(taps[i][0], got, e, e32, u16)
                cur, i = got, i + 1
            continue
        assert taps[i][0] == pre
        got = _stored(rt, taps[i], dtype)
        if kind == "relu":
            assert torch.equal(got, F.relu(cur)), pre
        elif kind == "out":
            n = CFG["latent_channels"] if side == "encoder" else CFG["out_channels"]
            e, e32 = _conv_case(sdr, pre, cur, scale_out=(side == "decoder"))
            within(pre, got[:, :n], e, e32, U32)
            assert bool((got[:, n:] == 0).all())
        else:
            e, e32 = _conv_case(sdr, pre, cur, stride=2 if kind == "down" else 1, up=(kind == "conv_up"))
            within(pre, got, e, e32, u16)
        cur, i = got, i + 1
    assert i == len(taps)
    return worst


def _reference(direction, sd, x, dtype):
    xd = x.double()
    f = TC.decode if direction == "decode" else TC.encode
    with torch.no_grad():
        pure = f(TC.as_double(sd), CFG, xd)
        rounded = f(TC.rounded_weights(sd, dtype), CFG, xd, TC.rounder(dtype))
    return pure, rounded


CASES = [("decode", h, w) for h, w in TC.DECODE_SHAPES] + [("encode", h, w) for h, w in TC.ENCODE_SHAPES]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("direction,h,w", CASES)
def test_every_launch_and_the_whole_plan_against_float64(dt, direction, h, w):
    vae, sd = model(dt)
    rt = _runtime(vae, direction)
    x = _inputs(direction, h, w)
    if direction == "decode":
        got = vae.decode(x.cuda(), return_dict=False)[0]
        assert got.shape == (2, 3, 8 * h, 8 * w) and got.dtype == torch.float32
    else:
        got = vae.encode(x.cuda()).latents
        assert got.shape == (2, 4, h // 8, w // 8) and got.dtype == torch.float32
    torch.cuda.synchronize()
    worst = check_taps(rt, direction + "r", dt, sd, x)
    pure, rounded = _reference(direction, sd, x, DT[dt])
    g = got.cpu().double()
    err_gpu, err_cpu = (g - pure).abs().max().item(), (rounded - pure).abs().max().item()
    cos = F.cosine_similarity(g.flatten(), pure.flatten(), dim=0).item()
    cos_r = F.cosine_similarity(rounded.flatten(), pure.flatten(), dim=0).item()
    record(f"{direction} {h}x{w} {dt}: max-abs vs float64 GPU {err_gpu:.4e} rounded restatement {err_cpu:.4e} "
           f"(max |ref| {pure.abs().max().item():.3f}), cosine GPU {cos:.7f} rounded {cos_r:.7f}; "
           f"worst launch error / bound {worst[0]:.3f} at {worst[1]}")
    assert err_gpu <= 2 * err_cpu, f"GPU {err_gpu:.4e} > 2 x rounded restatement {err_cpu:.4e}"
    # the same call again, and the tuple / attribute forms: the same bits
    again = vae.decode(x.cuda()).sample if direction == "decode" else vae.encode(x.cuda(), return_dict=False)[0]
    assert torch.equal(again, got)


def _bits(rt, x):
    return rt.run(x.cuda()).clone()


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("direction,h,w", [("decode", 5, 7), ("encode", 24, 40)])
def test_same_bits_on_a_poisoned_arena_and_at_other_batch_sizes(dt, direction, h, w):
    vae, _ = model(dt)
    rt = _runtime(vae, direction)
    x = _inputs(direction, h, w, B=2, seed=9)
    want = _bits(rt, x)
    taps = [rt.arena.view(t[1].ptr, (t[1].nbytes,), torch.uint8).clone() for t in rt.lay["taps"]]
    # NaNs everywhere (the 16-bit pattern 0xFFFF is a NaN in both formats and a NaN as fp32): run() writes the input staging
    # buffer itself, the plan must write everything else it reads
    rt.arena.buf.fill_(0xFF)
    got = _bits(rt, x)
    assert torch.equal(got, want) and not bool(torch.isnan(got).any())
    for t, before in zip(rt.lay["taps"], taps):
        assert torch.equal(rt.arena.view(t[1].ptr, (t[1].nbytes,), torch.uint8), before), t[0]
    # item by item at batch 1, and in last place of a batch of 3
    for i in range(2):
        assert torch.equal(_bits(rt, x[i:i + 1])[0], want[i]), f"item {i} alone"
    other = _inputs(direction, h, w, B=2, seed=10)
    three = _bits(rt, torch.cat([other, x[1:2]]))
    assert torch.equal(three[2], want[1]) and not torch.equal(three[0], want[0])


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_round_trip_forward_and_chunking(dt):
    from powerpaint_amd.models import autoencoder_tiny as M
    vae, sd = model(dt)
    x = _inputs("encode", 24, 40, B=3, seed=3)
    lat = vae.encode(x.cuda()).latents
    out = vae.decode(lat).sample                                               # decode(encode(x).latents) runs
    assert lat.shape == (3, 4, 3, 5) and out.shape == (3, 3, 24, 40) and bool(torch.isfinite(out).all())
    fwd = vae(x.cuda()).sample
    assert torch.equal(fwd, vae.decode(TC.quantise(lat)).sample)
    old = M.MAX_PIXELS
    try:
        M.MAX_PIXELS = 24 * 40                                                 # one image per plan run
        assert vae._chunks(3, 24 * 40) == [(0, 1), (1, 2), (2, 3)]
        assert torch.equal(vae.encode(x.cuda()).latents, lat) and torch.equal(vae.decode(lat).sample, out)
    finally:
        M.MAX_PIXELS = old
    with pytest.raises(ValueError):
        vae.decode(torch.zeros(1, 3, 4, 4, device="cuda"))
    with pytest.raises(ValueError):
        vae.encode(torch.zeros(1, 4, 8, 8, device="cuda"))
    g = torch.Generator(device="cuda").manual_seed(1)
    state = g.get_state().clone()
    vae.decode(lat, generator=g)
    assert torch.equal(g.get_state(), state)                                   # decode's generator is accepted and not touched
