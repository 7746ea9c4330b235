"""-m gpu: the small and step kernels of csrc/small.hip through the C ABI on the matrix of tests/small_cases.py.  Derivations:
that module's docstring; proof that every probe can fail: tests/test_small_probes.py.

  E cases    every output window EQUALS the fp64 reference cast once to its format, bit for bit;
  R cases    |out - ref| <= u |ref| + n_r 2^-24 A (the derived gate, nothing fitted);
  every case outputs are windows of sentinel-filled buffers (guards in front and behind, pad columns where the ABI has a
             stride); every byte outside a window is unchanged after the launch; inputs carry poisoned pads and tails, NaN
             where they must not be read;
  step cases with a ticket are launched twice in a row: after each launch the ticket is 0 and the counter has moved by exactly
             one; without a ticket the counter does not move;
  refusals   carry the stated code and happen before any launch: nothing at all is written.

A failure names the case, the first bad index and the border it lies on.  After a whole run of the file
profiles/small_exact_achieved.txt is rewritten: per (kernel, format, regime) the worst achieved / gate and the number of
bit-equal cases; no threshold is pinned on it.
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
import small_cases as SC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402

DEV = "cuda"
WORST, COUNT, T0 = {}, {}, [None]
SILU = L.PP_ACT_SILU
ACHIEVED_HEADER = ("# tests/test_small_exact_gpu.py on one MI355X: per (kernel, format, regime) the largest achieved error / gate of the R\n"
                   "# cases (gates: tests/small_cases.py, derived from rounding counts; expf / cosf / sinf / exp2f bounded by 2 ulp each, an\n"
                   "# assumption stated there; worst case, not fitted: the ratio shows the slack, no threshold is pinned on it) and the number\n"
                   "# of E cases that held bit equality.  The wall time is rounded to 5 s, at least 5 s, so that this tracked file is the\n"
                   "# same after every run.\n")


@pytest.fixture(scope="module", autouse=True)
def _achieved():
    T0[0] = time.time()
    yield
    if sum(COUNT.values()) != sum(len(SC.case_dtypes(c)) for c in SC.CASES if c.probe != "X") + len(SC.GN_CONV_CASES) * len(SC.DTYPES):
        return
    try:
        with open(os.path.join(ROOT, "profiles", "small_exact_achieved.txt"), "w") as f:
            f.write(ACHIEVED_HEADER)
            for key in sorted(COUNT):
                line = f"[small exact] {key[0]} {key[1]} {key[2]}: {COUNT[key]} cases"
                line += f", worst error / gate {WORST[key][0]:.3f} at {WORST[key][1]}" if key in WORST else ", bit-equal"
                f.write(line + "\n")
            wall = max(5, 5 * round((time.time() - T0[0]) / 5))          # (to 5 s: the tracked file stays as committed)
            f.write(f"# {len(SC.CASES)} cases of the matrix and {len(SC.GN_CONV_CASES)} of the fused conv_out, {sum(COUNT.values())} "
                    f"(case, format) runs checked; wall time of the file about {wall} s\n")
    except OSError:
        pass


def _family(c):
    if c.kernel == "conv_out":
        return "conv_out-" + ("mfma" if SC.conv_out_mfma(c.p["cin"]) else "scalar")
    if c.kernel == "step":
        return "step-" + c.p["kind"]
    if c.kernel == "mask":
        return f"mask_prep-mode{c.p['mode']}"
    return c.kernel


def _regime(c):
    return c.probe + ("-" + c.p["regime"] if c.kernel == "softmax" else "")


def _ptr(b, off: int = 0):
    return None if b is None else b.full.data_ptr() + b.base * b.full.element_size() + off


def _dev(x):
    if isinstance(x, SC.Buf):
        return x.to(DEV)
    if isinstance(x, list):
        return [_dev(v) for v in x]
    return x


def _launch(c, i, o, dt, j=0):
    """one call of the library for case `c`: inputs `i`, output windows `o` (both on the device); returns the error code"""
    lib, p, st = L.lib(), c.p, torch.cuda.current_stream().cuda_stream
    k = c.kernel
    if k == "conv_direct":
        return lib.pp_conv3x3_direct(_ptr(i["x"]), p["B"], p["H"], p["W"], p["cin"], _ptr(i["w"]), _ptr(i["bias"]), p["cout"],
                                     p["stride"], int(bool(p.get("silu"))), _ptr(i["add"]), _ptr(o["out"]), dt, st)
    if k == "conv_out":
        return lib.pp_conv3x3_smallcout(_ptr(i["x"]), p["B"], p["H"], p["W"], p["cin"], _ptr(i["w"]), _ptr(i["bias"]), 4,
                                        _ptr(o["out"]), dt, st)
    if k == "to_nhwc":
        return lib.pp_nchw_to_nhwc(_ptr(i["src"]), {"f32": 0, "bf16": 1, "fp16": 2}[p["src"]], p["B"], p["c"], p["hw"], p["bmod"],
                                   _ptr(o["dst"]), p["ldc"], p["c0"], dt, st)
    if k == "to_nchw":
        return lib.pp_nhwc_to_nchw(_ptr(i["src"]), p["B"], p["c"], p["hw"], _ptr(o["dst"]), 0 if p["dst"] == "f32" else dt, dt, st)
    if k == "add":
        return lib.pp_add_bf16(_ptr(i["a"]), _ptr(i["b"]), _ptr(o["out"]), p["n"], dt, st)
    if k == "skinny":
        return lib.pp_linear_skinny(_ptr(i["x"]), p["rows"], p["K"], _ptr(i["w"]), _ptr(i["bias"]), p["N"], _ptr(o["out"]),
                                    o["out"].ld, SILU if p.get("act_in") else 0, SILU if p.get("act_out") else 0, dt, st)
    if k == "temb":
        return lib.pp_timestep_embedding(_ptr(i["t"]), p["rows"], p["dim"], _ptr(o["out"]), st)
    if k == "softmax":
        return lib.pp_softmax_rows(_ptr(i["s"], p.get("s_off", 0)), p["lds"], p["rows"], p["n"], p["scale"],
                                   _ptr(o["p"], p.get("p_off", 0)), p["ldp"], dt, st)
    if k == "splice":
        return lib.pp_embed_splice(_ptr(i["table"]), _ptr(i["ext"]), _ptr(i["src"]), _ptr(o["out"]), p["n_rows"], p["row_bytes"], st)
    if k == "step_head":
        args = (_ptr(i["table"]), _ptr(i["step"]), _ptr(o["temb"]), p["row_floats"], _ptr(i["lat"]), p["B"], p["c"], p["hw"], p["bmod"],
                _ptr(o["x"]), p["ldc"], p["c0"], dt, _ptr(o["z"]), p["nz"])
        return lib.pp_step_head_scaled(*args, _ptr(i["div"]), st) if p["scaled"] else lib.pp_step_head(*args, st)
    if k == "zero":
        return lib.pp_zero_u64(_ptr(o["z"]), p["n"], st)
    if k == "blend":
        return lib.pp_latent_blend(_ptr(o["x"]), _ptr(i["x0"]), _ptr(i["m"]), _ptr(i["z"]), _ptr(i["tab"]), _ptr(i["step"]), p["B"],
                                   p["C"], p["hw"], st)
    if k == "mask":
        return lib.pp_mask_prep(p["mode"], _ptr(i["a"]), _ptr(i["b"]), _ptr(o["out"]), p["B"], p["c"], p["h"], p["w"], p.get("ho", 0),
                                p.get("wo", 0), st)
    assert k == "step"
    kind, n, cfg = p["kind"], p["n"], p["cfg"]
    tk = _ptr(o["ticket"]) if p["ticket"] else None
    head = (_ptr(i["eps"][j]), cfg, i["gs"], _ptr(o["x"]))
    tail = (_ptr(i["table"]), _ptr(o["step"]), tk, st)
    if kind in ("ddim", "dpm", "pndm", "unipc"):
        return lib.pp_cfg_sched_step(*head, _ptr(o.get("state")), n, ("ddim", "dpm", "pndm", "unipc").index(kind), *tail)
    if kind == "lcm":
        return lib.pp_cfg_lcm_step(*head, _ptr(i["z"][j]), n, *tail)
    if kind == "sigma":
        return lib.pp_cfg_sigma_step(*head, _ptr(i["z"][j]), n, *tail)
    if kind == "ksampler":
        return lib.pp_cfg_ksampler_step(*head, _ptr(o["state"]), _ptr(i["z"][j]), n, *tail)
    return lib.pp_ddim_variance_noise(_ptr(o["x"]), _ptr(i["z"][j]), n, _ptr(i["table"]), _ptr(o["step"]), st)


def _check_outside(c, t, o, what):
    for name, b in o.items():
        assert SC.outside_clean(b), (what, name, "bytes outside the window were written")
        cols = t.get("cols", {}).get(name)
        if cols is not None:                               # the pad columns of a row stride, the columns in front of c0
            keep = torch.ones(b.cols, dtype=torch.bool, device=DEV)
            keep[cols[0]:cols[0] + cols[1]] = False
            assert bool((SC.bits(b.view)[:, keep] == SC.SENT[b.full.element_size()]).all()), (what, name, "pad columns were written")


def _run(c, dtype, fmt, tamper=None, after=None, record=True):
    """tamper(t) / after(o): hooks of the negative controls below"""
    what = f"{c.id} {fmt}"
    t = SC.build(c, dtype)
    if tamper:
        tamper(t)
    dt = L.dtype_code(dtype) if dtype != torch.float32 else 0
    i = {k: _dev(v) for k, v in t["inp"].items()}
    o = {k: v.to(DEV) for k, v in t["out"].items()}
    if c.probe == "X":
        rc = _launch(c, i, o, dt)
        torch.cuda.synchronize()
        assert rc == c.expect, (what, "refused with", L.PP_ERR.get(rc, rc), "expected", L.PP_ERR[c.expect])
        for name, b in o.items():                          # refused before any launch: nothing was written at all
            assert bool((SC.bits(b.full) == SC.SENT[b.full.element_size()]).all()), (what, name, "a refused request wrote")
        return
    for j in range(t.get("launches", 1)):
        rc = _launch(c, i, o, dt, j)
        torch.cuda.synchronize()
        assert rc == 0, (what, "launch", j, L.PP_ERR.get(rc, rc), L.lib().pp_last_error().decode())
        if c.kernel == "step":
            moved = int(o["step"].view[0, 0]) - SC.STEP_FIRST
            assert int(o["ticket"].view[0, 0]) == 0, (what, "launch", j, "the ticket is", int(o["ticket"].view[0, 0]), "not 0")
            assert moved == (j + 1 if c.p["ticket"] else 0), (what, "launch", j, "the counter moved by", moved)
    if after:
        after(o)
    _check_outside(c, t, o, what)
    key = (_family(c), fmt, _regime(c))
    if record:
        COUNT[key] = COUNT.get(key, 0) + 1
    for name in t["ref"]:
        got = o[name].view
        msg, r = SC.compare(c, t, name, got)
        if r is not None:
            print(f"[small exact] {key[0]} {fmt} {key[2]} {c.id} {name}: error / gate {r:.3f}")
            if record and r > WORST.get(key, (-1.0, None))[0]:
                WORST[key] = (r, c.id)
        if msg:
            idx = [int(v) for v in msg.split("first bad index [")[1].split("]")[0].split(",")]
            c0 = t.get("cols", {}).get(name, (0, 0))[0]
            raise AssertionError((what, msg, SC.where(c, name, (idx[0], idx[1] + c0))))


@pytest.mark.parametrize("c", SC.CASES, ids=lambda c: c.id)
def test_case(c):
    failures = []
    for dtype, fmt in SC.case_dtypes(c):
        try:
            _run(c, dtype, fmt)
        except AssertionError as e:                        # both formats are run and reported
            failures.append(e.args[0] if e.args else repr(e))
    assert not failures, failures


def test_the_checks_notice_what_they_are_for():
    """negative controls on the device: one expected value off by one unit of fp32, one sentinel overwritten behind the window,
    one in a pad column, a reference 2 u off under the R gate -- each must fail the case that passes untouched"""
    c = next(k for k in SC.CASES if k.kernel == "skinny" and k.probe == "E" and k.p["rows"] == 5)
    dtype, fmt = SC.DTYPES[0]
    _run(c, dtype, fmt, record=False)

    def off_by_one(t):
        t["ref"]["out"][4, 332] += 1.0

    def behind(o):
        b = o["out"]
        b.full[b.base + b.rows * b.ld] = 1.0

    def pad(o):
        b = o["out"]
        b.full[b.base + b.cols] = 1.0
    for kw, msg in ((dict(tamper=off_by_one), "not bit-equal"), (dict(after=behind), "outside the window"),
                    (dict(after=pad), "outside the window")):
        with pytest.raises(AssertionError, match=msg):
            _run(c, dtype, fmt, record=False, **kw)
    r = next(k for k in SC.CASES if k.kernel == "conv_direct" and k.probe == "R" and k.p["cin"] == 4 and k.p["cout"] == 320)

    def two_u(t):
        t["ref"]["out"] *= 1 + 2 * SC.unit_roundoff(dtype)
    with pytest.raises(AssertionError, match="error / gate"):
        _run(r, dtype, fmt, tamper=two_u, record=False)
    n = next(k for k in SC.CASES if k.kernel == "to_nhwc" and k.p["c0"] > 0 and k.p["src"] == "f32")

    def front_cols(o):                                     # a column in front of c0, inside the row stride
        o["dst"].view[3, 0] = 1.0
    with pytest.raises(AssertionError, match="pad columns"):
        _run(n, dtype, fmt, after=front_cols, record=False)


def _gn_conv_call(t, p, dt, out_ptr, cout=4):
    return L.lib().pp_gn_conv3x3_smallcout(_ptr(t["x"]), p["B"], p["H"], p["W"], p["cin"], p["groups"], 1e-5, t["gamma"].data_ptr(),
                                           t["beta"].data_ptr(), t["acc"].data_ptr(), _ptr(t["w"]), _ptr(t["bias"]), cout, out_ptr, dt,
                                           torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("p", SC.GN_CONV_CASES, ids=lambda p: f"{p['H']}x{p['W']}-cin{p['cin']}")
def test_fused_conv_out_is_the_two_launches_bit_for_bit(p):
    """pp_gn_conv3x3_smallcout == pp_groupnorm_apply_acc -> pp_conv3x3_smallcout to the bit on data whose sums are exact in any
    order (small_cases.GN_CONV_CASES; the conv_out cases above hold pp_conv3x3_smallcout itself to its gate), in a guarded window"""
    B, H, W, cin, groups = p["B"], p["H"], p["W"], p["cin"], p["groups"]
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    assert lib.pp_gn_conv3x3_smallcout_supported(cin, 4, groups) == 1 and SC.gn_conv_supported(cin, 4, groups)
    for dtype, fmt in SC.DTYPES:
        what = f"gn_conv {H}x{W} cin {cin} {fmt}"
        dt = L.dtype_code(dtype)
        t = {k: (v.to(DEV) if isinstance(v, (SC.Buf, torch.Tensor)) else v) for k, v in SC.build_gn_conv(p, dtype).items()}
        t["gamma"], t["beta"] = t["gamma"].float().contiguous(), t["beta"].float().contiguous()
        y = torch.empty(B * H * W * cin, dtype=dtype, device=DEV)
        two = SC.window(B * 4 * H, W, 0, torch.float32).to(DEV)
        L.check(lib.pp_groupnorm_apply_acc(_ptr(t["x"]), cin, None, 0, B, H * W, groups, 1e-5, t["gamma"].data_ptr(),
                                           t["beta"].data_ptr(), t["acc"].data_ptr(), 1, y.data_ptr(), dt, st), "apply_acc")
        L.check(lib.pp_conv3x3_smallcout(y.data_ptr(), B, H, W, cin, _ptr(t["w"]), _ptr(t["bias"]), 4, _ptr(two), dt, st), "conv_out")
        L.check(_gn_conv_call(t, p, dt, _ptr(t["out"])), "pp_gn_conv3x3_smallcout")
        torch.cuda.synchronize()
        # the precondition of bit equality: the stored activation is a multiple of 2^-12 in [0.5, 2)
        yd = y.double()
        assert bool((yd * 4096 == torch.round(yd * 4096)).all()) and 0.5 <= float(yd.min()) and float(yd.max()) < 2.0, (what, "activation")
        assert SC.outside_clean(t["out"]) and SC.outside_clean(two), (what, "bytes outside the window were written")
        ne = SC.bits(t["out"].view.contiguous()) != SC.bits(two.view.contiguous())
        if bool(ne.any()):
            i = ne.nonzero()[0].tolist()
            yy, xx = i[0] % H, i[1]
            raise AssertionError((what, "fused != two launches at", int(ne.sum()), "elements; first", i, float(t["out"].view[tuple(i)]),
                                  float(two.view[tuple(i)]), "patch", (yy // 8, xx // 8),
                                  "patch edge" if yy % 8 in (0, 7) or xx % 8 in (0, 7) else ""))
        # and both are the conv of that activation: fp64, exact
        ref = torch.nn.functional.conv2d(yd.view(B, H, W, cin).permute(0, 3, 1, 2), t["w64"].view(4, 3, 3, cin).permute(0, 3, 1, 2),
                                         t["bias"].view[0].double(), padding=1).reshape(B * 4 * H, W)
        assert bool((two.view.double() == ref).all()), (what, "pp_conv3x3_smallcout on the exact activation")
        COUNT[("gn_conv", fmt, "E")] = COUNT.get(("gn_conv", fmt, "E"), 0) + 1


@pytest.mark.parametrize("p", SC.GN_CONV_REFUSED, ids=lambda p: f"cin{p['cin']}-g{p['groups']}-cout{p['cout']}")
def test_fused_conv_out_refuses_what_supported_refuses(p):
    assert L.lib().pp_gn_conv3x3_smallcout_supported(p["cin"], p["cout"], p["groups"]) == 0 and not SC.gn_conv_supported(p["cin"], p["cout"], p["groups"])
    dtype = SC.DTYPES[0][0]
    q = dict(p, cin=-(-p["cin"] // 32) * 32, groups=32)             # (buffers of a shape that can be built)
    t = {k: (v.to(DEV) if isinstance(v, (SC.Buf, torch.Tensor)) else v) for k, v in SC.build_gn_conv(q, dtype).items()}
    t["gamma"], t["beta"] = t["gamma"].float().contiguous(), t["beta"].float().contiguous()
    rc = _gn_conv_call(t, p, L.dtype_code(dtype), _ptr(t["out"]), cout=p["cout"])
    torch.cuda.synchronize()
    assert rc == SC.PP_ERR_UNSUPPORTED, L.PP_ERR.get(rc, rc)
    assert bool((SC.bits(t["out"].full) == SC.SENT[4]).all()), "a refused request wrote"


def test_matrix_size():
    print(f"[small exact] {len(SC.CASES)} cases, {sum(len(SC.case_dtypes(c)) for c in SC.CASES)} (case, format) runs")
    assert len(SC.CASES) >= 300
