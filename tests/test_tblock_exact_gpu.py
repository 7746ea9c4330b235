"""-m gpu: pp_ff_fused (4-wave and 8-wave form), pp_tfront, pp_xattn_block (plain, pre_w, src_wrap_rows, the wide kernel) and
pp_xattn_fold through the C ABI on the matrix of tests/tblock_cases.py.  Derivations: that module's docstring and
tests/norm_cases.py; proof that every probe can fail: tests/test_tblock_probes.py.

  E cases    every output window EQUALS the fp64 reference cast once to its format, bit for bit (signed zeros compare equal);
             the GroupNorm accumulators equal the integer moments of the stored values, the row moments their fp32 sums;
  R cases    |out - ref| <= the derived gate (nothing fitted); accumulators and row moments against the moments of the STORED
             values under gate_epilogue_acc / gate_row_stats_xattn;
  pp_tfront  hs as above; Q, K and V^T under gate_tfront_qkv computed from the hs the kernel stored; a second call that differs
             only in q_scale leaves hs, K and V^T bit-identical;
  pre_w      h = round16(x pre_w^T + pre_b + res) is read back by a second launch with H^T = 0 and no bias, held to bit equality
             (E) or its GEMM gate (R), and the output of an R case is gated from that h;
  pp_ff_fused both forms run every case; a case with accumulators is launched twice: equal bits;
  every case outputs are windows of sentinel-filled buffers (guard rows in front and behind, a row stride larger than the row);
             every byte outside a window is unchanged after the launch; strided inputs carry NaN in their pad columns and
             guard rows;
  refusals   carry the stated code and happen before any launch: nothing at all is written.

After a whole run of the file profiles/tblock_exact_achieved.txt is rewritten: per (kernel form, format, probe) the worst
achieved / gate and the number of bit-equal runs; no threshold is pinned on it.
"""
import ctypes as C
import os
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import tblock_cases as TC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import ops  # noqa: E402

DEV = "cuda"
WORST, COUNT, T0 = {}, {}, [None]
ACHIEVED_HEADER = (
    "# tests/test_tblock_exact_gpu.py on one MI355X: per (kernel form, format, probe) the largest achieved error / gate of the gated\n"
    "# windows (gates: tests/norm_cases.py and tests/tblock_cases.py, derived from rounding counts, worst case, not fitted: the\n"
    "# ratio shows the slack, no threshold is pinned on it) and the number of runs; E runs held bit equality on out / hs / gt / ht /\n"
    "# gbias, their ratio is that of the gated side windows (Q, K, V^T of pp_tfront; gcs of pp_xattn_fold).  Assumed, not derived:\n"
    "# v_rcp_f32 and v_exp_f32 within 1 ulp, rsqrtf within 4 * 2^-24 relative, gelu_fast_f within 2^-20 |g| of gelu.  gcs of\n"
    "# pp_xattn_fold sits far below its gate: the gate is the worst case of a 320- to 1280-term fp32 sum, the probe's rows hold few\n"
    "# distinct multiples of one quantum and sum (almost) exactly.  The wall time is rounded to 30 s, at least 30 s, so that this\n"
    "# tracked file is the same after every run.\n")


def _n_runs():
    return sum(len(TC.DTYPES) * len(TC.forms(c)) for c in TC.CASES)


@pytest.fixture(scope="module", autouse=True)
def _achieved():
    T0[0] = time.time()
    yield
    if sum(COUNT.values()) != _n_runs():
        return
    try:
        with open(os.path.join(ROOT, "profiles", "tblock_exact_achieved.txt"), "w") as f:
            f.write(ACHIEVED_HEADER)
            for key in sorted(COUNT):
                line = f"[tblock exact] {key[0]} {key[1]} {key[2]}: {COUNT[key]} runs"
                line += f", worst error / gate {WORST[key][0]:.3f} at {WORST[key][1]}" if key in WORST else ", bit-equal"
                f.write(line + "\n")
            wall = max(30, 30 * round((time.time() - T0[0]) / 30))
            f.write(f"# {len(TC.CASES)} cases, {sum(COUNT.values())} (case, form, format) runs, {len(TC.REFUSALS)} refusals; wall time of "
                    f"the file about {wall} s\n")
    except OSError:
        pass


def _ptr(b, off: int = 0):
    if b is None:
        return None
    if isinstance(b, TC.Buf):
        return b.full.data_ptr() + b.base * b.full.element_size() + off
    return b.data_ptr() + off


def _dev(x):
    if isinstance(x, (TC.Buf, torch.Tensor)):
        return x.to(DEV)
    return x


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _launch(c, p, i, o, dt, form, over=None, q_scale=None):
    """one call of the library: case parameters p, inputs i and output windows o on the device; `over`: the overrides of a
    refusal.  -> the return code"""
    lib, st, v = L.lib(), _stream(), (over or {})
    k = c.kernel
    if k == "ff":
        M = v.get("M_arg", p["M"])
        w8 = form == "w8"
        a = L.gemm_args(dt, M, 320, 1280, None, _ptr(i["w2"] if w8 else i["w2kp"]), _ptr(o["out"], v.get("out_off", 0)),
                        x2=_ptr(i["hs"]), K2=320, ldx2=v.get("ldx", i["hs"].ld), ldo=v.get("ldo", o["out"].ld),
                        ldres1=v.get("ldres1", i["res1"].ld if i["res1"] is not None else 0),
                        ldres2=v.get("ldres2", i["res2"].ld if i["res2"] is not None else 0),
                        rows_per_batch=v.get("rpb", p["rpb"]), scale=p["scale"])
        a.bias, a.res1, a.res2 = _ptr(i["bias2"]), _ptr(i["res1"], v.get("res1_off", 0)), _ptr(i["res2"])
        a.res1_wrap_rows = v.get("wrap", p["wrap"])
        for n, (cg, c0, G) in enumerate(p["gn"]):
            a.gn_acc[n], a.gn_cg[n], a.gn_c0[n], a.gn_groups[n] = _ptr(o[f"acc{n}"]), v.get("gn_cg", cg), c0, G
        g2 = v.get("g2")
        some = _ptr(o["out"])                              # (a valid device address for a field that must be refused unread)
        if g2 in ("rowvec", "row_stats_out", "ln_stats", "gn_next_out", "out_vt", "gn_in_acc"):
            setattr(a, g2, some)
        elif g2 == "act":
            a.act = L.PP_ACT_GEGLU
        elif g2 == "out_f32":
            a.out_f32 = 1
        elif g2 == "out_dup_rows":
            a.out_dup_rows = M
        elif g2 == "splitk":
            a.splitk = 2
        elif g2 == "N":
            a.N = 160
        elif g2 == "K":
            a.K = 1280
        cs1 = v["cs1"] if "cs1" in v else _ptr(i["cs1"])
        tiles = i["st"].shape[1] if i["st"] is not None else 0
        return lib.pp_ff_fused(C.byref(a), _ptr(i["w1"]), _ptr(i["b1"]), cs1, _ptr(i["st"]), tiles, 1e-5, 0 if w8 else 1, st)
    if k == "tfront":
        cc = v.get("c", 320)
        return lib.pp_tfront(_ptr(i["x"]), v.get("ldx", i["x"].ld), _ptr(i["acc"]), _ptr(i["gamma"]), _ptr(i["beta"]), 1e-6,
                             v.get("groups", p["groups"]), _ptr(i["w1"]), _ptr(i["b1"]), _ptr(i["w2p"]), _ptr(i["cs"]), _ptr(i["tb"]),
                             1e-5, _ptr(o["hs"], v.get("hs_off", 0)), v.get("ldhs", o["hs"].ld), _ptr(o["qk"], v.get("qk_off", 0)),
                             v.get("ldqk", o["qk"].ld), _ptr(o["vt"]), v.get("ldvt", o["vt"].ld), v.get("M_arg", p["M"]), cc,
                             v.get("rpb", p["rpb"]), float(v.get("q_scale", p["q_scale"] if q_scale is None else q_scale)), dt, st)
    if k == "xattn":
        cc = v.get("c", p["C"])
        tiles = v.get("ln_tiles", i["st"].shape[1] if i["st"] is not None else (p["ln"] if p["pre"] else 0))
        pre_w = v["pre_w"] if "pre_w" in v else _ptr(i["pre_w"])
        return lib.pp_xattn_block(_ptr(i["x"]), v.get("ldx", i["x"].ld), _ptr(i["res"], v.get("res_off", 0)),
                                  v.get("ldres", i["res"].ld if i["res"] is not None else 0), _ptr(i["st"]), tiles, 1e-5,
                                  _ptr(i["gt"]), _ptr(i["gcs"]), _ptr(i["gb"]), _ptr(i["ht"]), _ptr(i["bo"]),
                                  _ptr(o["out"], v.get("out_off", 0)), v.get("ldo", o["out"].ld), _ptr(o.get("stats")),
                                  v.get("M_arg", p["M"]), cc, v.get("rpb", p["rpb"]), v.get("wrap", p["wrap"]), pre_w, _ptr(i["pre_b"]),
                                  dt, st)
    assert k == "fold"
    return lib.pp_xattn_fold(_ptr(i["k"]), v.get("ldk", i["k"].ld), _ptr(i["vt"]), v.get("ldvt", i["ldvt"]), v.get("batch", p["B"]),
                             v.get("nctx", p["nctx"]), v.get("heads", 8), p["C"], _ptr(i["wq"]), _ptr(i["qcs"]), _ptr(i["qb"]),
                             _ptr(i["wo"]), float(i["scale"]), _ptr(o["gt"]), _ptr(o["gcs"]), _ptr(o["gb"]), _ptr(o["ht"]),
                             v.get("kperm", p["kperm"]), dt, st)


def _fresh(t):
    return {k: _dev(v) for k, v in t["inp"].items()}, {k: v.to(DEV) for k, v in t["out"].items()}


def _collect(o):
    return {k: b.view.cpu().clone() for k, b in o.items()}


def _guards(o, what):
    for name, b in o.items():
        assert TC.outside_clean(b), (what, name, "bytes outside the window were written")


def _family(c, form):
    if c.kernel == "ff":
        return "ff_fused-" + ("8wave" if form == "w8" else "4wave")
    if c.kernel == "xattn":
        return "xattn_wide" + str(c.p["C"]) if c.p["C"] != 320 else ("xattn_block-pre" if c.p["pre"] else "xattn_block")
    return {"tfront": "tfront", "fold": "xattn_fold"}[c.kernel]


def _run(c, dtype, fmt, form, record=True, tamper=None):
    """tamper(got, o): the hook of the negative controls: changes a finished result before it is judged"""
    what = f"{c.id} {fmt} {form}".strip()
    t = TC.build(c, dtype)
    dt = L.dtype_code(dtype)
    i, o = _fresh(t)
    rc = _launch(c, c.p, i, o, dt, form)
    torch.cuda.synchronize()
    assert rc == 0, (what, L.PP_ERR.get(rc, rc), L.lib().pp_last_error().decode())
    got = _collect(o)
    if c.kernel == "xattn" and c.p["pre"]:                 # h itself: the same launch with H^T = 0 and no bias stores round16(0 + h)
        i2, o2 = _fresh(t)
        i2["ht"].zero_()
        i2["bo"] = None
        assert _launch(c, c.p, i2, o2, dt, form) == 0
        torch.cuda.synchronize()
        got["h"] = o2["out"].view.cpu().clone()
        _guards(o2, what)
    if tamper:
        tamper(got, o)
    bad, worst = TC.judge(c, t, dtype, got)
    key = (_family(c, form), fmt, c.probe)
    if worst is not None:
        print(f"[tblock exact] {key[0]} {fmt} {c.probe} {c.id}: error / gate {worst:.3f}")
    if record:
        COUNT[key] = COUNT.get(key, 0) + 1
        if worst is not None and worst > WORST.get(key, (-1.0, None))[0]:
            WORST[key] = (worst, c.id)
    assert not bad, (what, bad)
    _guards(o, what)
    if tamper:
        return
    if c.kernel == "ff" and c.p["gn"]:                     # a repeated call gives equal bits
        i2, o2 = _fresh(t)
        assert _launch(c, c.p, i2, o2, dt, form) == 0
        torch.cuda.synchronize()
        for name, v in _collect(o2).items():
            assert torch.equal(TC.bits(v), TC.bits(got[name])), (what, name, "a repeated call differs")
    if c.kernel == "tfront" and c.p["q_scale"] != 1.0:     # q_scale touches the Q third and nothing else
        i2, o2 = _fresh(t)
        assert _launch(c, c.p, i2, o2, dt, form, q_scale=1.0) == 0
        torch.cuda.synchronize()
        g2 = _collect(o2)
        assert torch.equal(TC.bits(g2["hs"]), TC.bits(got["hs"])) and torch.equal(TC.bits(g2["vt"]), TC.bits(got["vt"])), (what, "hs / V^T")
        assert torch.equal(TC.bits(g2["qk"][:, 320:]), TC.bits(got["qk"][:, 320:])), (what, "K changed with q_scale")
        w = TC.tfront_qkv_windows(c, t, g2["hs"], dtype, q_scale=1.0)["qk"]
        r = TC.NC.worst_ratio(g2["qk"], w[0], w[1])
        assert r <= 1.0, (what, "Q at q_scale = 1: error / gate", r)
        _guards(o2, what)


@pytest.mark.parametrize("c", TC.CASES, ids=lambda c: c.id)
def test_case(c):
    failures = []
    for dtype, fmt in TC.DTYPES:
        for form in TC.forms(c):
            try:
                _run(c, dtype, fmt, form)
            except AssertionError as e:                    # every format and form is run and reported
                failures.append(e.args[0] if e.args else repr(e))
    assert not failures, failures


@pytest.mark.parametrize("c", TC.REFUSALS, ids=lambda c: c.id)
def test_refusal(c):
    """by return code only: refused before any launch, nothing is written"""
    base = TC.refusal_base(c)
    dtype, fmt = TC.DTYPES[0]
    t = TC.build(base, dtype)
    i, o = _fresh(t)
    before = {k: TC.bits(b.full).clone() for k, b in o.items()}
    over = {k: v for k, v in c.p["over"].items() if k != "probe"}
    rc = _launch(base, base.p, i, o, L.dtype_code(dtype), TC.forms(base)[0], over=over)
    torch.cuda.synchronize()
    assert rc == c.p["expect"], (c.id, "returned", L.PP_ERR.get(rc, rc), "expected", L.PP_ERR[c.p["expect"]])
    for k, b in o.items():
        assert torch.equal(TC.bits(b.full), before[k]), (c.id, k, "a refused request wrote")


def test_the_checks_notice_what_they_are_for():
    """negative controls: a finished result is changed on the host -- one element by one 16-bit ulp, one guard word, one
    accumulator by 1, two rows swapped, a gated value by twice its gate -- and each check must fire"""
    dtype, fmt = TC.DTYPES[0]
    c = TC.BY_ID["ff-E-gn-two"]
    _run(c, dtype, fmt, "w4", record=False, tamper=lambda got, o: None)

    def ulp(got, o):
        v = TC.bits(got["out"])
        v[200, 171] += 1

    def guard(got, o):
        b = o["out"]
        b.full[b.base + b.rows * b.ld + 3] = 1.0

    def pad(got, o):
        b = o["out"]
        b.full[b.base + 5 * b.ld + b.cols] = 1.0

    def acc(got, o):
        got["acc1"][2, 7] += 1

    def swap(got, o):
        got["out"][[5, 133]] = got["out"][[133, 5]]
    for fn, msg in ((ulp, "out: not bit-equal at 1 "), (guard, "outside the window"), (pad, "outside the window"), (acc, "acc1: not bit-equal"),
                    (swap, "out: not bit-equal")):
        with pytest.raises(AssertionError, match=msg):
            _run(c, dtype, fmt, "w4", record=False, tamper=fn)
    r = TC.BY_ID["xattn-R-plain"]

    def two_gates(got, o):
        t = TC.build(r, dtype)
        ref, gate = t["ref"]["out"]
        got["out"][7, 11] = (ref[7, 11] + 2.0 * gate[7, 11] + 2.0 ** -7 * ref[7, 11].abs()).to(dtype)
    with pytest.raises(AssertionError, match="error / gate"):
        _run(r, dtype, fmt, "", record=False, tamper=two_gates)
    tf = TC.BY_ID["tfront-E-rpb256-b3"]

    def vt_rows(got, o):                                   # two channels of V^T swapped: only the gate on V^T can see it
        got["vt"][[3, 4]] = got["vt"][[4, 3]]
    with pytest.raises(AssertionError, match="vt: error / gate"):
        _run(tf, dtype, fmt, "", record=False, tamper=vt_rows)


def test_the_wrappers_take_strided_windows_and_refuse_buffers_that_do_not_fit():
    """powerpaint_amd.ops: caller-owned outputs are windows of larger buffers and give the bits of the default call; a view that
    does not fit raises PPError before any launch"""
    dtype = torch.bfloat16
    # ---- pp_ff_fused
    c = TC.BY_ID["ff-E-open-chunk"]
    t = TC.build(c, dtype)
    i = {k: _dev(v) for k, v in t["inp"].items()}
    kw = dict(bias2=i["bias2"], res1=i["res1"].view, w2_kperm=True)
    ref = ops.ff_fused(i["hs"].view, i["w1"], i["b1"], i["w2kp"], **kw)
    big = torch.full((130, 336), 7.0, dtype=dtype, device=DEV)
    out = ops.ff_fused(i["hs"].view, i["w1"], i["b1"], i["w2kp"], out=big[1:129, 8:328], **kw)
    assert out.data_ptr() == big[1:129, 8:328].data_ptr() and torch.equal(out, ref) and torch.equal(ref.cpu().double(), t["ref"]["out"])
    assert bool((big[0] == 7).all()) and bool((big[129] == 7).all()) and bool((big[:, :8] == 7).all()) and bool((big[:, 328:] == 7).all())
    for bad in (big[:127, :320], big[:128, :328], big.t()[:128, :128], big[:128, :320].float(), big[:128, :320].cpu(), big[:128, ::2][:, :160]):
        with pytest.raises(L.PPError):
            ops.ff_fused(i["hs"].view, i["w1"], i["b1"], i["w2kp"], out=bad, **kw)
    with pytest.raises(L.PPError):
        ops.ff_fused(i["hs"].view.t()[:128, :128], i["w1"], i["b1"], i["w2kp"])
    with pytest.raises(L.PPError):
        ops.ff_fused(i["hs"].view, i["w1"], i["b1"], i["w2kp"], res1=i["res1"].view[:64])
    # ---- pp_tfront
    c = TC.BY_ID["tfront-E-groups16"]
    t = TC.build(c, dtype)
    i = {k: _dev(v) for k, v in t["inp"].items()}
    args = (i["x"].view, i["acc"], i["gamma"], i["beta"], i["w1"], i["b1"], i["w2p"], i["cs"], i["tb"], 128)
    hs0, qk0, vt0 = ops.tfront(*args, groups=16)
    hsb, qkb, vtb = (torch.full(s, 7.0, dtype=dtype, device=DEV) for s in ((258, 328), (258, 656), (2, 320, 136)))
    hs1, qk1, vt1 = ops.tfront(*args, groups=16, hs=hsb[1:257, :320], qk=qkb[1:257, 8:648], vt=vtb[:, :, :128])
    assert torch.equal(hs1, hs0) and torch.equal(qk1, qk0) and torch.equal(vt1, vt0) and torch.equal(hs0.cpu().double(), t["ref"]["hs"])
    assert bool((vtb[:, :, 128:] == 7).all()) and bool((hsb[:, 320:] == 7).all()) and bool((qkb[:, :8] == 7).all())
    for kwb in (dict(hs=hsb[:255, :320]), dict(qk=qkb[:256, :320]), dict(vt=vtb[:, :, :120]), dict(vt=vtb[:1, :, :128]),
                dict(vt=vtb[:, :319, :128]), dict(hs=hsb[:256, :320].half())):
        with pytest.raises(L.PPError):
            ops.tfront(*args, groups=16, **kwb)
    with pytest.raises(L.PPError):
        ops.tfront(i["x"].view, i["acc"][:, :8], *args[2:], groups=16)
    # ---- pp_xattn_block and pp_xattn_fold
    c = TC.BY_ID["xattn-E-nctx7"]
    t = TC.build(c, dtype)
    i = {k: _dev(v) for k, v in t["inp"].items()}
    folded = (i["gt"], i["gcs"], i["gb"], i["ht"])
    kw = dict(bias_o=i["bo"], res=i["res"].view, rows_per_batch=128)
    ref, st0 = ops.xattn_block(i["x"].view, folded, row_stats=True, **kw)
    big = torch.full((258, 336), 7.0, dtype=dtype, device=DEV)
    stb = torch.zeros(256, 2, 2, dtype=torch.float32, device=DEV)
    out, st1 = ops.xattn_block(i["x"].view, folded, row_stats=stb, out=big[1:257, 8:328], **kw)
    assert torch.equal(out, ref) and st1.data_ptr() == stb.data_ptr() and torch.equal(st1, st0)
    assert torch.equal(ref.cpu().double(), t["ref"]["out"]) and bool((big[:, :8] == 7).all()) and bool((big[257] == 7).all())
    for kwb in (dict(out=big[:255, :320]), dict(out=big[:256, :320].half()), dict(row_stats=stb[:255]), dict(row_stats=stb.double()),
                dict(row_stats=torch.zeros(256, 4, 2, device=DEV)[:, ::2])):
        with pytest.raises(L.PPError):
            ops.xattn_block(i["x"].view, folded, **dict(kw, **kwb))
    with pytest.raises(L.PPError):
        ops.xattn_block(i["x"].view, (i["gt"][:1], i["gcs"], i["gb"], i["ht"]), **kw)
    c = TC.BY_ID["fold-E-nctx7"]
    t = TC.build(c, dtype)
    i = {k: _dev(v) for k, v in t["inp"].items()}
    B, nctx, Cc = c.p["B"], c.p["nctx"], c.p["C"]
    vt3 = i["vt"].view.view(B, Cc, i["ldvt"])
    fargs = (i["k"].view, vt3[:, :, :nctx], B, nctx, 8, i["wq"], i["wo"])
    fkw = dict(q_colsum=i["qcs"].to(DEV), q_bias=i["qb"].to(DEV), kperm=c.p["kperm"])
    f0 = ops.xattn_fold(*fargs, **fkw)
    mine = (torch.empty(B, 640, Cc, dtype=dtype, device=DEV), torch.empty(B, 640, device=DEV), torch.empty(B, 640, device=DEV),
            torch.empty(B, Cc, 640, dtype=dtype, device=DEV))
    f1 = ops.xattn_fold(*fargs, gt=mine[0], gcs=mine[1], gbias=mine[2], ht=mine[3], **fkw)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(f1, mine)) and all(torch.equal(a, b) for a, b in zip(f0, f1))
    assert torch.equal(f0[3].reshape(B * Cc, 640).cpu().double(), t["ref"]["ht"])
    for kwb in (dict(gt=mine[0][:, :639]), dict(ht=mine[3].transpose(1, 2)), dict(gcs=mine[1].double()), dict(gbias=mine[2][:1])):
        with pytest.raises(L.PPError):
            ops.xattn_fold(*fargs, **dict(fkw, **kwb))
    with pytest.raises(L.PPError):
        ops.xattn_fold(i["k"].view[:, :312], *fargs[1:], **fkw)


def test_matrix_size():
    print(f"[tblock exact] {len(TC.CASES)} cases, {_n_runs()} (case, form, format) runs, {len(TC.REFUSALS)} refusals, {len(TC.DEFECTS)} defects")
    assert len(TC.CASES) >= 120 and _n_runs() >= 320 and len(TC.REFUSALS) >= 65
