"""CPU: DeepCache -- the float64 restatement (tests/deepcache_cases.py) against the plain oracle, the index table, the public
helper (powerpaint_amd/deepcache.py), the two launch plans of a patched runtime and the program the fused loop picks per
evaluation (dry builds: no launch runs in this file)."""
import functools
import os
import sys
from types import SimpleNamespace

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import deepcache_cases as DC  # noqa: E402
from powerpaint_amd import _lib as L  # noqa: E402
from powerpaint_amd import pipelines as PP  # noqa: E402
from powerpaint_amd import schedulers as PS  # noqa: E402
from powerpaint_amd import tome  # noqa: E402
from powerpaint_amd.deepcache import DeepCacheSDHelper  # noqa: E402
from powerpaint_amd.engine import DeepCache, Plan  # noqa: E402
from powerpaint_amd.pipelines._loop import DenoiseLoop  # noqa: E402
from test_hypertile import _launches  # noqa: E402
from test_ip_adapter import TINY, _describe, _hip_unet, _net, _pipe  # noqa: E402


def gen(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator("cpu").manual_seed(seed)) * scale).double()


def leaves_the_gate(out, ref):
    """test_models_gpu.close's gate (cosine >= 0.999 and max-abs <= 3e-2 max(1, max|ref|)), as a predicate: does `out` FAIL it?"""
    cos = torch.nn.functional.cosine_similarity(out.flatten(), ref.flatten(), dim=0).item()
    err = (out - ref).abs().max().item()
    return cos < 0.999 or err > 3e-2 * max(1.0, ref.abs().max().item()), cos, err


# ------------------------------------------------------------------------------------------------------------ restatement
@functools.lru_cache(maxsize=None)
def _o(kind, cin=4, seed=0):
    return DC.tiny_oracle(kind, seed=seed, in_channels=cin).double()


def _inputs(ev, cin=4, B=1, h=8, w=8):
    return gen(B, cin, h, w, seed=10 + ev), [901, 500, 99, 640, 333][ev], gen(B, 77, 768, seed=20 + ev)


@pytest.mark.parametrize("bid", [0, 1, 2])
def test_interval_one_and_evaluation_zero_are_the_plain_oracle(bid):
    o = _o("unet")
    every = DC.DeepCacheUNet(o, 1, bid)
    third = DC.DeepCacheUNet(o, 3, bid)
    for ev in range(3):
        x, t, e = _inputs(ev)
        with torch.no_grad():
            plain = o(x, t, e)[0]
        assert torch.equal(every(x, t, e)[0], plain)                       # cache_interval = 1: every output, exactly
        got = third(x, t, e)[0]
        if ev == 0:
            assert torch.equal(got, plain)                                 # evaluation 0 is full
    assert every.trace == ["F", "F", "F"] and third.trace == ["F", "S", "S"]


@pytest.mark.parametrize("bid", [0, 1, 2])
def test_shallow_on_the_inputs_of_the_full_one_reproduces_it(bid):
    """The same operations on the same numbers: a shallow evaluation fed the input and timestep of the full one in front of it
    gives that evaluation's output bit for bit (twice: the cache survives a shallow evaluation)."""
    o = _o("unet")
    w = DC.DeepCacheUNet(o, 3, bid)
    x, t, e = _inputs(0)
    full = w(x, t, e)[0]
    assert torch.equal(w(x, t, e)[0], full) and torch.equal(w(x, t, e)[0], full) and w.trace == ["F", "S", "S"]


@pytest.mark.parametrize("bid", [0, 1, 2])
def test_shallow_on_fresh_inputs_leaves_the_gate(bid):
    """The precondition of the must-fail assertions of tests/test_deepcache_gpu.py, in float64: on fresh inputs and timesteps a
    shallow evaluation is NOT the plain network at the small networks' gate, at every cache_branch_id (make_tiny's own weights:
    no sharpening is needed; measured cosine 0.80 .. 0.91)."""
    o = DC.tiny_oracle("unet", in_channels=4).double()
    w = DC.DeepCacheUNet(o, 3, bid)
    for ev in range(3):
        x, t, e = gen(2, 4, 16, 16, seed=10 + ev), [900, 500, 100][ev], gen(2, 77, 768, seed=20 + ev)
        with torch.no_grad():
            plain = o(x, t, e)[0]
        fails, cos, err = leaves_the_gate(w(x, t, e)[0], plain)
        print(f"[deepcache] id {bid} evaluation {ev} ({w.trace[-1]}): cosine {cos:.6f}, max-abs {err:.4f} against the plain oracle")
        assert fails == (ev > 0)


def test_side_networks_at_interval_one_are_the_plain_oracles():
    ob, oc, ou4, ou9 = _o("brushnet"), _o("controlnet"), _o("unet", 4, 1), _o("unet", 9, 1)
    x, t, e = _inputs(0)
    cond, img, x9 = gen(1, 5, 8, 8, seed=4), gen(1, 3, 64, 64, seed=5).abs(), gen(1, 9, 8, 8, seed=6)
    with torch.no_grad():
        dn, md, up = ob(x, t, e, cond, conditioning_scale=0.8, guess_mode=True)
        ref = ou4(x, t, e, down_block_add_samples=list(dn), mid_block_add_sample=md, up_block_add_samples=list(up))[0]
        cdn, cmd = oc(x, t, e, img, conditioning_scale=0.5, guess_mode=True)
        cref = ou9(x9, t, e, down_block_additional_residuals=cdn, mid_block_additional_residual=cmd)[0]
    wb, wu = DC.DeepCacheBrushNet(ob, 1, 0), DC.DeepCacheUNet(ou4, 1, 0)
    d2, m2, u2 = wb(x, t, e, cond, conditioning_scale=0.8, guess_mode=True)
    assert all(torch.equal(a, b) for a, b in zip(d2 + [m2] + u2, list(dn) + [md] + list(up)))
    assert torch.equal(wu(x, t, e, down_block_add_samples=list(d2), mid_block_add_sample=m2, up_block_add_samples=list(u2))[0], ref)
    wc, wu9 = DC.DeepCacheControlNet(oc, 1, 0), DC.DeepCacheUNet(ou9, 1, 0)
    c2, cm2 = wc(x, t, e, img, conditioning_scale=0.5, guess_mode=True)
    assert all(torch.equal(a, b) for a, b in zip(c2 + [cm2], list(cdn) + [cmd]))
    assert torch.equal(wu9(x9, t, e, down_block_additional_residuals=c2, mid_block_additional_residual=cm2)[0], cref)
    # a shallow evaluation produces the live positions only, with the full network's guess-mode scales there
    wb3, wc3 = DC.DeepCacheBrushNet(ob, 3, 0), DC.DeepCacheControlNet(oc, 3, 0)
    wb3(x, t, e, cond, guess_mode=True), wc3(x, t, e, img, guess_mode=True)
    d3, m3, u3 = wb3(x, t, e, cond, conditioning_scale=0.8, guess_mode=True)
    assert wb3.live == [0, 1, 4 + 1 + 3, 4 + 1 + 4] and m3 is DC.DEAD and d3[2] is DC.DEAD and u3[0] is DC.DEAD
    assert torch.equal(d3[1], dn[1]) and torch.equal(u3[4], up[4])          # (same inputs: the same numbers)
    c3, cm3 = wc3(x, t, e, img, conditioning_scale=0.5, guess_mode=True)
    assert wc3.live == [0, 1] and cm3 is DC.DEAD and torch.equal(c3[1], cdn[1])


# ------------------------------------------------------------------------------------------------------------ index table
@pytest.mark.parametrize("cfg,table", [(TINY, DC.INDEX_TINY), ({}, DC.INDEX_SD15)], ids=["tiny", "sd15"])
def test_index_table(cfg, table):
    from powerpaint_amd.runtime import NetRuntime
    net = _net(**cfg)
    for bid, (n, down, up, cache) in table.items():
        net.deepcache = DeepCache(bid)
        rt = NetRuntime(net, "cpu")
        rt.ensure(1, 16, 16, 77, 4, ("plain",))
        assert net.skip_count() == n
        w = rt.shallow_plan.walk
        assert (w["down"], w["up"], w["cache"]) == (down, up, cache), bid
        assert rt.step_plan.walk["cache"] == cache                          # the full form records the same place
        assert len(rt.step_plan.walk["down"]) == n and len(rt.step_plan.walk["up"]) == n + len(net.boc) - 1
    if cfg:                                                                 # ... and the restatement walks the same modules
        o = _o("unet")
        for bid, (n, down, up, cache) in table.items():
            wr = DC.DeepCacheUNet(o, 2, bid)
            x, t, e = _inputs(0)
            wr(x, t, e), wr(x, t, e)
            assert wr.n == n and (["conv_in"] + wr.down_names, wr.up_names, wr.cache_name) == (down, up, cache), bid


# ------------------------------------------------------------------------------------------------------------ helper
def test_helper_refusals_by_name():
    u = _hip_unet(**TINY)
    h = DeepCacheSDHelper(u)
    for bad in (0, -1, 2.0, "3", True, None):
        with pytest.raises(ValueError, match="cache_interval must be an integer >= 1"):
            h.set_params(cache_interval=bad)
    for bad in (-1, 3, 11, 1.0):
        with pytest.raises(ValueError, match="cache_branch_id"):
            h.set_params(cache_branch_id=bad)
    with pytest.raises(ValueError, match=r"cache_branch_id must lie in 0\.\.2 for this unet \(4 skip tensors\)"):
        h.set_params(cache_branch_id=3)
    with pytest.raises(NotImplementedError, match="skip_mode"):
        h.set_params(skip_mode="nonuniform")
    assert u.net.deepcache is None and not h.enabled
    with pytest.raises(TypeError):
        DeepCacheSDHelper(object()).enable()
    with pytest.raises(ValueError, match="no pipeline"):
        DeepCacheSDHelper().enable()
    full = _hip_unet()                                                      # SD-1.5: ids 0..10
    DeepCacheSDHelper(full).set_params(cache_branch_id=10)
    with pytest.raises(ValueError, match=r"0\.\.10"):
        DeepCacheSDHelper(full).set_params(cache_branch_id=11)


def test_set_params_before_enable_and_disable_restores():
    u = _hip_unet(**TINY)
    u.rt.ensure(2, 16, 16, 77, 4, ("plain",))
    want = (_describe(u.rt.step_plan), u.rt.key)
    h = DeepCacheSDHelper(u)
    assert h.set_params(cache_interval=5, cache_branch_id=1) is h and u.net.deepcache is None      # nothing patched yet
    assert h.enable() is h and tuple(u.net.deepcache) == (1, 5)
    u.rt.ensure(2, 16, 16, 77, 4, ("plain",))
    assert ("deepcache", 1) in u.rt.key and u.rt.key != want[1] and u.rt.shallow_plan is not None
    u.rt.dc_eval = 4
    h.set_params(cache_interval=2, cache_branch_id=1)                       # enabled: takes effect at once, counter back to 0
    assert tuple(u.net.deepcache) == (1, 2) and u.rt.dc_eval == 0
    assert h.disable() is h and u.net.deepcache is None
    u.rt.ensure(2, 16, 16, 77, 4, ("plain",))
    assert (_describe(u.rt.step_plan), u.rt.key) == want and u.rt.shallow_plan is None
    p = _pipe(u)                                                            # a pipeline patches the networks it holds
    DeepCacheSDHelper(p).enable()
    assert tuple(u.net.deepcache) == (0, 3)
    DeepCacheSDHelper(p).disable()
    assert u.net.deepcache is None


def test_token_merging_and_pag_are_refused_naming_both():
    u = _hip_unet(**TINY)
    tome.apply_patch(u)
    with pytest.raises(L.PPError, match=r"DeepCache.*token merging \(ToMe\)"):
        DeepCacheSDHelper(u).enable()
    assert u.net.deepcache is None
    tome.remove_patch(u)
    DeepCacheSDHelper(u).enable()
    tome.apply_patch(u)                                                     # the other order: refused when the plan is built
    with pytest.raises(L.PPError, match=r"DeepCache.*token merging \(ToMe\)"):
        u.rt.ensure(2, 16, 64, 77, 4, ("plain",))
    tome.remove_patch(u)
    from powerpaint_amd.engine import PAG
    with pytest.raises(L.PPError, match=r"DeepCache.*perturbed-attention guidance \(PAG, pag_scale > 0\)"):
        u.rt.ensure(3, 16, 16, 77, 4, ("plain",), pag=PAG(("mid_block.attentions.0",), 1))
    loop = _loop(deep=True)                                                 # ... and by the loop, before anything is built
    loop.unet.net.deepcache = DeepCache(0, 2)
    with pytest.raises(L.PPError, match=r"DeepCache.*perturbed-attention guidance \(PAG, pag_scale > 0\)"):
        loop.bind((1, 4, 8, 8), True, 7.5, None, pag_scale=3.0)


# ------------------------------------------------------------------------------------------------------------ plans
@pytest.mark.parametrize("twin", [False, True])
@pytest.mark.parametrize("H,W", [(64, 64), (13, 24)])
def test_unpatched_and_disabled_plans_are_the_parents(H, W, twin):
    from powerpaint_amd.runtime import NetRuntime
    never, net = _net(**TINY), _net(**TINY)
    rt0, rt = NetRuntime(never, "cpu"), NetRuntime(net, "cpu")
    rt0.ensure(2, H, W, 77, 4, ("plain",), twin=twin)
    want = (_describe(rt0.step_plan), _describe(rt0.setup_plan), rt0.arena.size, rt0.step_plan.flops, rt0.key)
    rt.ensure(2, H, W, 77, 4, ("plain",), twin=twin)
    before = (_launches(rt, rt.step_plan), _launches(rt, rt.setup_plan))
    net.deepcache = DeepCache(1, 3)
    rt.ensure(2, H, W, 77, 4, ("plain",), twin=twin)
    assert rt.shallow_plan is not None and rt.key != rt0.key
    net.deepcache = None
    rt.ensure(2, H, W, 77, 4, ("plain",), twin=twin)
    assert (_describe(rt.step_plan), _describe(rt.setup_plan), rt.arena.size, rt.step_plan.flops, rt.key) == want
    assert (_launches(rt, rt.step_plan), _launches(rt, rt.setup_plan)) == before          # argument for argument
    assert rt.shallow_plan is None


@pytest.mark.parametrize("twin", [False, True])
def test_patched_plans_of_a_64x64_sd15_unet(twin):
    """SD-1.5 geometry at 64 x 64, B = 8, cache_branch_id 0."""
    from powerpaint_amd.runtime import NetRuntime
    B, H, W = 8, 64, 64
    net = _net()
    rt = NetRuntime(net, "cpu")
    rt.ensure(B, H, W, 77, 4, ("plain",), twin=twin)
    d0, size0 = (_launches(rt, rt.step_plan), _launches(rt, rt.setup_plan)), rt.arena.size
    net.deepcache = DeepCache(0, 3)
    rt.ensure(B, H, W, 77, 4, ("plain",), twin=twin)
    # keeping c needs nothing of the full plan (no FreeU here): the unpatched launches, argument for argument; the shallow
    # plan's tensors lie above them
    assert (_launches(rt, rt.step_plan), _launches(rt, rt.setup_plan)) == d0 and rt.arena.size > size0
    sh, full = rt.shallow_plan, rt.step_plan
    names = [c[2] for c in sh.calls]
    selfattn = [c for c in sh.calls if c[2] == "attention" and list(c[1])[10] == list(c[1])[11]]
    assert len(selfattn) == 3 and names.count("xattn_block") == 3 and names.count("ff_fused") == 3      # three transformers
    assert names.count("conv3x3") == 1 + 2 * 3                                                  # conv_in + three resnets
    assert names.count("groupnorm_stats") == 1                              # c has no producer: its norm takes the stats launch
    rows = {B * H * W, B * H * W // 2}
    for i, (fn, args, name) in enumerate(sh.calls):                          # nothing below the top level
        a = getattr(args[0], "_obj", None) if args else None
        if isinstance(a, L.PPGemmArgs):
            assert a.M in rows, sh.describe(i)
        elif name.startswith("groupnorm"):
            assert args[5] == H * W, name
        elif name == "attention":
            assert args[10] == H * W
        else:
            assert name in ("zero_u64", "timestep_embedding", "linear_skinny", "tfront", "xattn_block", "conv_out"), name
    assert [c for c in sh.calls if c[2] == "conv_out"][0][1][-2] == rt.outputs["eps"]          # eps lands where the full plan's does
    assert sh.flops < full.flops
    print(f"[deepcache] SD-1.5 64x64 B=8 id 0 twin={twin}: shallow / full flops {sh.flops / full.flops:.4f}, "
          f"launches {len(sh.calls)} / {len(full.calls)}, arena {rt.arena.size / size0:.3f} x")
    # cache_interval alone: host schedule, no re-plan
    plans = (rt.step_plan, rt.shallow_plan, rt.key)
    net.deepcache = DeepCache(0, 5)
    rt.ensure(B, H, W, 77, 4, ("plain",), twin=twin)
    assert (rt.step_plan, rt.shallow_plan, rt.key) == plans
    net.deepcache = DeepCache(2, 5)
    rt.ensure(B, H, W, 77, 4, ("plain",), twin=twin)
    assert rt.step_plan is not plans[0] and ("deepcache", 2) in rt.key


def test_side_network_shallow_plans_produce_live_residuals_only():
    from powerpaint_amd.engine import SDNet
    from powerpaint_amd.runtime import NetRuntime
    for kind, extra, live in (("brushnet", dict(conditioning_channels=5), [0, 1, 4 + 1 + 3, 4 + 1 + 4]), ("controlnet", {}, [0, 1])):
        cfg = {k: v for k, v in TINY.items() if not (kind == "controlnet" and k == "up_block_types")}
        net = SDNet(kind, 4, **cfg, **extra)
        net.load_state_dict(net.synthetic_state_dict(meta=True), "cpu", materialize=False)
        net.deepcache = DeepCache(0, 3)
        rt = NetRuntime(net, "cpu")
        for pad in (False, True):
            rt.ensure(2, 16, 16, 77, net.cin0, ("plain",), cond_hw=(128, 128) if kind == "controlnet" else None,
                      scale=[0.1 * (i + 1) for i in range(len(net._zero_conv_specs()))], pad_uncond=pad)
            full, sh = rt.zero_conv_records(), rt.zero_conv_records(rt.shallow_plan)
            assert rt.shallow_plan.zero_conv_pos == live and len(sh) == len(live)
            for a, p in zip(sh, live):                                      # the full plan's buffers and scales, position by position
                assert a.out == full[p].out and a.scale == full[p].scale == pytest.approx(0.1 * (p + 1))
            rt._patch_scale(0.25)
            assert all(a.scale == 0.25 for a in sh + full)


def test_freeu_at_the_cache_point_leaves_c_alone():
    """FreeU rewrites the hidden tensor in place; at the cache point both plans send the scaled copy elsewhere."""
    from powerpaint_amd.runtime import NetRuntime
    net = _net(**TINY)
    net.deepcache = DeepCache(0, 3)
    rt = NetRuntime(net, "cpu")
    rt.ensure(2, 16, 16, 77, 4, ("plain",), freeu=(0.9, 0.2, 1.2, 1.4))
    c = rt.outputs["cache"].ptr
    for plan in (rt.step_plan, rt.shallow_plan):
        fu = [list(cl[1]) for cl in plan.calls if cl[2] == "freeu"]
        at = [a for a in fu if a[0] == c]
        assert len(at) == 1 and at[0][1] != c                               # hidden in: c; hidden out: a tensor of its own
        assert all(a[0] == a[1] for a in fu if a[0] != c)                   # every other FreeU launch: in place, as before


# ------------------------------------------------------------------------------------------------------------ schedule
def _host_tables(cls):
    class Host(cls):
        def _upload(self, device):
            super()._upload(device)
            self._coef_dev = self._coef.clone()
            self._ts_dev = self.timesteps.to(torch.float32).clone()
            self._step_dev = torch.zeros(1, dtype=torch.int32)
    return Host


class _Loop(DenoiseLoop):
    """DenoiseLoop with the network replaced by one named launch per plan (the stub of tests/test_guidance_rescale.py, with a
    shallow plan beside the full one): the assembly and the per-evaluation pick are the real code."""
    deep = True

    def _prepare_runtimes(self, *a, **kw):
        if getattr(self, "_stub", None) is None:
            full, sh = Plan(), Plan()
            full.add("unet", None)
            sh.add("unet_shallow", None)
            self._stub = SimpleNamespace(step_plan=full, shallow_plan=sh if self.deep else None, outputs={"eps": 0x10000},
                                         tome_blocks=lambda: [], ip_scales=lambda: (), net=self.unet.net)
        return self._stub, None, []

    def _head_launches(self, side_rts, rt, *a, shallow=False, **kw):
        return {id(rt): [(None, (), "step_head_shallow" if shallow else "step_head")]}, {id(rt): set()}


def _loop(cls=PS.DDIMScheduler, steps=7, deep=True, **kw):
    sch = _host_tables(cls)(**kw)
    sch.set_timesteps(steps)
    unet = SimpleNamespace(net=SimpleNamespace(tome=None, deepcache=None, params=None), device="cpu")
    loop = _Loop(unet, sch)
    loop.deep = deep
    return loop


def _picked(loop, evaluations):
    return "".join("S" if s else "F" for s in loop.shallow_rows(evaluations))


def test_program_picked_per_evaluation():
    loop = _loop(steps=7)
    loop.bind((1, 4, 8, 8), True, 7.5, None)
    assert loop.program_shallow is not None                                 # the plan is there; the network's setting decides
    assert _picked(loop, 7) == "FFFFFFF"                                    # (a helper that was disabled: every evaluation full)
    loop.unet.net.deepcache = DeepCache(0, 3)
    assert [c[2] for c in loop.program.calls] == ["step_head", "unet", "cfg_sched_step"]
    assert [c[2] for c in loop.program_shallow.calls] == ["step_head_shallow", "unet_shallow", "cfg_sched_step"]
    assert loop.program_shallow.calls[-1] is loop.program.calls[-1]         # one tail: the same step launch, the same counter
    assert _picked(loop, 7) == DC.SCHEDULES[(7, 3)] == DC.schedule(7, 3)
    # 4 Heun steps are 7 rows of the table: every row counts
    heun = _loop(PS.HeunDiscreteScheduler, steps=4)
    heun.bind((1, 4, 8, 8), True, 7.5, None)
    heun.unet.net.deepcache = DeepCache(0, 2)
    rows = int(heun._keep[0].numel())
    assert rows == 7 and _picked(heun, rows) == DC.SCHEDULES[(7, 2)] == DC.schedule(7, 2)
    # strength 0.5 of 6 steps: the pipeline hands the loop the last 3 timesteps; the first evaluation of the call is full
    pipe = PP.StableDiffusionInpaintPipeline(scheduler=PS.DDIMScheduler())
    pipe.scheduler.set_timesteps(6)
    ts, n = pipe.get_timesteps(6, 0.5, "cpu")
    assert n == len(ts) == 3 and _picked(loop, len(ts)) == DC.SCHEDULES[(3, 3)]
    loop.unet.net.deepcache = DeepCache(0, 1)
    assert _picked(loop, 5) == DC.SCHEDULES[(5, 1)]
    # without the patch: no second program
    plain = _loop(deep=False)
    plain.bind((1, 4, 8, 8), True, 7.5, None)
    assert plain.program_shallow is None and _picked(plain, 4) == "FFFF"
    for (ev, iv), want in DC.SCHEDULES.items():
        assert DC.schedule(ev, iv) == want
