"""CPU: the fused loop's program table (powerpaint_amd/pipelines/_loop.py: `_sets`, `_entry`, `_build`, `_set_scales`) on stub
runtimes -- one named launch per plan behind one launch its head replaces, host-side scheduler tables, two stub side runtimes,
so the per-set path of several ControlNets is assembled without a GPU (dry builds: no launch runs in this file)."""
import os
import sys
from types import SimpleNamespace

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from powerpaint_amd import schedulers as PS  # noqa: E402
from powerpaint_amd.engine import DeepCache, Plan  # noqa: E402
from powerpaint_amd.pipelines._loop import DenoiseLoop  # noqa: E402
from test_deepcache import _host_tables  # noqa: E402

SETS = [(0,), (0, 1), (1,), ()]
LIVE = [1]                                  # the zero-conv positions a stub side net's shallow plan keeps, of 2


def _plan(name, flops):
    p = Plan()
    p.add("temb", None)                     # (index 0: the launch the head replaces)
    p.add(name, None)
    p.count(name, flops)
    return p


class _Runtime:
    """A network runtime as far as `bind` and `_build` look: two plans, and for a side net `chained_step_calls`."""

    def __init__(self, name, flops, net):
        self.name, self.net = name, net
        self.step_plan, self.shallow_plan = _plan(name, flops), _plan(name + "_shallow", flops / 4)
        self.shallow_plan.zero_conv_pos = LIVE
        self.outputs = {"eps": 0x10000}

    def tome_blocks(self):
        return []

    def ip_scales(self):
        return ()

    def residual_block(self):
        return 0x20000, 16

    def chained_step_calls(self, target, accumulate, scale, skip=(), shallow=False):
        plan = self.shallow_plan if shallow else self.step_plan
        calls = [(fn, args, name + ("+" if accumulate else "=")) for i, (fn, args, name) in enumerate(plan.calls) if i not in skip]
        return calls, [SimpleNamespace(scale=scale) for _ in (LIVE if shallow else range(2))]


class _Loop(DenoiseLoop):
    def _prepare_runtimes(self, latents_shape, Be, Bs, do_cfg, half, guess_mode, nets, *a, **kw):
        if self.rt is None:
            sides = [_Runtime(f"net{k}", 10.0 * (k + 1), self.unet.net) for k in range(self.n_side)]
            self._stub = _Runtime("unet", 1000.0, self.unet.net), sides
        rt, sides = self._stub
        return rt, (sides[0] if len(sides) == 1 else None), sides

    def _head_launches(self, side_rts, rt, *a, shallow=False, **kw):
        rts = side_rts + [rt]
        return ({id(r): [(None, (), f"head_{r.name}" + ("_shallow" if shallow else ""))] for r in rts},
                {id(r): {0} for r in rts})


def _loop(n_side, **kw):
    sch = _host_tables(PS.DDIMScheduler)()
    sch.set_timesteps(4)
    unet = SimpleNamespace(net=SimpleNamespace(tome=None, deepcache=DeepCache(0, 2), params=None), device="cpu")
    side = None if n_side == 0 else SimpleNamespace() if n_side == 1 else \
        SimpleNamespace(nets=[None] * n_side, per_net=lambda v, name: list(v))
    loop = _Loop(unet, sch, side=side, side_kind="controlnet" if n_side else None, **kw)
    loop.n_side = n_side
    return loop.bind((1, 4, 8, 8), True, 7.5, None, controlnet_cond=[None] * n_side, side_scale=[0.5, 0.8][:n_side] or 1.0)


def _names(prog):
    return [c[2] for c in prog.calls]


def _want(included, shallow, chained):
    """heads of the included side nets, the UNet's head, the side bodies, the UNet's body, the tail"""
    sfx = "_shallow" if shallow else ""
    mark = (lambda n: "+" if n else "=") if chained else (lambda n: "")
    return [f"head_net{k}{sfx}" for k in included] + [f"head_unet{sfx}"] + \
        [f"net{k}{sfx}{mark(n)}" for n, k in enumerate(included)] + (["zero_u64"] if chained and not included else []) + \
        [f"unet{sfx}", "cfg_sched_step"]


def test_every_set_full_and_shallow_is_the_same_concatenation():
    loop = _loop(2)
    assert loop._multi and list(loop._sets) == [(0, 1)] and loop.program is loop._sets[(0, 1)].program[False]
    progs = []
    for st in SETS:
        ent = loop._entry(st)
        assert ent is loop._entry(st) and ent.active == st and list(ent.included) == list(st)
        if ent.program[True] is None:
            loop._build(ent, True)
        for shallow in (False, True):
            prog = ent.program[shallow]
            assert _names(prog) == _want(st, shallow, chained=True), (st, shallow)
            assert prog.flops == sum(10.0 * (k + 1) for k in st) / (4 if shallow else 1) + (250.0 if shallow else 1000.0)
            assert sorted(ent.records[shallow]) == list(st)
            progs.append(prog)
    assert sorted(loop._sets) == sorted(SETS) and len(progs) == 8
    tail = loop._parts[False]["tail"]
    assert loop._parts[True]["tail"] is tail and len(tail) == 1
    for prog in progs:                                  # one tail: the same call tuples, the same step counter
        assert all(a is b for a, b in zip(prog.calls[-len(tail):], tail))
    assert loop.program_shallow is loop._sets[(0, 1)].program[True] and loop.graph is None and loop.graph_shallow is None


def test_keep_closed_nets_includes_every_net():
    loop = _loop(2, keep_closed_nets=True)
    for st in SETS:
        ent = loop._entry(st)
        assert ent.active == st and list(ent.included) == [0, 1]
        assert _names(ent.program[False]) == _want((0, 1), False, chained=True)
    loop._set_scales(loop._entry((1,)), [0.5, 0.8])
    assert loop._entry((1,)).scales == (0.0, 0.8)


def test_scales_reach_both_record_lists_and_drop_both_graphs_of_that_set_alone():
    loop = _loop(2)
    for st in SETS:
        loop._build(loop._entry(st), True)
        loop._entry(st).graph = [f"full {st}", f"shallow {st}"]
    for st in SETS:
        ent = loop._sets[st]
        loop._set_scales(ent, [0.5, 0.8])
        assert ent.graph == [None, None] and ent.scales == tuple([0.5, 0.8][k] for k in st)
        for k in st:
            assert [r.scale for r in ent.records[False][k]] == [[0.5, 0.8][k]] * 2
            assert [r.scale for r in ent.records[True][k]] == [[0.5, 0.8][k]] * len(LIVE)
        for other in SETS[SETS.index(st) + 1:]:         # (not yet written: as captured, as assembled)
            o = loop._sets[other]
            assert o.graph == [f"full {other}", f"shallow {other}"] and o.scales is None
            assert all(r.scale == 0.0 for sh in (False, True) for recs in o.records[sh].values() for r in recs)
        ent.graph = ["again", "again"]
        loop._set_scales(ent, [0.5, 0.8])               # the same values: nothing to drop
        assert ent.graph == ["again", "again"]
        loop._set_scales(ent, [0.25, 0.4])
        assert ent.graph == ([None, None] if st else ["again", "again"])         # (the empty set carries no scale)
        ent.graph = [None, None]
    # the guess-mode ramp, per residual; the shallow records take the live positions' values
    loop._guess_ramp = [0.1, 1.0]
    ent = loop._sets[(0, 1)]
    loop._set_scales(ent, [0.5, 0.8])
    assert [r.scale for r in ent.records[False][1]] == [0.1 * 0.8, 1.0 * 0.8]
    assert [r.scale for r in ent.records[True][1]] == [1.0 * 0.8]


@pytest.mark.parametrize("n_side", [0, 1, 2])
def test_single_entry_and_per_set_loops_share_one_assembly(n_side, monkeypatch):
    built = []
    real = DenoiseLoop._build
    monkeypatch.setattr(DenoiseLoop, "_build", lambda self, ent, shallow: built.append((ent.active, shallow)) or real(self, ent, shallow))
    loop = _loop(n_side)
    every = tuple(range(n_side))
    assert built == [(every, False), (every, True)] and list(loop._sets) == [every] == [loop._all]
    assert loop._multi == (n_side > 1)
    assert _names(loop.program) == _want(every, False, chained=n_side > 1)
    assert _names(loop.program_shallow) == _want(every, True, chained=n_side > 1)
    assert loop.program_shallow.calls[-1] is loop.program.calls[-1]
    assert loop.program.flops == 1000.0 + sum(10.0 * (k + 1) for k in every)
    program = loop.program
    assert loop.bind((1, 4, 8, 8), True, 7.5, None, controlnet_cond=[None] * n_side,
                     side_scale=[0.5, 0.8][:n_side] or 1.0).program is program and len(built) == 2      # an equal key: nothing rebuilt
    if n_side > 1:
        loop._entry((1,))
        assert built[2:] == [((1,), False)]              # a set's shallow program: on demand
