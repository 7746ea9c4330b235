"""The fused loop's step dispatch on the GPU (powerpaint_amd/pipelines/_loop.py: `_resolve`, `_launch`): what every step of a
call replays is resolved before the first step, for this package's schedulers and for a duck-typed one alike -- so a call that
replays captured graphs and one that launches the same programs eagerly leave the same latents, bit for bit.  Tiny networks
(320/640 channels, 8 x 8 latents), 4 steps; {DDIM, a scheduler outside the package} x {one ControlNet, two ControlNets whose
guidance windows differ} x {DeepCache off, cache_interval 2}.  With DeepCache the two nets stay one set for the call (a changing
set is refused, which the last test holds)."""
import functools

import pytest
import torch

from powerpaint_amd import _lib as L
from powerpaint_amd import models as PM, pipelines as PP, schedulers as PS
from powerpaint_amd.engine import DeepCache
from powerpaint_amd.pipelines._loop import DenoiseLoop

pytestmark = pytest.mark.gpu
DEV = "cuda"
TINY = dict(block_out_channels=(320, 640), layers_per_block=1, down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
            up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"))
NO_UP = {k: v for k, v in TINY.items() if k != "up_block_types"}
B, S, STEPS = 1, 8, 4
WINDOWS = PP.StableDiffusionControlNetInpaintPipeline.control_schedule(STEPS, [0.5, 0.8], [0.0, 0.25], [0.5, 0.75])


class Duck:
    """A scheduler outside the package: the diffusers protocol, nothing else."""
    order, init_noise_sigma = 1, 1.0

    def __init__(self):
        self.timesteps = torch.tensor([801, 601, 401, 201])

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step(self, model_output, timestep, sample, generator=None, return_dict=True):
        return (sample - 0.1 * model_output,)


@functools.lru_cache(maxsize=None)
def _nets():
    def net(cls, seed, **kw):
        m = cls(device=DEV, **kw)
        return m.load_state_dict(m.net.synthetic_state_dict(device=DEV, seed=seed))
    return net(PM.UNet2DConditionModel, 0, in_channels=9, **TINY), [net(PM.ControlNetModel, 3 + i, in_channels=4, **NO_UP)
                                                                    for i in range(2)]


@functools.lru_cache(maxsize=None)
def _inputs():
    g = torch.Generator().manual_seed(0)
    mask = torch.zeros(B, 1, S, S)
    mask[:, :, 2:6, 1:5] = 1
    return dict(lat=torch.randn(B, 4, S, S, generator=g).to(DEV), mask=mask.to(DEV),
                mil=(torch.randn(B, 4, S, S, generator=g) * 0.5).to(DEV), pe=torch.randn(2 * B, 77, 768, generator=g).to(DEV),
                imgs=[torch.rand(B, 3, 8 * S, 8 * S, generator=g).to(DEV) for _ in range(2)])


def _loop(sched, n_nets):
    unet, cnets = _nets()
    sch = Duck() if sched == "duck" else PS.DDIMScheduler()
    if sched != "duck":
        sch.set_timesteps(STEPS, device=DEV)
    side = cnets[0] if n_nets == 1 else PM.MultiControlNetModel(cnets)
    i = _inputs()
    loop = DenoiseLoop(unet, sch, side=side, side_kind="controlnet")
    return loop.bind((B, 4, S, S), True, 7.5, i["pe"], prompt_embeds_side=i["pe"], static_inputs=[(i["mask"], 4), (i["mil"], 5)],
                     controlnet_cond=i["imgs"][0] if n_nets == 1 else i["imgs"], side_scale=0.7 if n_nets == 1 else [0.5, 0.8])


@pytest.fixture
def deepcache(request):
    unet, cnets = _nets()
    for m in [unet] + cnets:
        m.net.deepcache = DeepCache(0, 2) if request.param else None
    yield request.param
    for m in [unet] + cnets:
        m.net.deepcache = None


@pytest.mark.parametrize("deepcache", [False, True], indirect=True, ids=["plain", "deepcache"])
@pytest.mark.parametrize("n_nets", [1, 2])
@pytest.mark.parametrize("sched", ["ddim", "duck"])
def test_graph_replay_and_eager_launches_leave_the_same_latents(sched, n_nets, deepcache):
    loop = _loop(sched, n_nets)
    rows = [0.7] * STEPS if n_nets == 1 else [[0.5, 0.8]] * STEPS if deepcache else WINDOWS
    lat = _inputs()["lat"]
    graph = loop.run(lat, STEPS, use_graph=True, scale_schedule=rows).clone()
    assert loop.shallow_rows(STEPS) == ([False, True, False, True] if deepcache else [False] * STEPS)
    used = [ent for ent in loop._sets.values() if ent.graph[False] is not None]
    assert len(used) == (len({tuple(k for k, v in enumerate(r) if v != 0.0) for r in rows}) if n_nets == 2 else 1)
    assert all((ent.graph[True] is not None) == deepcache for ent in used)
    eager = loop.run(lat, STEPS, use_graph=False, scale_schedule=rows).clone()
    assert bool(torch.isfinite(graph).all()) and not torch.equal(graph, lat)
    assert torch.equal(graph, eager), f"{sched}, {n_nets} ControlNet(s), DeepCache {deepcache}: max diff {(graph - eager).abs().max()}"
    assert torch.equal(loop.run(lat, STEPS, use_graph=True, scale_schedule=rows), graph)        # the captured graphs, again


@pytest.mark.parametrize("deepcache", [True], indirect=True, ids=["deepcache"])
@pytest.mark.parametrize("sched", ["ddim", "duck"])
def test_deepcache_with_a_changing_set_of_controlnets_is_still_refused(sched, deepcache):
    loop = _loop(sched, 2)
    for use_graph in (True, False):
        with pytest.raises(L.PPError, match="DeepCache with several ControlNets whose set of active nets changes"):
            loop.run(_inputs()["lat"], STEPS, use_graph=use_graph, scale_schedule=WINDOWS)
