"""ControlNetModel (SD-1.5 canny/depth/hed/openpose) on the MI355X HIP path.

The reference uses the stock diffusers-0.27.0 class (built at /root/reference/app.py:121-123, called at
/root/reference/powerpaint/pipelines/pipeline_PowerPaint_ControlNet.py:1686-1694).  Returns `(list[12], Tensor)`.
The conditioning embedding of `controlnet_cond` is step-invariant and is computed once per distinct tensor.
"""
from types import SimpleNamespace
from typing import List, Sequence, Union

import torch

from .. import _lib as L
from ..engine import Plan
from ._base import SD15_DOWN, Output, _HipModel


class ControlNetModel(_HipModel):
    kind = "controlnet"

    def __init__(self, in_channels: int = 4, conditioning_channels: int = 3, down_block_types=SD15_DOWN,
                 block_out_channels=(320, 640, 1280, 1280), layers_per_block: int = 2, norm_num_groups: int = 32,
                 norm_eps: float = 1e-5, cross_attention_dim: int = 768, attention_head_dim: int = 8,
                 conditioning_embedding_out_channels=(16, 32, 96, 256), device="cuda", dtype=torch.bfloat16, **unused):
        self._extra_config = unused         # validated in the base constructor (check_fixed_config)
        super().__init__(in_channels, block_out_channels, layers_per_block, attention_head_dim, cross_attention_dim,
                         norm_num_groups, norm_eps, down_block_types, (), device, dtype,
                         conditioning_channels=conditioning_channels,
                         cond_embed_channels=conditioning_embedding_out_channels)
        self.config = SimpleNamespace(
            in_channels=in_channels, conditioning_channels=conditioning_channels,
            down_block_types=tuple(down_block_types), block_out_channels=tuple(block_out_channels),
            layers_per_block=layers_per_block, norm_num_groups=norm_num_groups, norm_eps=norm_eps,
            cross_attention_dim=cross_attention_dim, attention_head_dim=attention_head_dim,
            conditioning_embedding_out_channels=tuple(conditioning_embedding_out_channels),
            global_pool_conditions=False)

    def prepare(self, sample_shape, encoder_hidden_states, controlnet_cond, conditioning_scale=1.0,
                guess_mode: bool = False, pad_uncond: bool = False, twin: bool = False):
        """pad_uncond: outputs laid out as `cat([zeros_like(d), d])` for a UNet running the CFG pair (the pipeline's guess
        mode, pipeline_PowerPaint_ControlNet.py:1697-1702)."""
        B, Cin, H, W = sample_shape
        scale = conditioning_scale
        if guess_mode and not self.config.global_pool_conditions:
            n = len(self.net._zero_conv_specs())
            scale = [float(s) * conditioning_scale for s in torch.logspace(-1, 0, n)]
        self.rt.ensure(B, H, W, self._nctx(encoder_hidden_states), Cin, ("plain",),
                       cond_hw=tuple(controlnet_cond.shape[-2:]), scale=scale, pad_uncond=pad_uncond, twin=twin)
        self.rt.set_cond(controlnet_cond)
        self.rt.set_context(encoder_hidden_states)
        return self.rt

    def outputs(self):
        o = self.rt.outputs
        v = self.rt.act_as_nchw
        return [v(a) for a in o["down"]], v(o["mid"])

    @torch.no_grad()
    def forward(self, sample: torch.FloatTensor, timestep: Union[torch.Tensor, float, int],
                encoder_hidden_states: torch.Tensor, controlnet_cond: torch.FloatTensor,
                conditioning_scale: float = 1.0, class_labels=None, timestep_cond=None, attention_mask=None,
                added_cond_kwargs=None, cross_attention_kwargs=None, guess_mode: bool = False,
                return_dict: bool = True):
        for name, v in (("class_labels", class_labels), ("timestep_cond", timestep_cond),
                        ("attention_mask", attention_mask)):
            if v is not None:
                raise NotImplementedError(f"{name} is outside the PowerPaint hot path")
        if isinstance(conditioning_scale, (list, tuple)):
            conditioning_scale = conditioning_scale[0]
        rt = self.prepare(tuple(sample.shape), encoder_hidden_states, controlnet_cond, float(conditioning_scale),
                          guess_mode)
        rt.load_input([(sample, 0)])
        rt.set_timestep(timestep)
        rt.run_step()
        down, mid = self.outputs()
        if not return_dict:
            return (down, mid)
        return Output(down_block_res_samples=down, mid_block_res_sample=mid)

    __call__ = forward


class MultiControlNetModel:
    """Several ControlNets whose residuals are summed before the UNet sees them: the diffusers-0.27 wrapper the
    reference builds from a list (/root/reference/powerpaint/pipelines/pipeline_PowerPaint_ControlNet.py:281,306) and
    calls once per step with one control image and one scale per net (:1686-1694).  Same duck type: `.nets`, `.dtype`,
    `.device`, `.to()`, `forward(...)` -> `(down_block_res_samples, mid_block_res_sample)`.

    Every net runs its own launch plan on the same sample; the sum is formed in the zero convs' epilogues: net 0 writes
    its residual buffers, every later net adds into them in place (NetRuntime.chained_step_calls) -- no add launch, no
    extra pass over the residual tensors.  The 16-bit result is rounded once where the reference rounds every net's
    residual and then every partial sum.  There is no `from_pretrained` for the wrapper: load each net with
    `ControlNetModel.from_pretrained` and pass the list."""

    def __init__(self, controlnets: Sequence[ControlNetModel]):
        nets = list(controlnets)
        if not nets:
            raise L.PPError("MultiControlNetModel needs at least one ControlNetModel")
        for i, n in enumerate(nets):
            if not isinstance(n, ControlNetModel):
                raise L.PPError(f"MultiControlNetModel: entry {i} is a {type(n).__name__}, not a ControlNetModel")
        first = nets[0]
        for i, n in enumerate(nets[1:], 1):
            if n.dtype != first.dtype:
                raise L.PPError(f"MultiControlNetModel: net {i} computes in {n.dtype}, net 0 in {first.dtype}: the residuals "
                                f"are summed in one 16-bit buffer, load every net with the same torch_dtype")
            if n.device != first.device:
                raise L.PPError(f"MultiControlNetModel: net {i} lives on {n.device}, net 0 on {first.device}")
            for key in ("block_out_channels", "layers_per_block", "down_block_types"):
                a, b = getattr(n.config, key), getattr(first.config, key)
                if a != b:
                    raise L.PPError(f"MultiControlNetModel: net {i} has {key}={a}, net 0 has {b}: the nets must "
                                    f"produce residuals of the same shapes")
        self.nets: List[ControlNetModel] = nets
        self._plans = {}

    @property
    def dtype(self):
        return self.nets[0].dtype

    @property
    def device(self):
        return self.nets[0].device

    def to(self, *a, **k):
        for n in self.nets:
            n.to(*a, **k)
        return self

    def eval(self):
        return self

    def per_net(self, value, what: str) -> list:
        """A `forward` argument given per net: a list / tuple of len(nets)."""
        if not isinstance(value, (list, tuple)) or len(value) != len(self.nets):
            raise L.PPError(f"MultiControlNetModel: `{what}` must be a list of {len(self.nets)} entries (one per net)")
        return list(value)

    @torch.no_grad()
    def forward(self, sample: torch.FloatTensor, timestep: Union[torch.Tensor, float, int],
                encoder_hidden_states: torch.Tensor, controlnet_cond: List[torch.Tensor],
                conditioning_scale: List[float], class_labels=None, timestep_cond=None, attention_mask=None,
                added_cond_kwargs=None, cross_attention_kwargs=None, guess_mode: bool = False,
                return_dict: bool = True):
        for name, v in (("class_labels", class_labels), ("timestep_cond", timestep_cond),
                        ("attention_mask", attention_mask)):
            if v is not None:
                raise NotImplementedError(f"{name} is outside the PowerPaint hot path")
        conds = self.per_net(controlnet_cond, "controlnet_cond")
        scales = [float(s) for s in self.per_net(conditioning_scale, "conditioning_scale")]
        if len(self.nets) == 1:                                 # one net: that net's own plan, nothing redirected
            return self.nets[0].forward(sample, timestep, encoder_hidden_states, conds[0], scales[0],
                                        guess_mode=guess_mode, return_dict=False)
        rts = []
        for net, cond, sc in zip(self.nets, conds, scales):
            rt = net.prepare(tuple(sample.shape), encoder_hidden_states, cond, sc, guess_mode)
            rt.load_input([(sample, 0)])
            rt.set_timestep(timestep)
            rts.append(rt)
        key = tuple(id(rt.step_plan) for rt in rts)
        ent = self._plans.get(key)
        if ent is None:
            self._plans.clear()                                 # (plans of other shapes hold pointers into rebuilt arenas)
            plan = Plan()
            recs = []
            for k, rt in enumerate(rts):
                calls, r = rt.chained_step_calls(rts[0], accumulate=k > 0, scale=rt._scale)
                plan.calls += calls
                recs.append(r)
            plan.keep = [rt.step_plan for rt in rts]
            ent = self._plans[key] = (plan, recs)
        plan, recs = ent
        for rt, rec in zip(rts, recs):                          # this call's scales (by value in the launch records)
            vals = list(rt._scale) if isinstance(rt._scale, (list, tuple)) else [rt._scale] * len(rec)
            for r, v in zip(rec, vals):
                r.scale = float(v)
        plan.run(torch.cuda.current_stream().cuda_stream)
        return self.nets[0].outputs()

    __call__ = forward
