"""Per-network runtime: static arena, compiled launch plans, step-invariant setup, optional hipGraph replay."""
from typing import Dict, List, Optional, Sequence, Tuple

import ctypes as C

import torch

from . import _lib as L
from .engine import Act, Arena, Builder, Plan, SDNet, TOME_TABLE_ROWS, _align, level_sizes

_DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class NetRuntime:
    """Owns the device state of one SDNet for one (batch, latent size, wiring)."""

    def __init__(self, net: SDNet, device):
        self.net = net
        self.device = torch.device(device)
        self.key = None
        self.arena: Optional[Arena] = None
        self.step_plan: Optional[Plan] = None
        self.shallow_plan: Optional[Plan] = None       # DeepCache: the shallow form of the step (None without it)
        self.dc_eval = 0
        self.setup_plan: Optional[Plan] = None
        self.outputs: Dict[str, object] = {}
        self._ctx_id = None
        self._cond_id = None
        self._ctx_keep = None
        self._cond_keep = None
        self.graph = None
        self.lib = L.lib()
        self.gemm_tile = 0
        self.gemm_splitk = 0

    # ------------------------------------------------------------------ build
    def _ip_cells(self, n: int):
        """One ctypes.c_float per loaded IP-Adapter: the by-value `ip_scale` of its pp_ip_attn_add launches.  The cells outlive
        the plans (a rebuilt plan keeps the scales that were set)."""
        cells = self.__dict__.setdefault("_ip_scale_cells", [])
        del cells[n:]
        while len(cells) < n:
            cells.append(C.c_float(1.0))
        return cells

    def set_ip_scales(self, scales: Sequence[float]):
        """Per-adapter scales: eager runs see the new values at once; a captured graph carries by-value arguments, so this
        runtime's graph is dropped and `ip_scales()` tells a loop that captured the plan inside its own graph to re-capture."""
        cells = self._ip_cells(len(scales))
        if [c.value for c in cells] != [C.c_float(float(v)).value for v in scales]:
            for c, v in zip(cells, scales):
                c.value = float(v)
            self.graph = None

    def ip_scales(self) -> Tuple[float, ...]:
        return tuple(c.value for c in self.__dict__.get("_ip_scale_cells", [])[:len(getattr(self.net, "ip", []))])

    def set_ip_embeds(self, embeds: Optional[Sequence[torch.Tensor]]):
        """The call's image embeds, one [B, n, D] (base) or [B, n, S, E] (Plus) tensor per loaded adapter, copied into the setup plan's inputs; the setup plan
        runs again at the next set_context (the embeds change per call: they are never assumed unchanged)."""
        if "ip_in" not in self.lay:
            return
        for i, (entry, spec, e) in enumerate(zip(self.lay["ip_in"], self.net.ip, embeds)):
            (ptr, n), (T, D) = entry[:2], spec[:2]
            if len(spec) > 2:
                # Plus: the hidden states [B n S][E rounded up to 64] (the pad columns stay the arena's zeros), and the adapter's
                # latents repeated over the B n images -- the residual stream the Resampler's first layer reads
                # (device-to-device from the packed buffer; no launch of the plan)
                S, lat = entry[2], entry[3]
                dst = self.arena.view(ptr, (self.B * n * S, D), self.net.dtype, strides=(_align(D, 64), 1))
                dst.copy_(e.reshape(self.B * n * S, D).to(self.device))
                src = self.net.params.tensor(f"ip_adapter.{i}.resampler.latents")
                self.arena.view(lat, (self.B * n, T, spec.dim), self.net.dtype).copy_(src.unsqueeze(0).expand(self.B * n, -1, -1))
                continue
            dst = self.arena.view(ptr, (self.B * n, D), self.net.dtype, strides=(_align(D, 64), 1))
            dst.copy_(e.reshape(self.B * n, D).to(self.device))
        self._ctx_id = None

    def _xattn_queries(self, H: int, W: int) -> List[int]:
        """The distinct query counts per batch item (h * w) of the levels that hold a cross-attention, largest first."""
        n = len(self.net.boc)
        sizes = level_sizes(H, W, n)
        out = set()
        for pre, _ in self.net._attn_specs():
            part = pre.split(".")
            lvl = n - 1 if part[0] == "mid_block" else (int(part[1]) if part[0] == "down_blocks" else n - 1 - int(part[1]))
            out.add(sizes[lvl][0] * sizes[lvl][1])
        return sorted(out, reverse=True)

    def set_ip_masks(self, masks: torch.Tensor):
        """`ip_adapter_masks` [adapters, 1, H, W] -> the per-row weights the masked pp_ip_attn_add launches read: per adapter
        and distinct query count, IPAdapterMaskProcessor.downsample(mask_i, 1, nq, 1) (host torch: a few small bicubic
        resizes per call) written into the plan's fp32 buffers.  Stream-ordered writes to memory the kernels READ: eager runs
        and replays of a captured graph queued after this call see the new values, nothing is re-captured."""
        from .pipelines.image_processor import IPAdapterMaskProcessor
        bufs = self.lay.get("ip_row_w")
        if not bufs:
            raise L.PPError("set_ip_masks: the plan was built without ip_adapter_masks (NetRuntime.ensure(ip_masked=True))")
        if len(masks) != len(self.net.ip):
            raise ValueError(f"Number of ip_adapter_masks ({len(masks)}) must match number of IP-Adapters ({len(self.net.ip)})")
        m = masks.detach().to(device="cpu", dtype=torch.float32)
        for nq, ptrs in bufs.items():
            for i, ptr in enumerate(ptrs):
                w = IPAdapterMaskProcessor.downsample(m[i], 1, nq, 1).reshape(nq)
                self.arena.view(ptr, (nq,), torch.float32).copy_(w)

    def _build(self, arena: Arena, B, H, W, nctx, cin_total, wiring, cond_hw, scale, pad_uncond=False, twin=False,
               freeu=False, ip_n=(), ip_masked=False, pag=None):
        net = self.net
        pb_setup = Builder(arena, dtype=net.dtype)
        pb_setup.gemm_tile, pb_setup.gemm_splitk = self.gemm_tile, self.gemm_splitk
        lay = {}
        lay["t_dev"] = arena.alloc(256)
        # int64 accumulators of the GroupNorm statistics the GEMM epilogues produce (<= 96 norms per network); zeroed
        # by the first launch of every step
        gn_cap = 96 * B * 32 * 2 * 8
        lay["gn_acc"] = arena.alloc(gn_cap)
        lay["fault"] = arena.alloc(256)          # placement violations seen by the in-kernel split-K combines (check_faults)
        # network input, NHWC; the channels are zero-padded to one 64-deep K chunk (conv_in runs on the implicit-GEMM
        # kernel).  The arena is zero-filled and nothing else ever writes the pad channels.
        if cin_total != net.cin0:
            raise L.PPError(f"{net.kind} takes {net.cin0} input channels, got {cin_total}")
        lay["x_in"] = Act(arena.alloc(B * H * W * net.cin_pad * 2), B, H, W, net.cin_pad)
        lay["ehs"] = arena.alloc(B * nctx * net.ctx_dim * 2)
        cond = None
        if net.kind == "controlnet":
            ch, cw = cond_hw
            cond = Act(arena.alloc(B * ch * cw * net.conditioning_channels * 2), B, ch, cw, net.conditioning_channels)
            lay["cond"] = cond
        # slots for foreign residual tensors (copied in at forward time)
        kind, n_down, n_up = wiring[0], 0, 0
        slots: Dict[str, List[Act]] = {}
        if kind in ("brushnet", "controlnet") and net.kind == "unet":
            shapes = self._residual_shapes(B, H, W, with_up=(kind == "brushnet"))
            slots = {k: [Act(arena.alloc(b * h * w * c * 2), b, h, w, c) for (b, c, h, w) in v]
                     for k, v in shapes.items()}
        lay["slots"] = slots
        ip_kw = {}
        if getattr(net, "ip", None):
            # IP-Adapters: the call's image embeds, 16-bit [B][n][D rounded up to 64] per adapter (set_ip_embeds; the pad columns
            # stay the arena's zeros), and one by-value scale cell per adapter shared by all its launches (set_ip_scales)
            if len(ip_n) != len(net.ip):
                raise L.PPError(f"{len(net.ip)} IP-Adapters are loaded: the plan needs the image count of each")
            # (a Plus adapter's ip_n entry is (n, S): S hidden states of width D per image, and its latents repeated B n times)
            lay["ip_in"] = []
            for spec, n in zip(net.ip, ip_n):
                T, D = spec[:2]
                if len(spec) > 2:
                    n, S = n
                    lay["ip_in"].append((arena.alloc(B * n * S * _align(D, 64) * 2), n, S, arena.alloc(B * n * T * spec.dim * 2)))
                else:
                    lay["ip_in"].append((arena.alloc(B * n * _align(D, 64) * 2), n))
            ip_kw = dict(ip_in=lay["ip_in"], ip_scales=self._ip_cells(len(net.ip)))
            if ip_masked:
                # ip_adapter_masks: fp32 [nq] per adapter and distinct query count; the transformers of a level share it
                lay["ip_row_w"] = {nq: [arena.alloc(nq * 4) for _ in net.ip] for nq in self._xattn_queries(H, W)}
                ip_kw["ip_row_w"] = lay["ip_row_w"]
        net.build_setup(pb_setup, B, nctx, lay["ehs"], cond, hw0=(H, W), **ip_kw)
        pb = Builder(arena, dtype=net.dtype)
        pb.gemm_tile, pb.gemm_splitk = self.gemm_tile, self.gemm_splitk
        pb.gn_acc_base, pb.gn_acc_cap = lay["gn_acc"], gn_cap
        pb.fault_ptr = lay["fault"]
        kw = {}
        if net.kind == "unet" and kind == "brushnet":
            ptrs = wiring[1]
            dn = [p if p else s.ptr for p, s in zip(ptrs["down"], slots["down"])]
            up = [p if p else s.ptr for p, s in zip(ptrs["up"], slots["up"])]
            md = ptrs["mid"][0] if ptrs["mid"][0] else slots["mid"][0].ptr
            kw = dict(add_down=dn, add_mid=md, add_up=up)
        elif net.kind == "unet" and kind == "controlnet":
            ptrs = wiring[1]
            dn = [p if p else s.ptr for p, s in zip(ptrs["down"], slots["down"])]
            md = ptrs["mid"][0] if ptrs["mid"][0] else slots["mid"][0].ptr
            kw = dict(ctrl_down=dn, ctrl_mid=md)
        if freeu:
            # FreeU's (b1, s1, b2, s2), fp32: the pp_freeu launches READ them, so new values reach a captured graph as a
            # 16-byte write (set_freeu), with no re-capture
            lay["freeu"] = arena.alloc(256)
            kw["freeu"] = lay["freeu"]
        if getattr(net, "time_cond_proj_dim", None):
            # guidance embedding c, Wc c and the effective linear_1 bias b1 + W1 (Wc c), fp32 (set_timestep_cond)
            lay["tcond"] = arena.alloc(net.time_cond_proj_dim * 4)
            lay["tcond_mid"] = arena.alloc(net.boc[0] * 4)
            lay["b1_eff"] = arena.alloc(net.boc[0] * 4 * 4)
            kw["b1_eff"] = lay["b1_eff"]
        layout, stride = net.tome_layout(H, W)
        if layout:
            # token merging: the window table uint8 [evaluations][stride] (one segment per merging block), the device word that
            # names the row (the launches read it through `_tome_row`, a cell holding the POINTER: a denoising loop points it
            # at its own step counter), and per block the decisions of the last evaluation (tome_decisions)
            lay["tome"] = dict(layout=layout, stride=stride, rows=TOME_TABLE_ROWS, table=arena.alloc(TOME_TABLE_ROWS * stride),
                               word=arena.alloc(256), row=self._tome_row,
                               bufs={pre: tuple(arena.alloc(B * b.h * b.w * 4) for _ in range(3)) for pre, b in layout.items()})
            kw["tome"] = lay["tome"]
        if pag is not None:
            kw["pag"] = pag
        if pad_uncond:
            if net.kind == "unet":
                raise L.PPError("pad_uncond is an output layout of the side networks (BrushNet / ControlNet)")
            kw["pad_uncond"] = True
        dc = getattr(net, "deepcache", None)
        if dc is not None:
            kw["depth"] = int(dc.branch) + 1
        outs = net.build_step(pb, lay["x_in"], lay["t_dev"], scale=1.0, twin=twin, **kw)
        if pb.gn_acc_used:
            pb.plan.calls.insert(0, (L.lib().pp_zero_u64, (lay["gn_acc"], pb.gn_acc_used // 8), "zero_u64"))
        # what build_step recorded (Builder.taps; DESIGN.md "Taps"): block outputs, and tensors inside blocks with the entry of
        # plan.calls that completes each (the tuple, so the launch inserted above moves nothing)
        lay["taps"] = pb.taps
        if dc is not None:
            # DeepCache: the shallow form of the same walk, a plan of its own on the same arena.  Its tensors lie ABOVE everything
            # the full plan allocated: nothing it writes can touch c (which lives among the full plan's tensors), the setup
            # plan's outputs or the input / residual slots.  The accumulator pool is shared -- every plan zeroes what it uses
            # with its first launch, and nothing cached lives there.
            ps = Builder(arena, dtype=net.dtype)
            ps.gemm_tile, ps.gemm_splitk = self.gemm_tile, self.gemm_splitk
            ps.gn_acc_base, ps.gn_acc_cap = lay["gn_acc"], gn_cap
            ps.fault_ptr = lay["fault"]
            net.build_step(ps, lay["x_in"], lay["t_dev"], scale=1.0, twin=twin, cached=outs, **kw)
            if ps.gn_acc_used:
                ps.plan.calls.insert(0, (L.lib().pp_zero_u64, (lay["gn_acc"], ps.gn_acc_used // 8), "zero_u64"))
            lay["shallow_plan"] = ps.plan
        return lay, pb_setup.plan, pb.plan, outs

    def _residual_shapes(self, B, H, W, with_up: bool):
        """(batch, C, h, w) of the residual tensors the UNet accepts, in reference order."""
        net = self.net
        boc = net.boc
        sizes = level_sizes(H, W, len(boc))
        down = [(B, boc[0], H, W)]
        for i, c in enumerate(boc):
            h, w = sizes[i]
            for _ in range(net.L):
                down.append((B, c, h, w))
            if i != len(boc) - 1:
                h, w = sizes[i + 1]
                down.append((B, c, h, w))
        out = {"down": down, "mid": [(B, boc[-1], h, w)]}
        if with_up:
            up = []
            for i, c in enumerate(reversed(boc)):
                for _ in range(net.L + 1):
                    up.append((B, c, h, w))
                if i != len(boc) - 1:
                    h, w = sizes[len(boc) - 2 - i]
                    up.append((B, c, h, w))
            out["up"] = up
        return out

    def ensure(self, B: int, H: int, W: int, nctx: int, cin_total: int, wiring=("plain",), cond_hw=None,
               scale: float = 1.0, pad_uncond: bool = False, twin: bool = False, freeu=None, ip_n=(),
               ip_masked: bool = False, pag=None):
        """pag: None, or the engine.PAG setting of a UNet (the transformers whose self-attention is the identity for the last
        pag.n batch items) -- part of the plan key; without it the key and the plan of a network that never had it.  Refused
        together with token merging.
        freeu: None, or (s1, s2, b1, b2) of UNet2DConditionModel.enable_freeu -- on / off is part of the plan key (the
        plan gains one pp_freeu launch per resnet of up blocks 0 and 1), the values live in device memory the launches read.
        ip_n: images per loaded IP-Adapter in this call's embeds, (images, hidden states per image) for a Plus adapter (part of
        the key only while adapters are loaded).
        ip_masked: `ip_adapter_masks` are bound (all adapters or none, as in diffusers 0.27) -- every pp_ip_attn_add launch is
        then the masked entry, reading per-row weights that set_ip_masks fills; part of the key, the values are not.
        twin: the caller vouches that the second half of every network input (x_in, ControlNet conditioning) equals the
        first -- a CFG pair built from one tensor; the step plan then runs the prompt-independent prefix on one half
        (SDNet.build_step)."""
        def freeze(w):
            if len(w) == 1:
                return w
            return (w[0], tuple((k, tuple(v)) for k, v in sorted(w[1].items())))

        key = (B, H, W, nctx, cin_total, freeze(wiring), cond_hw, self.gemm_tile, self.gemm_splitk, bool(pad_uncond),
               bool(twin)) + (("freeu",) if freeu is not None else ())      # (without FreeU: the key of a plan that never had it)
        ip = getattr(getattr(self, "net", None), "ip", None)
        if ip:
            key += (("ip", tuple(ip), tuple(tuple(int(v) for v in n) if isinstance(n, (tuple, list)) else int(n) for n in ip_n),
                     bool(ip_masked)),)
        elif ip_masked:
            raise L.PPError("ip_adapter_masks need a loaded IP-Adapter")
        tm = getattr(getattr(self, "net", None), "tome", None)
        if tm is not None:                                       # (without token merging: the key of a plan that never had it)
            key += (("tome", tuple(tm)),)
        ht = getattr(getattr(self, "net", None), "hypertile", None)
        if ht is not None:                                       # (without HyperTile: the key of a plan that never had it)
            if tm is not None:
                raise L.PPError("HyperTile together with token merging (ToMe) on the same network is not implemented")
            key += (("hypertile", tuple(ht)),)
        if pag is not None:
            if tm is not None and tm.ratio > 0:
                from .pag import check_supported
                check_supported(tome=True)
            key += (("pag", tuple(pag.layers), int(pag.n)),)
        dc = getattr(getattr(self, "net", None), "deepcache", None)
        if dc is not None:                                       # (without DeepCache: the key of a plan that never had it)
            if tm is not None:
                raise L.PPError("DeepCache together with token merging (ToMe) on the same network is not implemented")
            if pag is not None:
                raise L.PPError("DeepCache together with perturbed-attention guidance (PAG, pag_scale > 0) is not implemented")
            key += (("deepcache", int(dc.branch)),)               # (cache_interval is host schedule: no part of the key)
        if isinstance(scale, (list, tuple)):
            scale = tuple(float(v) for v in scale)       # (one representation: a list never equals the stored tuple)
        if key == self.key:
            if scale != self._scale:
                self._patch_scale(scale)
            self.set_freeu(freeu)
            return
        # (the one synchronising probe of the library runs here, at plan-build time and never under a stream capture: are
        #  workgroups placed on the XCDs round-robin by linear id?  Plans combine split-K in-kernel only if so.)
        self.xcd_placement_ok = bool(self.lib.pp_xcd_placement_ok())
        self._tome_row = C.c_void_p(0)
        dry = Arena()
        self._build(dry, B, H, W, nctx, cin_total, wiring, cond_hw, scale, pad_uncond, twin, freeu is not None, ip_n,
                    bool(ip_masked), pag)
        self.arena = Arena(_align(dry.peak, 4096), self.device)
        self.lay, self.setup_plan, self.step_plan, self.outputs = self._build(
            self.arena, B, H, W, nctx, cin_total, wiring, cond_hw, scale, pad_uncond, twin, freeu is not None, ip_n,
            bool(ip_masked), pag)
        self.shallow_plan = self.lay.pop("shallow_plan", None)
        self.dc_eval = 0                                # evaluations since the plans were built / the helper was enabled
        self.twin = bool(twin)
        self.pad_uncond = bool(pad_uncond)
        self.key = key
        self._scale = 1.0
        if scale != 1.0:
            self._patch_scale(scale)
        self._ctx_id = None
        self._cond_id = None
        self._ctx_keep = self._cond_keep = None
        self.graph = None
        self.B, self.H, self.W, self.nctx = B, H, W, nctx
        self._freeu = None
        self.set_freeu(freeu)
        self._tcond_key = self._tcond_keep = None      # (a fresh arena: the effective bias is recomputed by the next set_timestep_cond)
        self.tome_bind(None)

    # ------------------------------------------------------------------ token merging (DESIGN.md "Token merging")
    def tome_blocks(self):
        """{prefix: ToMeBlock} of the transformers whose self-attention runs on merged tokens in this plan (may be empty)."""
        return dict(getattr(self, "lay", {}).get("tome", {}).get("layout", {}))

    def tome_bind(self, row_ptr: Optional[int]):
        """Which device int32 names the window-table row the pp_tome_match launches use: a denoising loop's step counter, or
        None for the runtime's own word (always 0: `tome_fill(1, ...)` in front of a bare forward).  The pointer is a by-value
        argument: a graph captured before keeps the one it was captured with, so this runtime's own graph is dropped."""
        tm = getattr(self, "lay", {}).get("tome")
        if tm is None:
            return
        ptr = int(row_ptr) if row_ptr else tm["word"]
        if self._tome_row.value != ptr:
            self._tome_row.value = ptr
            self.graph = None

    def tome_fill(self, evaluations: int, state) -> int:
        """Draw the destination windows of `evaluations` network evaluations into the table: per evaluation one
        torch.randint(sy*sx, (hsy, wsx, 1)) per merging block in execution order, from `state`'s CPU generator -- tomesd's
        draws.  No draw (index 0 everywhere) with use_rand off or an odd logical batch (the batch of the forward, both CFG
        halves).  One host-to-device copy; stream-ordered, so replays of a captured graph queued behind it read the new rows."""
        tm = getattr(self, "lay", {}).get("tome")
        if tm is None:
            return 0
        if evaluations > tm["rows"]:
            raise L.PPError(f"token merging: {evaluations} network evaluations in one call, the window table holds {tm['rows']}")
        t = self.net.tome
        host = torch.zeros(evaluations, tm["stride"], dtype=torch.uint8)
        draws = 0
        if t.use_rand and self.B % 2 == 0:
            g = state.generator()
            for e in range(evaluations):
                for b in tm["layout"].values():
                    host[e, b.offset:b.offset + b.nd] = torch.randint(t.sy * t.sx, (b.h // t.sy, b.w // t.sx, 1),
                                                                    generator=g).reshape(-1).to(torch.uint8)
                    draws += 1
        self.arena.view(tm["table"], (evaluations, tm["stride"]), torch.uint8).copy_(host)
        self._tome_rows_filled = evaluations
        return draws

    def tome_table(self) -> torch.Tensor:
        """The filled rows of the window table, uint8 [evaluations][row bytes] (a copy)."""
        tm = self.lay["tome"]
        return self.arena.view(tm["table"], (getattr(self, "_tome_rows_filled", 1), tm["stride"]), torch.uint8).clone()

    def tome_decisions(self):
        """{prefix: (best_dst int32 [b, n], score fp32 [b, n], pos int32 [b, n])} of the LAST evaluation, copies; b is the
        batch the block ran on (one CFG half under the twin prefix)."""
        tm = self.lay["tome"]
        out = {}
        for pre, blk in tm["layout"].items():
            n, b = blk.h * blk.w, tm["batch"][pre]
            best, score, pos = tm["bufs"][pre]
            out[pre] = (self.arena.view(best, (b, n), torch.int32).clone(), self.arena.view(score, (b, n), torch.float32).clone(),
                        self.arena.view(pos, (b, n), torch.int32).clone())
        return out

    def set_freeu(self, values):
        """Write FreeU's (s1, s2, b1, b2) where the plan's pp_freeu launches read them, if they changed (stream-ordered:
        eager runs and replays of a captured graph queued after this call see the new values)."""
        if values is None or "freeu" not in self.lay:
            return
        values = tuple(float(v) for v in values)
        if values != self._freeu:
            s1, s2, b1, b2 = values
            self.arena.view(self.lay["freeu"], (4,), torch.float32).copy_(torch.tensor([b1, s1, b2, s2], dtype=torch.float32))
            self._freeu = values

    tcond_version = 0      # moves whenever the effective linear_1 bias changed: rows of a time-embedding table made before are stale

    def set_timestep_cond(self, c: Optional[torch.Tensor]):
        """`timestep_cond` of a guidance-embedded UNet (config.time_cond_proj_dim = d): c [1 or B, d], every row the same
        (the pipelines repeat one guidance scale over the batch).  diffusers' TimestepEmbedding computes
        linear_1(t_emb + cond_proj(c)) = W1 t_emb + (b1 + W1 (Wc c)); c is constant over a call, so the bracket is computed
        HERE, once per distinct c, by two pp_linear_skinny launches into a buffer at a stable address that the step plan's
        linear_1 launch reads as its bias.  None: the plain bias (diffusers skips cond_proj without a `timestep_cond`)."""
        net = self.net
        d = getattr(net, "time_cond_proj_dim", None)
        if not d:
            if c is not None:
                raise ValueError("timestep_cond needs a UNet with config.time_cond_proj_dim")
            return
        pver = getattr(net.params, "version", 0)
        if c is not None:
            if c.dim() != 2 or c.shape[1] != d:
                raise ValueError(f"timestep_cond must be [B or 1, {d}], got {tuple(c.shape)}")
            c = c.detach()[:1].to(torch.float32)
            # a host tensor is compared by value (the pipelines build a new one per call); a device tensor by identity
            ident = tuple(c.flatten().tolist()) if c.device.type == "cpu" else (c.data_ptr(), c._version)
        else:
            ident = None
        key = (ident, pver)
        if self._tcond_key is not None and key == self._tcond_key:
            return
        te = net.boc[0] * 4
        eff = self.arena.view(self.lay["b1_eff"], (te,), torch.float32)
        if c is None:
            eff.copy_(net.params.tensor("time_embedding.linear_1.bias"))
        else:
            self.arena.view(self.lay["tcond"], (d,), torch.float32).copy_(c.reshape(-1).to(self.device))
            P, dt, st = net.P, L.dtype_code(net.dtype), _stream()
            L.check(self.lib.pp_linear_skinny(self.lay["tcond"], 1, d, P["time_embedding.cond_proj.weight"], None, net.boc[0],
                                              self.lay["tcond_mid"], net.boc[0], 0, 0, dt, st), "pp_linear_skinny")
            L.check(self.lib.pp_linear_skinny(self.lay["tcond_mid"], 1, net.boc[0], P["time_embedding.linear_1.weight"],
                                              P["time_embedding.linear_1.bias"], te, self.lay["b1_eff"], te, 0, 0, dt, st),
                    "pp_linear_skinny")
        self._tcond_key, self._tcond_keep = key, c      # (an identity only holds while the tensor lives, as _ctx_keep)
        self.tcond_version = self.tcond_version + 1

    def _patch_scale(self, scale):
        """conditioning_scale is baked into the zero-conv GEMM launches; patch it in place (float or per-output list)."""
        zc = [args[0]._obj for fn, args, name in self.step_plan.calls if name == "zero_conv"]
        vals = list(scale) if isinstance(scale, (list, tuple)) else [scale] * len(zc)
        for a, v in zip(zc, vals):
            a.scale = float(v)
        if self.shallow_plan is not None:                  # (the shallow plan's zero convs: the live positions, the same values)
            for a, p in zip(self.zero_conv_records(self.shallow_plan), self.shallow_plan.zero_conv_pos):
                a.scale = float(vals[p])
            self.graph_shallow = None
        self._scale = tuple(float(v) for v in scale) if isinstance(scale, (list, tuple)) else scale
        self.graph = None

    # ------------------------------------------------------------------ several side networks, one sum
    def zero_conv_records(self, plan: Optional[Plan] = None):
        """The PPGemmArgs of the step plan's zero-conv launches, in output order (down..., mid[, up...]); of the shallow plan:
        the live positions only (`plan.zero_conv_pos` names them)."""
        return [args[0]._obj for fn, args, name in (plan or self.step_plan).calls if name == "zero_conv"]

    def residual_block(self) -> Tuple[int, int]:
        """(pointer, 64-bit words) of the contiguous arena block that holds every residual output of a side network
        (SDNet.build_step allocates them back to back; with pad_uncond the zeroed unconditional halves included)."""
        o = self.outputs
        acts = list(o["down"]) + [o["mid"]] + list(o.get("up", []))
        end = acts[-1].ptr + acts[-1].rows * acts[-1].C * 2
        return acts[0].ptr, (end - acts[0].ptr + 7) // 8

    def chained_step_calls(self, target: "NetRuntime", accumulate: bool, scale, skip=(), shallow: bool = False):
        """This side network's step launches (indices in `skip` left out) with the zero convs writing into `target`'s
        residual buffers instead of its own: `accumulate=False` overwrites them (the first network of a sum),
        `accumulate=True` adds to what they hold IN PLACE, `out = res1 = target buffer` -- the sum of several ControlNets
        rides the zero convs' epilogues, `v = (acc + bias) * scale + res1` (include/pp_hip.h, "res1 may alias out"), and
        costs no launch and no pass of its own.  `scale`: a float or one value per zero conv.
        The launch records are COPIES (the network's own plan, its scale and its outputs stay as they are); the caller keeps
        the returned records alive as long as the calls.  With pad_uncond the network's launch that zeroes the unconditional
        halves is pointed at the target's block when it overwrites and dropped when it accumulates.
        shallow (DeepCache): the shallow plans of both, whose zero convs are the live positions (`scale` stays one value per
        zero conv of the FULL plan).
        Returns (calls, records)."""
        plan = self.shallow_plan if shallow else self.step_plan
        mine, theirs = self.zero_conv_records(plan), target.zero_conv_records(target.shallow_plan if shallow else None)
        if len(mine) != len(theirs) or any((a.M, a.N, a.ldo) != (b.M, b.N, b.ldo) for a, b in zip(mine, theirs)):
            raise L.PPError("side networks whose residuals are summed must produce residuals of the same shapes")
        nfull = len(self.zero_conv_records())
        vals = [float(v) for v in scale] if isinstance(scale, (list, tuple)) else [float(scale)] * nfull
        if len(vals) != nfull:
            raise L.PPError(f"{len(vals)} residual scales for {nfull} zero convs")
        if shallow:
            vals = [vals[p] for p in plan.zero_conv_pos]
        pad_ptr = self.residual_block()[0] if self.pad_uncond else 0
        calls, records, k = [], [], 0
        for i, (fn, args, name) in enumerate(plan.calls):
            if i in skip:
                continue
            if name == "zero_conv":
                a, b = mine[k], theirs[k]
                if a.out_dup_rows or a.res1_wrap_rows or a.res1:
                    raise L.PPError("zero conv with a residual or a twin store cannot join a sum")
                r = type(a).from_buffer_copy(a)
                r.scale = vals[k]
                r.out = b.out
                r.res1, r.ldres1 = (b.out, b.ldo) if accumulate else (None, a.ldres1)
                records.append(r)
                calls.append((fn, (C.byref(r),), name))
                k += 1
            elif name == "zero_u64" and pad_ptr and args[0] == pad_ptr:
                if not accumulate:
                    calls.append((fn, target.residual_block(), name))
            else:
                calls.append((fn, args, name))
        return calls, records

    # ------------------------------------------------------------------ inputs
    def set_timestep(self, t):
        tv = self.arena.view(self.lay["t_dev"], (1,), torch.float32)
        if torch.is_tensor(t):
            tv.copy_(t.reshape(-1)[:1].to(torch.float32), non_blocking=True)
        else:
            tv.fill_(float(t))

    def set_context(self, ehs: torch.Tensor, force: bool = False):
        """encoder_hidden_states [B, nctx, ctx_dim]; recomputes the hoisted cross-attention K/V^T only on change."""
        ident = (ehs.data_ptr(), ehs._version, tuple(ehs.shape), getattr(self.net.params, "version", 0))
        if not force and ident == self._ctx_id:
            return
        dst = self.arena.view(self.lay["ehs"], (self.B, self.nctx, self.net.ctx_dim), self.net.dtype)
        dst.copy_(ehs.to(self.device))
        if self.net.kind != "controlnet" or self._cond_id is not None:
            self.setup_plan.run(_stream())
        self._ctx_id = ident
        self._ctx_keep = ehs      # the identity is only an identity while the tensor lives: a freed temporary's address
        #                           (and version 0) is handed to the next temporary by the caching allocator

    def set_cond(self, cond: torch.Tensor):
        """ControlNet conditioning image [B,3,8H,8W] (NCHW, any float dtype)."""
        ident = (cond.data_ptr(), cond._version, tuple(cond.shape))
        if ident == self._cond_id:
            return
        c = self.lay["cond"]
        # the whole batch, or one CFG half (copied to both halves, as load_input does); anything else would leave rows stale
        if cond.shape[0] == c.B:
            self.load_nchw(cond, c.ptr, c.C, 0, c.H * c.W)
        elif 2 * cond.shape[0] == c.B:
            self.load_nchw(cond, c.ptr, c.C, 0, c.H * c.W, batch=c.B, batch_mod=cond.shape[0])
        else:
            raise L.PPError(f"controlnet_cond has batch {cond.shape[0]}, the network runs batch {c.B}")
        self._cond_id = ident
        self._cond_keep = cond    # (same reason as _ctx_keep)
        if self._ctx_id is not None:
            self.setup_plan.run(_stream())

    def load_nchw(self, src: torch.Tensor, dst_ptr: int, ldc: int, c0: int, hw: int, batch: Optional[int] = None,
                  batch_mod: int = 0):
        src = src.to(self.device)
        if src.dtype not in _DT:
            src = src.float()
        src = src.contiguous()
        nb = batch if batch is not None else src.shape[0]
        L.check(self.lib.pp_nchw_to_nhwc(src.data_ptr(), _DT[src.dtype], nb, src.shape[1], hw, batch_mod, dst_ptr, ldc,
                                         c0, L.dtype_code(self.net.dtype), _stream()), "pp_nchw_to_nhwc")

    def load_input(self, parts: Sequence[Tuple[torch.Tensor, int]]):
        """parts: (NCHW tensor, channel offset); a tensor with half the batch is CFG-duplicated."""
        x = self.lay["x_in"]
        for t, c0 in parts:
            mod = t.shape[0] if t.shape[0] != x.B else 0
            self.load_nchw(t, x.ptr, x.C, c0, x.H * x.W, batch=x.B, batch_mod=mod)

    def load_residual(self, group: str, idx: int, t: torch.Tensor):
        s = self.lay["slots"][group][idx]
        if tuple(t.shape) != (s.B, s.C, s.H, s.W):
            raise L.PPError(f"residual {group}[{idx}] has shape {tuple(t.shape)}, expected {(s.B, s.C, s.H, s.W)}")
        self.load_nchw(t, s.ptr, s.C, 0, s.H * s.W)

    # ------------------------------------------------------------------ run
    def run_step(self, use_graph: bool = False):
        """One forward pass on its own (a model's `forward`): with token merging, fresh windows first -- a one-row table."""
        if "tome" in self.lay:
            self.tome_bind(None)
            self.tome_fill(1, self.net.tome_state)
        shallow = self.next_is_shallow()
        if use_graph:
            if self.graph is None:
                self.capture()                     # (the full plan first: its warm-up leaves a valid c for the shallow plan's)
            if shallow and self.__dict__.get("graph_shallow") is None:
                self.graph_shallow = self._capture(self.shallow_plan)
            (self.graph_shallow if shallow else self.graph).replay()
        else:
            (self.shallow_plan if shallow else self.step_plan).run(_stream())

    def next_is_shallow(self) -> bool:
        """DeepCache, a module called directly: count this evaluation; it is full iff its number is a multiple of
        cache_interval (the counter starts at 0 with every new plan and with DeepCacheSDHelper.enable())."""
        dc = getattr(self.net, "deepcache", None)
        if dc is None or self.shallow_plan is None:
            return False
        e, self.dc_eval = self.dc_eval, self.dc_eval + 1
        return e % int(dc.interval) != 0

    def capture(self):
        self.graph = self._capture(self.step_plan)
        self.graph_shallow = None

    def _capture(self, plan: Plan):
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            plan.run(s.cuda_stream)                # warm-up (sets func attributes outside capture)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            plan.run(_stream())
        return g

    def combines_in_kernel(self) -> bool:
        """Does the step plan (or DeepCache's shallow plan: one fault word serves both) hand tile counters to any split-K
        launch (PPGemmArgs.tile_ctr)?"""
        return any(getattr(a, "tile_ctr", None) for p in (self.step_plan, self.shallow_plan)
                   for a in getattr(p, "keep", []))

    def check_faults(self, blocking: bool = True):
        """The in-kernel split-K combine (csrc/gemm_combine.h) sums a tile's slabs through ONE XCD's L2.  Splits of a tile on
        different XCDs would count their arrivals in different L2s, never complete, give up, and leave their abandoned shares
        counted in the plan's fault word; so does a second-arrival wait that hit its bound.  A non-zero word means results since
        the last check may hold stale or missing partial sums: refuse.
        blocking=True synchronises and reads the word.  blocking=False costs the stream nothing: the word is copied to pinned
        host memory behind the work queued so far and examined by a LATER call (any check_faults) once that copy has landed --
        a pipeline call must not end in a device synchronisation (it would serialise the host's preparation of the next call
        behind this one's GPU work, +0.6 % at 50 steps), and a violation is a property of the box / plan, not of one call."""
        if self.arena is None or "fault" not in getattr(self, "lay", {}):
            return
        word = self.arena.view(self.lay["fault"], (1,), torch.int32)
        pend = self.__dict__.setdefault("_fault_pending", [])
        bad = 0
        if blocking:
            bad = int(word.item())
            pend.clear()
        else:
            while pend and pend[0][1].query():
                bad = max(bad, int(pend.pop(0)[0].item()))
            if len(pend) < 4:                                    # (bounded: the host may run many calls ahead)
                host = torch.empty(1, dtype=torch.int32, pin_memory=True)
                host.copy_(word, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                pend.append((host, ev))
        if bad:
            word.zero_()
            pend.clear()
            raise L.PPError(f"{bad} split-K shares were left uncombined or tiles combined across XCDs (workgroup placement "
                            f"changed under the plan): results are not trustworthy; rebuild the plan with PP_LAB=1 PP_FUSED_COMBINE=0")

    # ------------------------------------------------------------------ outputs
    def act_as_nchw(self, a: Act) -> torch.Tensor:
        """Zero-copy NCHW-logical (channels_last strides) bf16 torch view of an arena activation."""
        t = self.arena.view(a.ptr, (a.B, a.C, a.H, a.W), self.net.dtype,
                            strides=(a.H * a.W * a.C, 1, a.W * a.C, a.C))
        t._pp_nhwc_ptr = a.ptr
        return t

    def eps_tensor(self) -> torch.Tensor:
        return self.arena.view(self.outputs["eps"], (self.B, self.net.out_channels, self.H, self.W), torch.float32)
