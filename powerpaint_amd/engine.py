"""Host-side execution engine for the MI355X denoising hot path.

Design (MI355X-first):
  * parameters live in ONE contiguous device buffer per network (`ParamPack`) in kernel-ready layouts
    ([Cout][ky][kx][Cin] bf16 conv weights, fused QKV / KV matrices, GEGLU-interleaved FF weights, fp32 biases and
    norm affine) -> a single RCCL broadcast moves a whole network over xGMI;
  * activations are NHWC bf16 inside one static `Arena` (stack-scoped bump allocator: temporaries of a resnet /
    transformer block are released at block exit so consecutive blocks reuse the same, Infinity-Cache-hot addresses);
  * a forward pass is compiled ONCE per (shape, wiring) into a `Plan` -- a flat list of C-ABI launches with baked
    pointers -- which is replayed eagerly (ctypes, ~2 us / launch) or captured into a hipGraph;
  * everything that varies per denoising step is read from device memory by the kernels (timestep, scheduler
    coefficients, step counter), so a captured step replays with zero host->device traffic.
"""
import ctypes as C
import enum
import math
import os
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib as L

ALIGN = 256


def _align(x: int, a: int = ALIGN) -> int:
    return (x + a - 1) // a * a


# ------------------------------------------------------------------------------------------------------------------
def _lab_switch(name: str) -> bool:
    """A/B switches of the launch-plan compiler (measurement scripts, bisecting).  They are honoured only when PP_LAB=1
    is set as well: the product has one code path, and a stray PP_* variable in a user's environment changes nothing."""
    return not (os.environ.get("PP_LAB") == "1" and os.environ.get(name, "1") == "0")


# (lab) PP_GN_EPILOGUE=0: every GroupNorm keeps its own statistics launch
GN_STATS_IN_EPILOGUE = _lab_switch("PP_GN_EPILOGUE")
# A GroupNorm apply behind a split-K launch at the 16x16 / 8x8 levels rides in that launch's combine (PPGemmArgs.gn_next_*).
# (lab) PP_GN_NEXT=0: the separate apply launch
GN_NEXT_IN_COMBINE = _lab_switch("PP_GN_NEXT")
# ResnetBlock2D's norm -> SiLU -> conv3x3 as ONE launch (csrc/conv_gn.hip).  (lab) PP_FUSE_GN_CONV=0: apply launch + conv
FUSE_GN_CONV = _lab_switch("PP_FUSE_GN_CONV")
# round 5: the CFG-identical prefix of a forward pass (conv_in .. first self-attention) on ONE half of the batch where the
# caller vouches for identical halves (SDNet.build_step(twin=True)).  (lab) PP_TWIN=0: the whole batch everywhere
TWIN_PREFIX = _lab_switch("PP_TWIN")
# round 6: the split-K combine inside the producing kernel, every split combining its own share of the tile
# (csrc/gemm_combine.h, PPGemmArgs.tile_ctr).  (lab) PP_FUSED_COMBINE=0: the separate combine launches
FUSED_COMBINE = _lab_switch("PP_FUSED_COMBINE")
# Upsample2D's `nearest 2x -> conv3x3` as four 2x2 sub-pixel convs on folded weights, 4/9 of the MACs (PPGemmArgs.subpix,
# csrc/conv_gn.hip NMODE 4), where pp_upconv_subpix_supported() routes it.  (lab) PP_UPCONV_SUBPIX=0: the nine-tap launch
# over the upsampled image everywhere -- the plan of ABI v27, bit for bit
UPCONV_SUBPIX = _lab_switch("PP_UPCONV_SUBPIX")
# (lab) PP_UPCONV_SUBPIX=2: also where the library says "runs" but does not route (the 8 -> 16 upsampler, a weight stream
# that would read 16/9 of the weight bytes: the arm of its A/B)
UPCONV_SUBPIX_FROM = 1 if (os.environ.get("PP_LAB") == "1" and os.environ.get("PP_UPCONV_SUBPIX") == "2") else 2


def level_sizes(H: int, W: int, levels: int) -> List[Tuple[int, int]]:
    """(h, w) of the `levels` resolution levels of a UNet whose latent is H x W.  Downsample2D is a conv3x3 with stride 2 and
    padding 1, so a level is the CEIL half of the one above, h -> (h - 1) // 2 + 1 (13 -> 7 -> 4 -> 2), not h >> level; on the way
    up every upsampler resizes to the size of the level it returns to (unet_2d_condition.py:1120-1126,1311-1312 of the
    reference: `upsample_size`).  The one place the size chain is written down: SDNet.build_setup sizes the step-invariant
    operands with it, build_step reaches the same sizes through its convs, NetRuntime its residual slots."""
    out = [(H, W)]
    for _ in range(levels - 1):
        h, w = out[-1]
        out.append(((h - 1) // 2 + 1, (w - 1) // 2 + 1))
    return out


class Arena:
    """Stack-scoped bump allocator over one device buffer (or a dry counting arena when device is None)."""

    def __init__(self, nbytes: int = 0, device=None):
        self.dry = device is None
        self.size = nbytes
        if not self.dry:
            self.buf = torch.zeros(max(nbytes, ALIGN) + ALIGN, dtype=torch.uint8, device=device)
            skew = (-self.buf.data_ptr()) % ALIGN
            self.buf = self.buf[skew:skew + max(nbytes, ALIGN)]
            self.base = self.buf.data_ptr()
        else:
            self.buf = None
            self.base = 1 << 20  # fake non-null base for dry runs
        self.off = 0
        self.peak = 0

    def alloc(self, nbytes: int) -> int:
        off = _align(self.off)
        self.off = off + nbytes
        self.peak = max(self.peak, self.off)
        if not self.dry and self.off > self.size:
            raise L.PPError(f"arena overflow: need {self.off} > {self.size}")
        return self.base + off

    def mark(self) -> int:
        return self.off

    def release(self, m: int):
        self.off = m

    def view(self, ptr: int, shape: Sequence[int], dtype: torch.dtype, strides: Optional[Sequence[int]] = None):
        """torch view of arena memory (element strides)."""
        esize = torch.empty((), dtype=dtype).element_size()
        off = ptr - self.base
        assert off % esize == 0
        typed = self.buf.view(dtype)
        if strides is None:
            n = 1
            for s in shape:
                n *= s
            return typed[off // esize: off // esize + n].view(*shape)
        return torch.as_strided(typed, tuple(shape), tuple(strides), off // esize)


class ParamPack:
    """All parameters of one network in one contiguous device buffer (single-collective broadcast unit)."""

    def __init__(self):
        self.items: List[Tuple[str, torch.Tensor]] = []
        self.offsets: Dict[str, int] = {}
        self.shapes: Dict[str, Tuple[torch.Size, torch.dtype]] = {}
        self.total = 0
        self.buf = None
        self.ptr: Dict[str, int] = {}
        self.version = 0      # bumped whenever the VALUES in `buf` change in place (re-broadcast, param_buffer() writes):
        #                       caches derived from the weights (time-embedding table, folded cross-attention operands) key on it

    def touch(self):
        self.version += 1

    def add(self, name: str, t: torch.Tensor, dtype: torch.dtype):
        assert name not in self.offsets, name
        t = t.detach().to(dtype).contiguous()
        off = _align(self.total)
        self.offsets[name] = off
        self.shapes[name] = (t.shape, dtype)
        self.total = off + t.numel() * t.element_size()
        self.items.append((name, t))

    def to_device(self, device, materialize: bool = True):
        self.buf = torch.zeros(_align(self.total) + ALIGN, dtype=torch.uint8, device=device)
        skew = (-self.buf.data_ptr()) % ALIGN
        self.buf = self.buf[skew:skew + _align(self.total)]
        base = self.buf.data_ptr()
        for name, t in self.items:
            off = self.offsets[name]
            if materialize and t.device.type != "meta":
                nb = t.numel() * t.element_size()
                self.buf[off:off + nb].copy_(t.view(-1).view(torch.uint8))
            self.ptr[name] = base + off
        self.items = []  # drop host copies
        return self

    def regrow(self, keep: int):
        """Re-lay the tail of the buffer on the device: the first `keep` bytes (the network's own entries) are copied as they
        are into a NEW contiguous buffer and the entries `add()`ed since (behind a `forget`) are appended behind them.  Every
        pointer changes: whoever baked one into a plan rebuilds it."""
        old = self.buf
        self.total = max(self.total, keep)
        buf = torch.zeros(_align(self.total) + ALIGN, dtype=torch.uint8, device=old.device)
        skew = (-buf.data_ptr()) % ALIGN
        buf = buf[skew:skew + _align(self.total)]
        buf[:keep].copy_(old[:keep])
        for name, t in self.items:
            off, nb = self.offsets[name], t.numel() * t.element_size()
            buf[off:off + nb].copy_(t.view(-1).view(torch.uint8))
        self.items = []
        self.buf = buf
        base = buf.data_ptr()
        self.ptr.clear()              # (SDNet.P is this dict)
        self.ptr.update({name: base + off for name, off in self.offsets.items()})
        self.touch()

    def forget(self, prefix: str, keep: int):
        """Drop the entries named `prefix`... (all of which lie behind byte `keep`); the next add() lands at `keep`."""
        for name in [n for n in self.offsets if n.startswith(prefix)]:
            assert self.offsets[name] >= keep, name
            del self.offsets[name], self.shapes[name]
            self.ptr.pop(name, None)
        self.total = keep

    def tensor(self, name: str) -> torch.Tensor:
        shape, dtype = self.shapes[name]
        off = self.offsets[name]
        n = 1
        for s in shape:
            n *= s
        es = torch.empty((), dtype=dtype).element_size()
        return self.buf[off:off + n * es].view(dtype).view(shape)


@dataclass
class Act:
    """NHWC bf16 activation [B][H][W][C] living in an arena."""
    ptr: int
    B: int
    H: int
    W: int
    C: int
    producer: object = None   # PPGemmArgs of the launch that writes this tensor (GroupNorm statistics subscribe to it)
    dup_half: int = 0         # > 0: the producer computed batch items [0, dup_half) and stored every row twice (the CFG twin
    #                           prefix, PPGemmArgs.out_dup_rows); this Act is the full-batch view of that tensor
    gn_filled: object = None  # (acc, groups) shared by the (hidden, skip) pair a pp_freeu launch wrote: that launch has
    #                           already added the statistics of concat(hidden, skip) to `acc` (Builder.freeu)

    @property
    def rows(self) -> int:
        return self.B * self.H * self.W

    @property
    def nbytes(self) -> int:
        return self.rows * self.C * 2


class TapF32(NamedTuple):
    """A recorded tensor (Builder.taps) that is no NHWC Act of the 16-bit format: fp32, dense, `shape` as stored (the UNet's
    eps: NCHW; temb_all: one row)."""
    ptr: int
    shape: Tuple[int, ...]

    @property
    def nbytes(self) -> int:
        n = 4
        for d in self.shape:
            n *= d
        return n


class Plan:
    """Flat list of C-ABI launches with baked arguments."""

    def __init__(self):
        self.calls: List[Tuple] = []     # (fn, args_tuple, name)
        self.keep: List = []             # keep ctypes structs alive
        self.flops = 0.0                 # algorithmic FLOPs (2*MAC of conv/linear/attention matmuls)
        self.flops_by_kind: Dict[str, float] = {}  # FLOPs the launches EXECUTE, by launch name
        self.flops_skipped = 0.0         # part of `flops` no launch executes (sub-pixel upsampling convs: 5 of 9 taps)
        self.walk = None                 # SDNet.build_step: the modules the walk ran ({"down", "up", "cache"}: DeepCache's index table)
        self.zero_conv_pos = None        # shallow form of a side network: which _zero_conv_specs positions its zero convs are

    def add(self, name: str, fn, *args):
        self.calls.append((fn, args, name))

    def count(self, kind: str, flops: float):
        self.flops += flops
        self.flops_by_kind[kind] = self.flops_by_kind.get(kind, 0.0) + flops

    def skip(self, flops: float):
        """MACs of the algorithm that the plan's launches do not execute: in `flops`, not in `flops_by_kind` / `flops_executed`."""
        self.flops += flops
        self.flops_skipped += flops

    @property
    def flops_executed(self) -> float:
        return self.flops - self.flops_skipped

    def run(self, stream: int):
        for fn, args, name in self.calls:
            rc = fn(*args, stream)
            if rc != 0:
                L.check(rc, name)

    def run_timed(self, stream_obj) -> Dict[str, float]:
        """Eager replay with a HIP event pair around every launch (on the launch stream); ms per kernel name."""
        evs = []
        s = stream_obj.cuda_stream
        for fn, args, name in self.calls:
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record(stream_obj)
            rc = fn(*args, s)
            e1.record(stream_obj)
            if rc != 0:
                L.check(rc, name)
            evs.append((name, e0, e1))
        stream_obj.synchronize()
        out: Dict[str, float] = {}
        self.last_launch_ms = []
        for name, e0, e1 in evs:
            dt = e0.elapsed_time(e1)
            out[name] = out.get(name, 0.0) + dt
            self.last_launch_ms.append(dt)
        return out

    def describe(self, i: int) -> str:
        """Human-readable shape of launch i (GEMM-family launches carry a PPGemmArgs)."""
        fn, args, name = self.calls[i]
        a = getattr(args[0], "_obj", None) if args else None
        if isinstance(a, L.PPGemmArgs):
            return (f"{name} M={a.M} N={a.N} K={a.K} {'conv' if a.x_mode else 'lin'}"
                    f"{' s2' if a.stride == 2 else ''}{' up' if a.up else ''}{' cat' if a.c2 else ''}"
                    f" gm={L.lib().pp_gemm_tile_group_m(C.byref(a))}")
        return name


class Builder:
    """Appends launches to a Plan, allocating outputs / workspaces from an Arena."""

    def __init__(self, arena: Arena, plan: Optional[Plan] = None, dtype: torch.dtype = torch.bfloat16):
        self.arena = arena
        self.plan = plan or Plan()
        self.lib = L.lib()
        self.dtype = dtype                # 16-bit storage format of activations / matrix weights
        self.dt = L.dtype_code(dtype)     # ... as the C ABI's dtype code
        self.gemm_tile = 0       # tuning overrides (0 = auto)
        self.gemm_splitk = 0
        self.last_gemm = None    # PPGemmArgs of the most recent GEMM launch
        # GroupNorm statistics accumulated by the producers' epilogues: [gn_acc_base, +gn_acc_cap) bytes of persistent
        # arena memory for the int64 accumulators (0 = every GroupNorm keeps its own statistics launch)
        self.gn_acc_base = 0
        self.gn_acc_cap = 0
        self.gn_acc_used = 0
        # device word the in-kernel split-K combine counts placement violations in (NetRuntime.check_faults); 0 = none given
        self.fault_ptr = 0
        # (name, Act[, accumulator pointer]) of block outputs, in plan order, for the builds that record them (vae.py).
        # SDNet.build_step: (name, Act | TapF32) of a block output, which keeps its bytes to the end of the plan, and
        # (name, Act, call) of a tensor inside a block, whose memory is released behind the block: `call` is the entry of
        # plan.calls that completes it (the tuple itself: an index would move when a launch is put in front of the plan)
        self.taps: List[Tuple] = []

    # -- memory
    def alloc(self, nbytes: int) -> int:
        return self.arena.alloc(nbytes)

    def new_act(self, B, H, W, Cc) -> Act:
        return Act(self.alloc(B * H * W * Cc * 2), B, H, W, Cc)

    def tap_inner(self, name: str, act: "Act"):
        """Record a tensor inside a block: complete once the launch recorded last has run."""
        self.taps.append((name, act, self.plan.calls[-1]))

    def mark(self):
        return self.arena.mark()

    def release(self, m):
        self.arena.release(m)

    # -- ops
    def _gemm(self, a: L.PPGemmArgs, name: str):
        if a.tile == 0:
            a.tile = self.gemm_tile
        if a.splitk == 0:
            a.splitk = self.gemm_splitk
        a.dtype = self.dt
        ws = self.lib.pp_gemm_workspace_bytes(C.byref(a))
        if ws:
            a.workspace = self.alloc(ws)
            # tile counters of the in-kernel combine: persistent words of the pool the step's first launch zeroes (private to
            # this launch; every launch also leaves them zero).  A permission: pp_gemm_bf16 decides per launch.
            if FUSED_COMBINE and self.gn_acc_cap:
                nctr = _align(self.lib.pp_gemm_combine_ctr_bytes(C.byref(a)), 8)
                if nctr and self.gn_acc_used + nctr <= self.gn_acc_cap:
                    a.tile_ctr = self.gn_acc_base + self.gn_acc_used
                    a.combine_fault = self.fault_ptr or None
                    self.gn_acc_used += nctr
        self.plan.keep.append(a)
        self.last_gemm = a
        a._arena_top = self.arena.off       # everything this launch reads or scratches lies below (see _apply_in_producer_combine)
        self.plan.add(name, self.lib.pp_gemm_bf16, C.byref(a))
        if a.subpix:      # four parities of M rows on four taps each; the nine-tap algorithm has 9/4 of these MACs
            self.plan.count(name, 4 * 2.0 * a.M * a.N * a.K)
            self.plan.skip(5 * 2.0 * a.M * a.N * a.K)
        else:
            self.plan.count(name, 2.0 * a.M * a.N * a.K)

    def linear(self, x: int, rows: int, K: int, w: int, N: int, bias: int = 0, ldx: Optional[int] = None,
               x2: int = 0, K2: int = 0, ldx2: int = 0, res1: int = 0, ldres1: int = 0, res2: int = 0,
               ldres2: int = 0, scale: float = 1.0, act: int = 0, out: int = 0, ldo: Optional[int] = None,
               rowvec: int = 0, ld_rowvec: int = 0, rows_per_batch: int = 0, out_vt: int = 0, vt_col0: int = 0,
               vt_ld: int = 0, out_f32: bool = False, row_stats_out: int = 0, ln_stats: int = 0, ln_colsum: int = 0,
               ln_tiles: int = 0, ln_dim: int = 0, ln_eps: float = 1e-5, name: str = "gemm", res1_wrap: int = 0,
               w_batch_stride: int = 0, vec_batch_stride: int = 0) -> int:
        """out[rows][N] = epilogue(X[rows][K(+K2)] @ W[N][K+K2]^T).  Returns the output pointer.
        row_stats_out / ln_*: LayerNorm folded across two GEMMs (see include/pp_hip.h).  res1_wrap: res1 holds only that
        many rows (one half of a CFG pair), row m adds row m mod res1_wrap.  w_batch_stride / vec_batch_stride: one weight
        matrix (and bias / column-sum vector) per batch item of rows_per_batch rows."""
        n_out = N // 2 if act == L.PP_ACT_GEGLU else (vt_col0 if out_vt else N)
        if ldo is None:
            ldo = n_out
        if not out:
            out = self.alloc(rows * ldo * (4 if out_f32 else 2))
        m = self.mark()
        a = L.gemm_args(self.dt, rows, N, K, x, w, out, x2=x2, K2=K2, ldx=ldx, ldx2=ldx2, ldo=ldo, ldres1=ldres1, ldres2=ldres2,
                        rows_per_batch=rows_per_batch, scale=scale)
        a.bias, a.rowvec, a.ld_rowvec, a.res1, a.res2 = bias or None, rowvec or None, ld_rowvec, res1 or None, res2 or None
        a.w_batch_stride, a.vec_batch_stride, a.res1_wrap_rows = w_batch_stride, vec_batch_stride, res1_wrap
        a.act, a.out_f32 = act, int(out_f32)
        a.out_vt, a.vt_col0, a.vt_ld = out_vt or None, vt_col0, vt_ld
        a.row_stats_out = row_stats_out or None
        if ln_stats:
            a.ln_stats, a.ln_colsum, a.ln_tiles, a.ln_dim, a.ln_eps = ln_stats, ln_colsum, ln_tiles, ln_dim, ln_eps
        self._gemm(a, name)
        self.release(m)
        return out

    def conv3x3(self, x: Act, w: int, cout: int, bias: int = 0, stride: int = 1, up: bool = False,
                x2: Optional[Act] = None, rowvec: int = 0, res1: int = 0, res2: int = 0, scale: float = 1.0,
                out: Optional[Act] = None, x3: Optional[Act] = None, x4: Optional[Act] = None,
                name: str = "conv3x3", gn_in: Optional[Tuple[int, int, int, float, int]] = None, dup: bool = False,
                up_size: Optional[Tuple[int, int]] = None) -> Act:
        """up_size (with up): the nearest resize goes to that (h, w), 2 H or 2 H - 1 rows, 2 W or 2 W - 1 columns.
        gn_in = (gamma, beta, gamma_beta_interleaved, eps, groups): the conv input is SiLU(GroupNorm(concat(x, x2))).
        Where the statistics arrive from the producers' epilogues and the shape suits csrc/conv_gn.hip the norm runs in
        the conv's loader (ONE launch, the normalised activation is never written); else pp_groupnorm_apply(_acc) + conv.
        dup: x is ONE half of a CFG pair whose halves are identical; the launch stores every output row twice and the
        returned Act is the full batch (PPGemmArgs.out_dup_rows, Act.dup_half)."""
        if gn_in is not None:
            gamma, beta, gb, eps, groups = gn_in
            acc = self._subscribe_gn_stats(x, x2, groups) if FUSE_GN_CONV else 0
            fused = None
            if acc:
                fused = (acc, gb, groups, eps)
            else:
                x, x2 = self.groupnorm(x, gamma, beta, eps, True, x2=x2, groups=groups), None
        else:
            fused = None
        c2 = x2.C if x2 is not None else 0
        ptr = lambda t: t.ptr if t is not None else None      # noqa: E731
        # (x3, x4: the 1x1 tail over concat(x3, x4) at the output pixel -- the merged conv_shortcut)
        a = L.conv3x3_args(self.dt, x.B, x.H, x.W, x.C, cout, x.ptr, ptr(x2), c2, ptr(x3), x3.C if x3 is not None else 0,
                           ptr(x4), x4.C if x4 is not None else 0, stride, up, w=w, scale=scale, up_size=up_size)
        ho, wo = a.hout, a.wout
        if dup:
            assert out is None and gn_in is None
            out = self.new_act(2 * x.B, ho, wo, cout)
            out.dup_half = x.B
        if out is None:
            out = self.new_act(x.B, ho, wo, cout)
        m = self.mark()
        a.out, a.bias, a.rowvec, a.res1, a.res2 = out.ptr, bias or None, rowvec or None, res1 or None, res2 or None
        if dup:
            a.out_dup_rows = a.M
            if self.lib.pp_gemm_workspace_bytes(C.byref(a)):      # (split-K: the combine does not write twins)
                raise L.PPError("twin-prefix conv would run split-K; the caller must not request dup for this shape")
        if fused is not None:
            a.gn_in_acc, a.gn_in_gb, a.gn_in_groups, a.gn_in_eps, a.gn_in_silu = fused[0], fused[1], fused[2], fused[3], 1
            if not self.lib.pp_conv_gn_preferred(C.byref(a)):
                # (the statistics subscription stays: the apply launch reads the same accumulators)
                a.gn_in_acc, a.gn_in_gb, a.gn_in_groups, a.gn_in_silu = None, None, 0, 0
                gamma, beta, gb, eps, groups = gn_in
                self.release(m)
                xn = self._apply_in_producer_combine(x, fused[0], gamma, beta, eps, True, None) if x2 is None else None
                if xn is None:
                    xn = self.new_act(x.B, x.H, x.W, x.C + c2)
                    self.plan.add("groupnorm_apply", self.lib.pp_groupnorm_apply_acc, x.ptr, x.C,
                                  x2.ptr if x2 is not None else None, c2, x.B, x.H * x.W, groups, eps, gamma, beta, fused[0],
                                  1, xn.ptr, self.dt)
                m = self.mark()
                a.x1, a.x2, a.c1, a.c2 = xn.ptr, None, x.C + c2, 0
        self._gemm(a, name)
        out.producer = a
        self.release(m)
        return out

    def conv3x3_up_subpix(self, x: Act, wfold: int, cout: int, bias: int = 0, res2: int = 0, name: str = "conv3x3") -> Act:
        """Upsample2D's `nearest 2x -> conv3x3` in its sub-pixel form (PPGemmArgs.subpix): four 2x2 convs over the source x on
        the folded weights at `wfold` (pp_upconv_fold, SDNet.build_setup) -> [B][2H][2W][cout]; res2 has the output's shape.
        The caller has asked pp_upconv_subpix_supported()."""
        a = L.conv3x3_args(self.dt, x.B, x.H, x.W, x.C, cout, x.ptr, w=wfold)
        a.K, a.subpix = 4 * x.C, 1
        out = self.new_act(x.B, 2 * x.H, 2 * x.W, cout)
        a.out, a.bias, a.res2 = out.ptr, bias or None, res2 or None
        self._gemm(a, name)
        out.producer = a
        return out

    def groupnorm(self, x: Act, gamma: int, beta: int, eps: float, silu: bool, x2: Optional[Act] = None,
                  groups: int = 32, out: Optional[Act] = None) -> Act:
        c2 = x2.C if x2 is not None else 0
        Ct = x.C + c2
        hw = x.H * x.W
        out_given = out
        x2p = x2.ptr if x2 is not None else None
        acc = self._subscribe_gn_stats(x, x2, groups)
        if acc and x2 is None:
            fused = self._apply_in_producer_combine(x, acc, gamma, beta, eps, silu, out_given)
            if fused is not None:
                return fused
        if out is None:
            out = self.new_act(x.B, x.H, x.W, Ct)
        if acc:
            # the statistics arrive from the epilogues of the launches that produced x (and x2): no stats launch
            self.plan.add("groupnorm_apply", self.lib.pp_groupnorm_apply_acc, x.ptr, x.C, x2p, c2, x.B, hw, groups, eps,
                          gamma, beta, acc, int(silu), out.ptr, self.dt)
            return out
        m = self.mark()
        ws = self.alloc(self.lib.pp_groupnorm_workspace_bytes(x.B, hw, Ct))
        self.plan.add("groupnorm_stats", self.lib.pp_groupnorm_stats, x.ptr, x.C, x2p, c2, x.B, hw, groups, ws,
                      self.dt)
        self.plan.add("groupnorm_apply", self.lib.pp_groupnorm_apply, x.ptr, x.C, x2p, c2, x.B, hw, groups, eps,
                      gamma, beta, ws, int(silu), out.ptr, self.dt)
        self.release(m)
        return out

    def _apply_in_producer_combine(self, x: Act, acc: int, gamma: int, beta: int, eps: float, silu: bool,
                                   out: Optional[Act]) -> Optional[Act]:
        """The apply of a single-tensor GroupNorm whose input was written by the launch right in front of it in the plan: if
        that launch ends in the split-K combine that owns whole (batch item, group) populations (pp_gemm_gn_next_ok: the
        16x16 and 8x8 levels), the combine writes the normalised tensor as well and no apply launch is added.  `acc` = the
        statistics subscription of this norm (its accumulators are still filled)."""
        a = x.producer
        if not GN_NEXT_IN_COMBINE or a is None or not acc or not self.plan.calls or a.gn_next_out or \
                getattr(a, "_fused_ff", False):
            return None
        last = self.plan.calls[-1][1]
        if not last or getattr(last[0], "_obj", None) is not a:      # something ran in between: its scratch may alias
            return None
        sub = 0 if a.gn_acc[0] == acc else 1 if a.gn_acc[1] == acc else -1
        if sub < 0 or not self.lib.pp_gemm_gn_next_ok(C.byref(a), sub):
            return None
        if out is None:
            # the producer's combine writes this tensor while it still reads its split-K slabs and residuals -- scratch the
            # caller has RELEASED by now: allocate above everything that was live when the producer was recorded
            self.arena.off = max(self.arena.off, getattr(a, "_arena_top", self.arena.off))
            out = self.new_act(x.B, x.H, x.W, x.C)
        elif out.ptr < self.arena.base + getattr(a, "_arena_top", 0):
            return None                                     # (a caller-provided buffer that may alias that scratch)
        a.gn_next_out, a.gn_next_gamma, a.gn_next_beta = out.ptr, gamma, beta
        a.gn_next_eps, a.gn_next_silu, a.gn_next_sub = eps, int(silu), sub
        return out

    def _subscribe_gn_stats(self, x: Act, x2: Optional[Act], groups: int) -> int:
        """If every input tensor of this GroupNorm is written by a GEMM launch whose epilogue can accumulate the
        statistics, patch those launches (PPGemmArgs.gn_acc slot) and return the accumulator pointer, else 0."""
        if not (GN_STATS_IN_EPILOGUE and self.gn_acc_cap):
            return 0
        if x.gn_filled is not None or (x2 is not None and x2.gn_filled is not None):
            # written by a pp_freeu launch: it summed the pair it wrote, for the norm over exactly that pair (the producers'
            # epilogues saw the tensors before FreeU and must not be asked)
            f = x.gn_filled
            return f[0] if (f is not None and x2 is not None and x2.gn_filled is f and f[1] == groups) else 0
        hw = x.H * x.W
        parts = [(x, 0)] + ([(x2, x.C)] if x2 is not None else [])
        Ct = x.C + (x2.C if x2 is not None else 0)
        if hw % 64 or Ct % groups or Ct // groups < 8:     # (>= 8 channels per group: LDS group slots per 160-col tile)
            return 0
        for t, _ in parts:
            a = t.producer
            if a is None or (a.gn_acc[0] and a.gn_acc[1]):
                return 0
            rows = hw // 4 if a.subpix else hw      # (sub-pixel form: the request counts SOURCE pixels, a quarter of the tensor's)
            rpb = a.rows_per_batch
            a.rows_per_batch = rows
            ok = self.lib.pp_gemm_gn_stats_ok(C.byref(a))
            a.rows_per_batch = rpb
            if not ok or (rpb not in (0, rows)):
                return 0
        nbytes = x.B * groups * 2 * 8
        if self.gn_acc_used + nbytes > self.gn_acc_cap:
            return 0
        acc = self.gn_acc_base + self.gn_acc_used
        self.gn_acc_used += nbytes
        for t, c0 in parts:
            a = t.producer
            k = 0 if not a.gn_acc[0] else 1
            a.rows_per_batch = hw // 4 if a.subpix else hw
            a.gn_acc[k], a.gn_cg[k], a.gn_c0[k], a.gn_groups[k] = acc, Ct // groups, c0, groups
            if t.dup_half:       # this consumer sees the full (twice-stored) tensor: both halves' accumulators get the sums
                a.gn_dup_batch, a.gn_dup_mask = t.dup_half, a.gn_dup_mask | (1 << k)
        return acc

    def freeu(self, h: Act, sk: Act, bs: int, groups: int, h_out: Optional[Act] = None) -> Tuple[Act, Act]:
        """FreeU in front of an up-block resnet, ONE launch (csrc/freeu.hip): the first half of the hidden tensor's channels
        times b, the skip tensor through the four-bin Fourier filter with scale s; `bs` = device pointer to (b, s).  Both
        tensors are rewritten IN PLACE: inside a UNet step neither has another reader behind this point (the hidden tensor
        is the previous block's output, the skip tensor's down-path consumer ran long before), every replay recomputes them,
        and neither is an output or a residual slot.  The launch also adds the statistics of concat(hidden', skip') to a
        fresh accumulator, which the returned Acts carry for the resnet's norm1 (_subscribe_gn_stats).
        h_out: where the hidden tensor must SURVIVE the launch (DeepCache's cached tensor, which later evaluations read again),
        the scaled copy goes there instead."""
        assert (h.B, h.H, h.W) == (sk.B, sk.H, sk.W)
        ho = h_out.ptr if h_out is not None else h.ptr
        Ct, nbytes, acc = h.C + sk.C, h.B * groups * 2 * 8, 0
        if GN_STATS_IN_EPILOGUE and self.gn_acc_cap and Ct % groups == 0 and self.gn_acc_used + nbytes <= self.gn_acc_cap:
            acc = self.gn_acc_base + self.gn_acc_used
            self.gn_acc_used += nbytes
        self.plan.add("freeu", self.lib.pp_freeu, h.ptr, ho, h.C, sk.ptr, sk.ptr, sk.C, h.B, h.H, h.W, bs, acc or None,
                      groups, self.dt)
        filled = (acc, groups) if acc else None
        return (Act(ho, h.B, h.H, h.W, h.C, gn_filled=filled), Act(sk.ptr, sk.B, sk.H, sk.W, sk.C, gn_filled=filled))

    def layernorm(self, x: int, rows: int, Cc: int, gamma: int, beta: int, eps: float = 1e-5, out: int = 0) -> int:
        out = out or self.alloc(rows * Cc * 2)
        self.plan.add("layernorm", self.lib.pp_layernorm, x, rows, Cc, gamma, beta, eps, out, self.dt)
        return out

    def attention(self, q: int, ldq: int, k: int, ldk: int, vt: int, ldvt: int, B: int, heads: int, nq: int,
                  nk: int, d: int, out: int = 0, ldo: int = 0, log2q: bool = False) -> int:
        """log2q: q already holds Q * d^-0.5 * log2(e) (pp_tfront q_scale) -> the PP_ATTN_PIPE_LOG2 kernel."""
        Cc = heads * d
        if not out:
            out, ldo = self.alloc(B * nq * Cc * 2), Cc
        if log2q:
            self.plan.add("attention", self.lib.pp_attention_fwd_variant, q, ldq, k, ldk, vt, ldvt, out, ldo, B, heads, nq,
                          nk, d, float(d) ** -0.5, self.dt, L.PP_ATTN_PIPE_LOG2)
        else:
            self.plan.add("attention", self.lib.pp_attention_fwd, q, ldq, k, ldk, vt, ldvt, out, ldo, B, heads, nq, nk,
                          d, float(d) ** -0.5, self.dt)
        self.plan.count("attention", 4.0 * B * heads * nq * nk * d)
        return out

    def attention_tiled(self, q: int, ldq: int, k: int, ldk: int, vt: int, ldvt: int, B: int, heads: int, h: int, w: int,
                        nh: int, nw: int, d: int, out: int = 0, ldo: int = 0, log2q: bool = False) -> int:
        """Self-attention restricted to the nh x nw tiles of the h x w token grid (HyperTile: pp_attention_fwd_tiled, the tiled
        form of the pipelined kernel): the same operands as `attention` with nq = nk = h * w, one launch, and 1 / (nh nw) of its
        scores -- which is what the plan counts."""
        Cc, n = heads * d, h * w
        if not out:
            out, ldo = self.alloc(B * n * Cc * 2), Cc
        self.plan.add("attention", self.lib.pp_attention_fwd_tiled, q, ldq, k, ldk, vt, ldvt, out, ldo, B, heads, h, w, nh, nw,
                      d, float(d) ** -0.5, L.PP_ATTN_PIPE_LOG2 if log2q else L.PP_ATTN_AUTO, self.dt)
        self.plan.count("attention", 4.0 * B * heads * n * (n // (nh * nw)) * d)
        return out

    def ip_attn_add(self, q: int, ldq: int, k_ip: int, v_ip: int, o: int, ldo: int, B: int, heads: int, nq: int, nk: int,
                    d: int, scale, row_w: int = 0):
        """IP-Adapter's image-prompt term added in place to a cross-attention output (csrc/ip_attn.hip): `scale` is a
        ctypes.c_float CELL handed over by value at every launch -- whoever owns it (NetRuntime.set_ip_scales) changes the
        value of eager runs in place; a captured graph carries the value it was captured with.  row_w (ip_adapter_masks):
        device pointer to the fp32 [nq] weights of the adapter's mask at this level -- the record is then the masked entry,
        which READS them (NetRuntime.set_ip_masks rewrites them under a captured graph)."""
        if row_w:
            self.plan.add("ip_attn_add", self.lib.pp_ip_attn_add_masked, q, ldq, k_ip, v_ip, o, ldo, B, heads, nq, nk, d,
                          float(d) ** -0.5, scale, row_w, self.dt)
        else:
            self.plan.add("ip_attn_add", self.lib.pp_ip_attn_add, q, ldq, k_ip, v_ip, o, ldo, B, heads, nq, nk, d,
                          float(d) ** -0.5, scale, self.dt)
        self.plan.count("ip_attn_add", 4.0 * B * nq * nk * heads * d)

    def perceiver_attn(self, q: int, ldq: int, kv_x: int, ldkx: int, nx: int, kv_l: int, ldkl: int, nl: int, B: int, heads: int,
                       nq: int, out: int = 0) -> int:
        """The Resampler's attention (csrc/perceiver_attn.hip): nq queries per item over the nx + nl keys of the two [K | V]
        segments the to_kv GEMMs wrote; head dimension 64.  Returns o [B * nq][heads * 64]."""
        d = 64
        out = out or self.alloc(B * nq * heads * d * 2)
        self.plan.add("perceiver_attn", self.lib.pp_perceiver_attn, q, ldq, kv_x, ldkx, nx, kv_l or None, ldkl, nl, out,
                      heads * d, B, heads, nq, d, float(d) ** -0.5, self.dt)
        self.plan.count("perceiver_attn", 4.0 * B * heads * nq * (nx + nl) * d)
        return out

    def ff_fused(self, hs: int, rows: int, Cc: int, hw: int, w1: int, b1: int, cs1: int, ln_stats: int, ln_tiles: int,
                 w2: int, bias2: int, out: int, res1: int = 0, res1_wrap: int = 0, res2: int = 0, w2_kperm: bool = False):
        """FeedForward (GEGLU) + FF2 . proj_out of a C = 320 transformer as ONE launch (csrc/ff_fused.hip, pp_ff_fused): the
        [rows][4C] GEGLU tensor is never written.  The launch record is the PPGemmArgs of the SECOND GEMM (what the two-launch
        plan hands pp_gemm_bf16 for `[g | hs] [W_po W_ff2 | W_po]^T`), so GroupNorm-statistics subscriptions of the consumer
        patch it exactly as they patch a GEMM.  Returns that record."""
        # (x1 is never read: the tensor it would name does not exist)
        a = L.gemm_args(self.dt, rows, Cc, 4 * Cc, hs, w2, out, x2=hs, K2=Cc, rows_per_batch=hw)
        a.bias, a.res1, a.res2, a.res1_wrap_rows = bias2 or None, res1 or None, res2 or None, res1_wrap
        a.splitk = 1
        a._fused_ff = True                  # (no split-K combine behind this launch: _apply_in_producer_combine keeps off)
        self.plan.keep.append(a)
        self.last_gemm = a
        a._arena_top = self.arena.off
        self.plan.add("ff_fused", self.lib.pp_ff_fused, C.byref(a), w1, b1, cs1 or None, ln_stats or None, ln_tiles, 1e-5,
                      int(w2_kperm))
        self.plan.count("ff_fused", 2.0 * rows * 8 * Cc * Cc + 2.0 * rows * Cc * 5 * Cc)   # (FF1 + [g | hs] W2'^T)
        return a

    def add(self, a: int, b: int, out: int, n: int):
        self.plan.add("add", self.lib.pp_add_bf16, a, b, out, n, self.dt)


# ------------------------------------------------------------------------------------------------------------------
# parameter preparation (diffusers state-dict keys -> kernel layouts)
# ------------------------------------------------------------------------------------------------------------------
def _conv_igemm(w: torch.Tensor) -> torch.Tensor:
    """[Cout,Cin,3,3] -> [Cout, 9*Cin] with k = (ky*3+kx)*Cin + ci."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def _conv_direct(w: torch.Tensor) -> torch.Tensor:
    """[Cout,Cin,3,3] -> [3,3,Cin,Cout]."""
    return w.permute(2, 3, 1, 0)


CIN_CHUNK = 64   # K chunk of the implicit-GEMM conv: one (tap, 64 channels) slice per main-loop step


def _conv_igemm_cpad(w: torch.Tensor, cpad: int) -> torch.Tensor:
    """conv_in ([Cout, 4|9, 3, 3]) for the implicit-GEMM kernel: input channels zero-padded to `cpad` (one 64-deep K
    chunk per tap; the network input buffer carries the same zero channels), then the igemm layout."""
    pad = cpad - w.shape[1]
    if pad:
        w = torch.cat([w, torch.zeros(w.shape[0], pad, 3, 3, dtype=w.dtype, device=w.device)], 1)
    return _conv_igemm(w)


def _kperm(w: torch.Tensor) -> torch.Tensor:
    """[N][K] -> the input index permuted inside every group of 32: storage position 8 kg + j holds index
    16 (j >> 2) + 4 kg + (j & 3).  A lane's 16-byte A fragment (k-group kg) of a GEMM whose B operand comes straight out of
    the previous GEMM's MFMA accumulators (four consecutive columns per register quad) then lines up with it: the layout
    csrc/tfront.hip and csrc/xattn_fused.hip chain two GEMMs with."""
    K = w.shape[-1]
    assert K % 32 == 0
    kp = torch.arange(K)
    s32, kg, j = kp // 32, (kp // 8) % 4, kp % 8
    kk = 32 * s32 + 16 * (j // 4) + 4 * kg + (j % 4)
    return w[..., kk]


def _kperm_geglu(w: torch.Tensor) -> torch.Tensor:
    """[N][K] -> the input (hidden-unit) index permuted inside every group of 32: storage position 8 kg + 2 q + e holds unit
    8 q + 2 kg + e.  The GEGLU of an MFMA accumulator quad (h0, h1, g0, g1) is two hidden units (2 kg, 2 kg + 1 of the
    16-column block q), so a lane's four quads of a 64-column chunk ARE its 16-byte B fragment of a GEMM whose A operand is
    packed like this: how csrc/ff_fused.hip chains FF1 -> GEGLU -> FF2 in registers."""
    K = w.shape[-1]
    assert K % 32 == 0
    sp = torch.arange(K)
    s32, r = sp // 32, sp % 32
    kg, q, e = r // 8, (r // 2) % 4, r % 2
    return w[..., 32 * s32 + 8 * q + 2 * kg + e]


def _geglu_interleave(w: torch.Tensor) -> torch.Tensor:
    """GEGLU proj rows [h(0..F) ; g(0..F)] -> groups of four rows (h_{2q}, h_{2q+1}, g_{2q}, g_{2q+1})."""
    F2 = w.shape[0]
    F = F2 // 2
    h, g = w[:F], w[F:]
    rest = w.shape[1:]
    h = h.reshape(F // 2, 2, *rest)
    g = g.reshape(F // 2, 2, *rest)
    return torch.cat([h, g], dim=1).reshape(F2, *rest)


@dataclass
class PackRecipe:
    """How ONE 16-bit packed entry (and the fp32 side vectors that belong to it) is made of diffusers tensors."""
    name: str                       # packed entry
    rows: List[str]                 # source modules ("<module>.weight" [N][K] | [Cout][Cin][k][k]) concatenated along rows
    cols: str = "plain"             # column order: plain | igemm (_conv_igemm) | kperm | kperm_geglu | direct (_conv_direct)
    cin_pad: int = 0                # igemm: input channels zero-padded to this many (conv_in)
    tail: Optional[str] = None      # module whose [N][Kt] weight follows as a K tail (conv_shortcut merged into conv2)
    compose: Optional[str] = None   # module W2: the entry is [W_rows @ W2 | W_rows] (`cols` orders the product's columns)
    row_order: str = "plain"        # plain | geglu (_geglu_interleave)
    gamma: Optional[str] = None     # LayerNorm module folded in: per-column factor norm.weight (beta = norm.bias)
    colsum: Optional[str] = None    # fp32 entry: row sums of the ROUNDED weights
    bias: Optional[str] = None      # fp32 entry: W beta (+ badd)   | composed: W_rows b2 + badd
    badd: Optional[str] = None      # diffusers key of the additive bias

    def sources(self) -> List[str]:
        return list(self.rows) + ([self.tail] if self.tail else []) + ([self.compose] if self.compose else [])


@dataclass
class PackVec:
    """One fp32 packed vector: copy | sum of two | cat | gb ((gamma, beta) interleaved) | geglu (interleaved) of state-dict keys."""
    name: str
    op: str
    keys: Tuple[str, ...]


class ToMe(NamedTuple):
    """Token merging in front of the self-attentions (powerpaint_amd/tome.py, DESIGN.md "Token merging"): tomesd's arguments.
    Part of a plan's key; the window draws are data."""
    ratio: float
    max_downsample: int
    sx: int
    sy: int
    use_rand: bool


class ToMeBlock(NamedTuple):
    """One transformer whose self-attention runs on merged tokens: its grid, the destinations nd, the merged sources r and
    the offset of its windows inside a row of the window table."""
    h: int
    w: int
    nd: int
    r: int
    offset: int


TOME_TABLE_ROWS = 1000       # network evaluations of one pipeline call the window table holds


class HyperTile(NamedTuple):
    """Tiled self-attention at the top level (powerpaint_amd/hypertile.py, DESIGN.md "HyperTile"): the target tile size in
    pixels.  Part of a plan's key."""
    tile_size: int


def hypertile_split(v: int, tile_size: int) -> int:
    """Tiles along a latent side of v pixels: v // side, side = the smallest divisor of v that is >= min(T, v) with
    T = max(32, tile_size) // 8 latent pixels (HyperTile's rule at swap_size = 1)."""
    T = min(max(32, int(tile_size)) // 8, v)
    side = next(s for s in range(T, v + 1) if v % s == 0)
    return v // side


class DeepCache(NamedTuple):
    """DeepCache (powerpaint_amd/deepcache.py): `branch` = cache_branch_id, part of the plan key; `interval` = cache_interval, host
    schedule only (which of the two plans an evaluation runs) and no part of any key."""
    branch: int
    interval: int = 3


class PAG(NamedTuple):
    """Perturbed-attention guidance on a UNet (powerpaint_amd/pag.py, DESIGN.md "Perturbed-attention guidance"): the
    transformers whose self-attention is the identity for the LAST `n` batch items.  Part of a plan's key; the scales are not
    the network's business (the loop's pp_pag_combine reads them)."""
    layers: Tuple[str, ...]
    n: int


class XAttnForm(enum.Enum):
    """How the cross-attention sub-block of a transformer (norm2 -> to_q -> attention over the prompt -> to_out + residual)
    runs.  SDNet.xattn_form decides; the value is the `kperm` pp_xattn_fold lays the folded operands out with."""
    CHAIN = None        # to_q -> attention -> to_out, three launches, nothing folded
    BLOCK = 0           # one pp_xattn_block launch
    BLOCK_PRE = 1       # ... with attn1.to_out (+ residual) in front, in the same launch
    TWO_GEMM = 2        # two GEMMs with per-prompt weights (PP_ACT_SOFTMAX80 in the first one's epilogue)


class XAttnFold(NamedTuple):
    """Folded cross-attention operands of one transformer (written by pp_xattn_fold in the setup plan) and the step
    geometry their form was resolved for."""
    gt: int
    gcs: int
    gb: int
    ht: int
    kperm: int
    rows: int           # of the full batch
    hw: int             # positions per batch item

    @property
    def form(self) -> XAttnForm:
        return XAttnForm(self.kperm)


class _TransformerBlock:
    """One transformer being compiled (SDNet._transformer): what its three stages share.  rows: of the input x (ONE half of
    a CFG pair under `twin`); rows_o: of the full batch, which everything behind the first cross-attention runs on."""

    def __init__(self, net: "SDNet", pb: "Builder", pre: str, x: Act, twin: bool):
        self.net, self.pb, self.pre, self.x, self.twin = net, pb, pre, x, twin
        self.tb = f"{pre}.transformer_blocks.0"
        self.rows, self.hw = x.rows, x.H * x.W
        self.rows_o = 2 * x.rows if twin else x.rows
        self.tiles = (x.C + 159) // 160

    def tap(self, what: str, ptr: int, rows: int):
        """Record one of the tensors the chosen form stores (Builder.taps); the launch recorded last completes it."""
        x = self.x
        self.pb.tap_inner(f"{self.pre}.{what}", Act(ptr, rows // self.hw, x.H, x.W, x.C))

    def attend_tapped(self, hs: int, *args, **kw) -> int:
        a = self.attend(hs, *args, **kw)
        self.tap("attn1", a, self.rows)
        return a

    def producer(self, rows: int) -> int:
        """Row-moment buffer written by the GEMM that produces the next LayerNorm's input."""
        return self.pb.alloc(rows * self.tiles * 8) if self.net.fold_ln else 0

    def normed(self, h: int, st: int, nrm: str, lin: str, rows: int):
        """-> (x pointer, kwargs) for the Linear `lin` applied to LayerNorm_nrm(h)."""
        P, tb, Cc = self.net.P, self.tb, self.x.C
        if self.net.fold_ln:
            return h, dict(bias=P[f"{tb}.{lin}.bias"], ln_stats=st, ln_colsum=P[f"{tb}.{lin}.colsum"],
                           ln_tiles=self.tiles, ln_dim=Cc, ln_eps=1e-5)
        xn = self.pb.layernorm(h, rows, Cc, P[f"{tb}.{nrm}.weight"], P[f"{tb}.{nrm}.bias"])
        return xn, (dict(bias=P[f"{tb}.{lin}.bias"]) if lin == "ff1" else {})

    def self_attention(self) -> Tuple[int, int]:
        """norm -> proj_in -> norm1 -> QKV -> attention.  -> (hs, a): the hidden state behind proj_in and attn1's output in
        front of its to_out, which belongs to whichever launch the cross-attention form gives it to."""
        net, pb, P, x, pre, tb = self.net, self.pb, self.net.P, self.x, self.pre, self.tb
        Cc, rows, hw, d = x.C, self.rows, self.hw, x.C // net.heads
        if net.fold_ln and net.fuse_tfront and f"{tb}.attn1.qkv.weight_kp" in P and \
                pb.lib.pp_tfront_supported(rows, Cc, hw, net.groups):
            acc = pb._subscribe_gn_stats(x, None, net.groups)
            if acc:
                hs = pb.alloc(rows * Cc * 2)
                vt = pb.alloc(x.B * Cc * hw * 2)
                qk = pb.alloc(rows * 2 * Cc * 2)
                # (round 5) Q leaves the front end as Q * d^-0.5 * log2(e) where the pipelined attention kernel covers the
                # shape: its scores then come out of the MFMA as exp2 arguments (PP_ATTN_PIPE_LOG2)
                n_att = hw - self.tome_r()                       # (token merging: attention runs on the merged rows)
                log2q = bool(net.attn_log2 and pb.lib.pp_attention_log2_ok(n_att, n_att, d))
                pb.plan.add("tfront", pb.lib.pp_tfront, x.ptr, Cc, acc, P[f"{pre}.norm.weight"], P[f"{pre}.norm.bias"], 1e-6,
                            net.groups, P[f"{pre}.proj_in.weight"], P[f"{pre}.proj_in.bias"],
                            P[f"{tb}.attn1.qkv.weight_kp"], P[f"{tb}.attn1.qkv.colsum"], P[f"{tb}.attn1.qkv.bias"], 1e-5, hs, Cc,
                            qk, 2 * Cc, vt, hw, rows, Cc, hw, (float(d) ** -0.5) * 1.4426950408889634 if log2q else 1.0, pb.dt)
                pb.plan.count("tfront", 2.0 * rows * Cc * Cc + 2.0 * rows * 3 * Cc * Cc)     # (proj_in + QKV)
                self.tap("proj_in", hs, rows)
                return hs, self.attend_tapped(hs, qk, 2 * Cc, vt, hw, log2q=log2q)
        st = self.producer(rows)
        n = pb.groupnorm(x, P[f"{pre}.norm.weight"], P[f"{pre}.norm.bias"], 1e-6, False, groups=net.groups)
        hs = pb.linear(n.ptr, rows, Cc, P[f"{pre}.proj_in.weight"], Cc, P[f"{pre}.proj_in.bias"], row_stats_out=st,
                       name="conv1x1")
        self.tap("proj_in", hs, rows)
        ln, kw = self.normed(hs, st, "norm1", "attn1.qkv", rows)
        if hw % 8 == 0:       # fused QKV GEMM, V written transposed by the epilogue
            vt = pb.alloc(x.B * Cc * hw * 2)
            qk = pb.linear(ln, rows, Cc, P[f"{tb}.attn1.qkv.weight"], 3 * Cc, out_vt=vt, vt_col0=2 * Cc, vt_ld=hw,
                           rows_per_batch=hw, name="linear", **kw)
            return hs, self.attend_tapped(hs, qk, 2 * Cc, vt, hw)
        # tiny latents (hw < 8, e.g. 2x2): V^T rows must be 16-byte aligned and zero padded -> unfused transpose
        ldvt = _align(hw, 8)
        vt = pb.alloc(x.B * Cc * ldvt * 2)
        qkv = pb.linear(ln, rows, Cc, P[f"{tb}.attn1.qkv.weight"], 3 * Cc, name="linear", **kw)
        pb.plan.add("transpose_v", pb.lib.pp_transpose_v, qkv + 4 * Cc, 3 * Cc, x.B, hw, Cc, vt, ldvt)
        return hs, self.attend_tapped(hs, qkv, 3 * Cc, vt, ldvt)

    def tome_r(self) -> int:
        """Sources this block merges in front of its self-attention (0: none -- SDNet.tome_layout decides)."""
        tm = self.net._tome_step
        return tm["layout"][self.pre].r if tm and self.pre in tm["layout"] else 0

    def attend(self, hs: int, qk: int, ldqk: int, vt: int, ldvt: int, log2q: bool = False) -> int:
        """attn1 over Q | K rows (row stride ldqk elements, K behind Q) and V^T.  With token merging on this block: match on
        hs, select, merge Q | K and V^T, attention on n - r rows, unmerge -- merging is a mean and the projections are affine,
        so the merged rows of Q, K, V are the projections of the merged tokens, and what reads the output stays as it is."""
        net, pb, x = self.net, self.pb, self.x
        Cc, hw, B, d = x.C, self.hw, x.B, x.C // net.heads
        r = self.tome_r()
        pg = net._pag_step
        ht = (net._ht_step or {}).get(self.pre)
        if ht is not None and ht[2]:
            # HyperTile: the same operands, the tiled entry; under PAG on the leading batch items, as the untiled launch is
            if r:
                raise L.PPError(f"{self.pre}: HyperTile together with token merging (ToMe) is not implemented")
            perturbed = pg.n if pg is not None and self.pre in pg.layers else 0
            a = pb.attention_tiled(qk, ldqk, qk + 2 * Cc, ldqk, vt, ldvt, B - perturbed, net.heads, x.H, x.W, ht[0], ht[1], d,
                                   out=pb.alloc(B * hw * Cc * 2), ldo=Cc, log2q=log2q)
            if perturbed:
                pb.plan.add("attn_identity_v", pb.lib.pp_attn_identity_v, vt, ldvt, B - perturbed, perturbed, hw, Cc, a, Cc)
            return a
        if pg is not None and self.pre in pg.layers:
            # perturbed-attention guidance: softmax attention on the leading batch items (same pointers, smaller batch); for the
            # trailing pg.n items attn1's output is V itself, copied out of V^T into the same buffer
            if r:
                raise L.PPError(f"{self.pre}: token merging (ToMe) together with perturbed-attention guidance (PAG) is not implemented")
            a = pb.alloc(B * hw * Cc * 2)
            pb.attention(qk, ldqk, qk + 2 * Cc, ldqk, vt, ldvt, B - pg.n, net.heads, hw, hw, d, out=a, ldo=Cc, log2q=log2q)
            pb.plan.add("attn_identity_v", pb.lib.pp_attn_identity_v, vt, ldvt, B - pg.n, pg.n, hw, Cc, a, Cc)
            return a
        if not r:
            return pb.attention(qk, ldqk, qk + 2 * Cc, ldqk, vt, ldvt, B, net.heads, hw, hw, d, log2q=log2q)
        tm, lib = net._tome_step, pb.lib
        blk, t = tm["layout"][self.pre], net.tome
        nm, ldvt2 = hw - r, _align(hw - r, 8)
        best, score, pos = tm["bufs"][self.pre]
        tm.setdefault("batch", {})[self.pre] = B          # (NetRuntime.tome_decisions: one CFG half under the twin prefix)
        rowtok, seg, lst = pb.alloc(B * nm * 4), pb.alloc(B * (blk.nd + 1) * 4), pb.alloc(B * r * 4)
        qk2, vt2 = pb.alloc(B * nm * 2 * Cc * 2), pb.alloc(B * Cc * ldvt2 * 2)
        a2, a = pb.alloc(B * nm * Cc * 2), pb.alloc(B * hw * Cc * 2)
        pb.plan.add("tome_match", lib.pp_tome_match, hs, Cc, B, x.H, x.W, Cc, t.sx, t.sy, tm["table"] + blk.offset, tm["stride"],
                    tm["rows"], tm["row"], best, score, pb.dt)
        pb.plan.count("tome_match", 2.0 * B * hw * blk.nd * Cc)
        pb.plan.add("tome_select", lib.pp_tome_select, best, score, B, hw, blk.nd, r, pos, rowtok, seg, lst)
        pb.plan.add("tome_merge", lib.pp_tome_merge, qk, ldqk, vt, ldvt, B, hw, Cc, blk.nd, r, rowtok, seg, lst, qk2, 2 * Cc, vt2,
                    ldvt2, pb.dt)
        pb.attention(qk2, 2 * Cc, qk2 + 2 * Cc, 2 * Cc, vt2, ldvt2, B, net.heads, nm, nm, d, out=a2, ldo=Cc, log2q=log2q)
        pb.plan.add("tome_unmerge", lib.pp_tome_unmerge, a2, Cc, pos, B, hw, nm, Cc, a, Cc)
        return a

    def cross_attention(self, hs: int, a: int, xa: Optional[XAttnFold], kv: Tuple[int, int, int, int]) -> Tuple[int, int]:
        """attn1.to_out + residual, then the cross-attention sub-block in the form build_setup resolved (xa: its folded
        operands, None for the chain; kv: the hoisted K / V^T the chain reads).  -> (hs, st) on rows_o rows."""
        net, pb, P, x, tb = self.net, self.pb, self.net.P, self.x, self.tb
        Cc, rows, rows_o, hw, tiles, fold = x.C, self.rows, self.rows_o, self.hw, self.tiles, self.net.fold_ln
        form = xa.form if xa is not None else XAttnForm.CHAIN
        if xa is not None and (xa.rows, xa.hw) != (rows_o, hw):
            raise L.PPError(f"{self.pre}: the cross-attention operands were folded for {xa.rows} rows of {xa.hw} positions "
                            f"per batch item, the step reaches it with {rows_o} of {hw} (build_setup's hw0)")
        if self.twin and form not in (XAttnForm.BLOCK, XAttnForm.BLOCK_PRE):
            raise L.PPError("twin prefix without the fused cross-attention block (build_step checks twin_prefix_ok first)")
        wrap = rows if self.twin else 0
        if form is XAttnForm.BLOCK_PRE:
            # attn1.to_out + residual in front of the cross-attention sub-block, same launch (G^T was folded with kperm = 1)
            st = self.producer(rows_o)
            o = pb.alloc(rows_o * Cc * 2)
            pb.plan.add("xattn_block", pb.lib.pp_xattn_block, a, Cc, hs, Cc, None, tiles, 1e-5, xa.gt, xa.gcs, xa.gb, xa.ht,
                        P[f"{tb}.attn2.to_out.bias"], o, Cc, st or None, rows_o, Cc, hw, wrap,
                        P[f"{tb}.attn1.to_out.weight"], P[f"{tb}.attn1.to_out.bias"], pb.dt)
            pb.plan.count("xattn_block", 6.0 * rows_o * Cc * Cc + 4.0 * rows_o * net._nctx * Cc)   # (+ attn1.to_out)
            self.tap("attn2", o, rows_o)
            return o, st
        st = self.producer(rows)
        hs = pb.linear(a, rows, Cc, P[f"{tb}.attn1.to_out.weight"], Cc, P[f"{tb}.attn1.to_out.bias"], res1=hs,
                       row_stats_out=st, name="linear")
        self.tap("attn1_out", hs, rows)
        ln, kw = self.normed(hs, st, "norm2", "attn2.to_q", rows)
        if form is XAttnForm.TWO_GEMM:
            # the folded sub-block as two GEMMs with one (G^T, H^T) per batch item (setup plan: pp_xattn_fold(kperm = 2))
            S = net.heads * 80
            stats = dict(ln_stats=kw["ln_stats"], ln_colsum=xa.gcs, ln_tiles=tiles, ln_dim=Cc, ln_eps=1e-5) if fold else {}
            prob = pb.linear(ln, rows, Cc, xa.gt, S, bias=xa.gb, act=L.PP_ACT_SOFTMAX80, rows_per_batch=hw,
                             w_batch_stride=S * Cc, vec_batch_stride=S, name="linear", **stats)
            st = self.producer(rows)
            hs = pb.linear(prob, rows, S, xa.ht, Cc, P[f"{tb}.attn2.to_out.bias"], res1=hs, row_stats_out=st,
                           rows_per_batch=hw, w_batch_stride=Cc * S, name="linear")
        elif form is XAttnForm.BLOCK:
            st = self.producer(rows_o)
            o = pb.alloc(rows_o * Cc * 2)
            pb.plan.add("xattn_block", pb.lib.pp_xattn_block, ln, Cc, hs, Cc, kw.get("ln_stats"), tiles if fold else 0,
                        1e-5, xa.gt, xa.gcs, xa.gb, xa.ht, P[f"{tb}.attn2.to_out.bias"], o, Cc, st or None, rows_o, Cc, hw,
                        wrap, None, None, pb.dt)
            # (the FLOPs of the chain it stands for: the folded form multiplies twice as much)
            pb.plan.count("xattn_block", 4.0 * rows_o * Cc * Cc + 4.0 * rows_o * net._nctx * Cc)
            hs = o
        else:
            # K / V^T hoisted out of the step: encoder_hidden_states are step-invariant
            q = pb.linear(ln, rows, Cc, P[f"{tb}.attn2.to_q.weight"], Cc, name="linear", **kw)
            a = pb.attention(q, Cc, kv[0], kv[1], kv[2], kv[3], x.B, net.heads, hw, net._nctx, Cc // net.heads)
            # IP-Adapter: a += scale_i * softmax(q K_i^T / sqrt(d)) V_i per adapter, in place, in front of to_out
            # (with ip_adapter_masks: times the adapter's per-row weights of this level, build_setup's ip_row_w)
            row_w = net.ip_row_w[hw] if net.ip_row_w else [0] * len(net.ip_scale_cells)
            for (k_ip, v_ip, nk_ip), cell, w in zip(net.ip_kv.get(self.pre, ()), net.ip_scale_cells, row_w):
                pb.ip_attn_add(q, Cc, k_ip, v_ip, a, Cc, x.B, net.heads, hw, nk_ip, Cc // net.heads, cell, w)
            st = self.producer(rows)
            hs = pb.linear(a, rows, Cc, P[f"{tb}.attn2.to_out.weight"], Cc, P[f"{tb}.attn2.to_out.bias"], res1=hs,
                           row_stats_out=st, name="linear")
        self.tap("attn2", hs, rows_o)
        return hs, st

    def feed_forward(self, hs: int, st: int, out: int, res2: int):
        """norm3 -> GEGLU -> FF2 -> proj_out + the transformer's residual (+ res2), into `out`.  -> the launch that wrote it."""
        net, pb, P, x, pre, tb = self.net, self.pb, self.net.P, self.x, self.pre, self.tb
        Cc, rows = x.C, self.rows_o
        wrap = self.rows if self.twin else 0          # the transformer's input (the proj_out residual) holds one half only
        w2n = f"{pre}.ff2_proj_out.weight" + ("" if net.ff_w8 else "_kp")
        if net.fold_ln and net.fuse_ff and net.merge_ff2_proj_out and w2n in P and \
                pb.lib.pp_ff_fused_supported(rows, Cc, self.hw):
            return pb.ff_fused(hs, rows, Cc, self.hw, P[f"{tb}.ff1.weight"], P[f"{tb}.ff1.bias"], P[f"{tb}.ff1.colsum"],
                               st, self.tiles, P[w2n], P[f"{pre}.ff2_proj_out.bias"], out,
                               res1=x.ptr, res1_wrap=wrap, res2=res2, w2_kperm=not net.ff_w8)
        # GEGLU fused into the first GEMM's epilogue
        ln, kw = self.normed(hs, st, "norm3", "ff1", rows)
        g = pb.linear(ln, rows, Cc, P[f"{tb}.ff1.weight"], 8 * Cc, act=L.PP_ACT_GEGLU, name="linear_geglu", **kw)
        if net.merge_ff2_proj_out:
            pb.linear(g, rows, 4 * Cc, P[f"{pre}.ff2_proj_out.weight"], Cc, P[f"{pre}.ff2_proj_out.bias"], x2=hs, K2=Cc,
                      ldx2=Cc, res1=x.ptr, res1_wrap=wrap, res2=res2, out=out, name="linear")
        else:
            hs = pb.linear(g, rows, 4 * Cc, P[f"{tb}.ff2.weight"], Cc, P[f"{tb}.ff2.bias"], res1=hs, name="linear")
            pb.linear(hs, rows, Cc, P[f"{pre}.proj_out.weight"], Cc, P[f"{pre}.proj_out.bias"], res1=x.ptr, res1_wrap=wrap,
                      res2=res2, out=out, name="conv1x1")
        return pb.last_gemm


class SDNet:
    """One network of the SD-1.5 family ("unet" | "brushnet" | "controlnet") compiled to HIP launch plans.

    Mirrors the wiring of /root/reference/powerpaint/models/unet_2d_condition.py:1040-1363 (UNet incl. the fork's
    *_add_samples), /root/reference/powerpaint/models/BrushNet_CA.py:690-952 (BrushNet) and the diffusers-0.27.0
    ControlNetModel used at /root/reference/powerpaint/pipelines/pipeline_PowerPaint_ControlNet.py:1686-1694.
    """

    # BasicTransformerBlock.norm1/2/3 folded into the GEMMs on either side (no LayerNorm launch, no normalised copy in
    # HBM).  (lab) PP_FOLD_LN=0 keeps the stand-alone pp_layernorm launches (A/B measurements, bisecting).
    fold_ln = _lab_switch("PP_FOLD_LN")
    # FeedForward.net[2] and Transformer2DModel.proj_out composed into one GEMM ((lab) PP_MERGE_FF2=0: two launches)
    merge_ff2_proj_out = _lab_switch("PP_MERGE_FF2")
    fuse_conv_out = _lab_switch("PP_FUSE_CONV_OUT")      # (lab) =0: conv_norm_out apply and conv_out as two launches
    # the C = 320 cross-attention sub-blocks (norm2 -> to_q -> 77-key attention -> to_out + residual) as ONE pp_xattn_block
    # launch each, K / V folded into the projections once per prompt (pp_xattn_fold in the setup plan): 55 against 66 us
    # per block at 64x64, step -0.55 % (profiles/r03_xattn_fused_ab.txt).  (lab) PP_XATTN_FUSED=0: the three-launch chain
    fuse_xattn = _lab_switch("PP_XATTN_FUSED")
    # round 4: Transformer2DModel.norm -> proj_in -> LayerNorm1-folded QKV at C = 320 as ONE launch (csrc/tfront.hip;
    # three launches and two activation round trips before).  (lab) PP_TFRONT=0: the chain
    fuse_tfront = _lab_switch("PP_TFRONT")
    # round 5: BasicTransformerBlock.attn1.to_out (+ residual) rides in front of the fused cross-attention block at C = 320
    # (five more weight slabs in pp_xattn_block, one launch and one hidden-state round trip less).  (lab) PP_XATTN_PRE=0
    fuse_xattn_pre = _lab_switch("PP_XATTN_PRE")
    # round 5: FeedForward (GEGLU) + FF2 . proj_out at C = 320 as ONE launch with the hidden dimension streamed
    # (csrc/ff_fused.hip; two launches and the [M][4C] GEGLU round trip before).  (lab) PP_FF_FUSED=0: the two launches
    fuse_ff = _lab_switch("PP_FF_FUSED")
    # ... as the 8-wave kernel (two waves per SIMD, GEGLU values exchanged through LDS, W2' in natural hidden order).
    # (lab) PP_FF_W8=0: the 4-wave kernel (one wave per SIMD, GEGLU chained in registers, W2' hidden index permuted)
    ff_w8 = _lab_switch("PP_FF_W8")
    # round 5: the fused front end hands Q over pre-multiplied by d^-0.5 * log2(e) and self-attention runs the
    # PP_ATTN_PIPE_LOG2 form of the pipelined kernel (no multiply-add per score).  (lab) PP_ATTN_LOG2=0: plain Q
    attn_log2 = _lab_switch("PP_ATTN_LOG2")
    # round 4: the same for C = 640 / 1280 (64-row tiles x 320-column groups, xattn_wide_kernel).  (lab) PP_XATTN_WIDE=0
    # keeps the chain at those levels
    fuse_xattn_wide = _lab_switch("PP_XATTN_WIDE")
    # ... up to this width: at C = 1280 the kernel loses (59 against 47 us per block: four column groups recompute the
    # logits, and a 4-wave workgroup pays ~150 cycles of issue per LDS-DMA piece with no partner wave to hide it);
    # (lab) PP_XATTN_WIDE_C=1280 runs it there too
    xattn_wide_max_c = int(os.environ.get("PP_XATTN_WIDE_C", "640")) if os.environ.get("PP_LAB") == "1" else 640
    # round 5: above that width (C = 1280: the 16x16 level and the mid block) the folded sub-block runs as TWO plain GEMMs with
    # per-prompt weights -- logits + per-head softmax in the first one's epilogue (PP_ACT_SOFTMAX80), probabilities x H^T +
    # residual in the second -- instead of to_q -> 77-key attention -> to_out: one launch less and half the multiplications
    # per block.  (lab) PP_XATTN_2G=0: the three-launch chain
    fuse_xattn_2g = _lab_switch("PP_XATTN_2G")
    # ResnetBlock2D.conv_shortcut merged into conv2 as a 1x1 K tail (needs 64-channel multiples; (lab) PP_MERGE_SHORTCUT=0 off)
    _merge_shortcut_env = _lab_switch("PP_MERGE_SHORTCUT")

    def __init__(self, kind: str, in_channels: int, block_out_channels=(320, 640, 1280, 1280), layers_per_block=2,
                 heads=8, cross_attention_dim=768, groups=32, eps=1e-5,
                 down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
                 up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"),
                 conditioning_channels: int = 0, cond_embed_channels=(16, 32, 96, 256), out_channels: int = 4,
                 dtype: torch.dtype = torch.bfloat16, time_cond_proj_dim: Optional[int] = None):
        assert kind in ("unet", "brushnet", "controlnet")
        # guidance-embedded (LCM-distilled) UNet: TimestepEmbedding.cond_proj [boc[0]][d], no bias (diffusers 0.27)
        if time_cond_proj_dim is not None and (kind != "unet" or int(time_cond_proj_dim) <= 0 or int(time_cond_proj_dim) % 8):
            raise L.PPError(f"time_cond_proj_dim={time_cond_proj_dim!r}: a positive multiple of 8, on the UNet only")
        self.time_cond_proj_dim = int(time_cond_proj_dim) if time_cond_proj_dim is not None else None
        L.dtype_code(dtype)              # bf16 | fp16 (raises otherwise)
        self.dtype = dtype
        self.kind = kind
        self.in_channels = in_channels
        self.conditioning_channels = conditioning_channels
        # channels of the network input as conv_in sees it, and as the input buffer stores it (zero-padded: see build_step)
        self.cin0 = in_channels + (conditioning_channels if kind == "brushnet" else 0)
        self.cin_pad = _align(self.cin0, CIN_CHUNK)
        self.boc = tuple(block_out_channels)
        self.merge_shortcut = self._merge_shortcut_env and all(c % 64 == 0 for c in self.boc)
        self.L = layers_per_block
        self.heads = heads
        self.ctx_dim = cross_attention_dim
        self.groups, self.eps = groups, eps
        self.down_types, self.up_types = tuple(down_block_types), tuple(up_block_types)
        self.cond_embed_channels = tuple(cond_embed_channels)
        self.out_channels = out_channels
        self.params: Optional[ParamPack] = None
        self.P: Dict[str, int] = {}
        self.temb_off: Dict[str, int] = {}
        self.temb_total = 0
        # IP-Adapters (set_ip_adapters): per adapter (tokens per image, image-embed dimension) -- the plain pair for a base
        # adapter, an ip_adapter.IPPlus (the pair, then the Resampler's sizes) for a Plus one; empty = a network without any
        self.ip: List[Tuple[int, ...]] = []
        # what build_setup leaves for build_step (per plan: every build_setup starts them afresh)
        self._nctx = 0                                          # context tokens
        self.kv: Dict[str, Tuple[int, int, int, int]] = {}      # transformer -> hoisted cross-attention (K, ldk, V^T, ldvt)
        self.xa: Dict[str, XAttnFold] = {}                      # ... -> folded cross-attention operands (none: the chain)
        self.ip_kv: Dict[str, List[Tuple[int, int, int]]] = {}  # ... -> per IP-Adapter (K_i, V_i, tokens)
        self.ip_scale_cells: list = []                          # per IP-Adapter: its ctypes.c_float scale cell
        self.ip_row_w: Dict[int, List[int]] = {}                # ip_adapter_masks: {queries of a level: weight buffer per adapter}
        self.ip_tok: List[Tuple[int, int]] = []                 # per IP-Adapter: (image tokens e_i, tokens per batch item)
        self.upfold: Dict[str, int] = {}                        # upsampler conv -> its sub-pixel folded weights
        self.cond_emb: Optional[Act] = None                     # (controlnet) the conditioning embedding
        for c in self.boc:
            if c % 64 or (c // heads) not in (40, 80, 160):
                raise L.PPError(f"unsupported channel width {c} (need multiple of 64 and head_dim in 40/80/160)")

    # ---------------------------------------------------------------- structure walk (shared by params and plans)
    def _resnet_specs(self) -> List[Tuple[str, int, int]]:
        """(prefix, cin, cout) of every ResnetBlock2D in execution order."""
        out = []
        boc, Lp = self.boc, self.L
        oc = boc[0]
        for i in range(len(boc)):
            ic, oc = oc, boc[i]
            for j in range(Lp):
                out.append((f"down_blocks.{i}.resnets.{j}", ic if j == 0 else oc, oc))
        out.append(("mid_block.resnets.0", boc[-1], boc[-1]))
        out.append(("mid_block.resnets.1", boc[-1], boc[-1]))
        if self.kind != "controlnet":
            rev = list(reversed(boc))
            oc = rev[0]
            for i in range(len(boc)):
                prev, oc = oc, rev[i]
                ic = rev[min(i + 1, len(boc) - 1)]
                for j in range(Lp + 1):
                    skip = ic if j == Lp else oc
                    rin = prev if j == 0 else oc
                    out.append((f"up_blocks.{i}.resnets.{j}", rin + skip, oc))
        return out

    def _attn_specs(self) -> List[Tuple[str, int]]:
        out = []
        for i, t in enumerate(self.down_types):
            if t == "CrossAttnDownBlock2D":
                out += [(f"down_blocks.{i}.attentions.{j}", self.boc[i]) for j in range(self.L)]
        out.append(("mid_block.attentions.0", self.boc[-1]))
        if self.kind != "controlnet":
            rev = list(reversed(self.boc))
            for i, t in enumerate(self.up_types):
                if t == "CrossAttnUpBlock2D":
                    out += [(f"up_blocks.{i}.attentions.{j}", rev[i]) for j in range(self.L + 1)]
        return out

    _tome_step: Optional[Dict[str, object]] = None
    _pag_step: Optional[PAG] = None  # perturbed-attention guidance of the step plan being built (build_step(pag=...))
    _ht_step: Optional[Dict[str, Tuple[int, int, bool, str]]] = None   # hypertile_layout of the step plan being built
    hypertile: Optional[HyperTile] = None   # tiled top-level self-attention (powerpaint_amd/hypertile.py)

    def hypertile_layout(self, H: int, W: int) -> Dict[str, Tuple[int, int, bool, str]]:
        """THE place that decides which self-attentions run tiled on an H x W latent: {prefix: (nh, nw, tiled, reason)} over
        every transformer in execution order ({} without the patch).  A block tiles when its token grid is the latent grid
        itself (depth 0), the rule gives more than one tile and pp_attention_tiled_ok takes the geometry; `reason` says which
        of these failed."""
        t = self.hypertile
        if t is None:
            return {}
        n = len(self.boc)
        sizes = level_sizes(H, W, n)
        out = {}
        for pre, c in self._attn_specs():
            part = pre.split(".")
            lvl = n - 1 if part[0] == "mid_block" else (int(part[1]) if part[0] == "down_blocks" else n - 1 - int(part[1]))
            h, w = sizes[lvl]
            d = c // self.heads
            if lvl != 0 or (h, w) != (H, W):
                out[pre] = (1, 1, False, f"depth {lvl}: only the blocks on the latent grid itself are tiled (max_depth = 0)")
                continue
            nh, nw = hypertile_split(h, t.tile_size), hypertile_split(w, t.tile_size)
            if nh * nw == 1:
                out[pre] = (1, 1, False, f"the rule leaves a {h}x{w} latent in one tile at tile_size {t.tile_size}")
            elif not L.lib().pp_attention_tiled_ok(h, w, nh, nw, d):
                out[pre] = (nh, nw, False, f"{nh}x{nw} tiles of {h // nh}x{w // nw} tokens at head dim {d} are outside "
                                           f"pp_attention_tiled_ok (include/pp_hip.h)")
            else:
                out[pre] = (nh, nw, True, "tiled")
        return out
    tome: Optional[ToMe] = None      # token merging (powerpaint_amd/tome.py: apply_patch / remove_patch)
    deepcache: Optional[DeepCache] = None      # shallow evaluations on a cached deep feature (powerpaint_amd/deepcache.py)

    def skip_count(self) -> int:
        """n: the skip tensors of the down path -- conv_in's output, every down layer's, every downsampler's (SD-1.5: 12)."""
        return 1 + sum(self.L + (i != len(self.boc) - 1) for i in range(len(self.boc)))

    def tome_layout(self, H: int, W: int) -> Tuple[Dict[str, ToMeBlock], int]:
        """THE place that decides which transformers merge tokens, and how many: -> ({prefix: ToMeBlock} in execution order,
        bytes of one row of the window table).  tomesd's rules: a block takes part when ceil(sqrt(orig_tokens // tokens)) <=
        max_downsample; r = int(tokens * ratio), capped at the number of source tokens; r == 0 leaves the block untouched."""
        t = self.tome
        if t is None:
            return {}, 0
        n = len(self.boc)
        sizes = level_sizes(H, W, n)
        out, off = {}, 0
        for pre, c in self._attn_specs():
            part = pre.split(".")
            lvl = n - 1 if part[0] == "mid_block" else (int(part[1]) if part[0] == "down_blocks" else n - 1 - int(part[1]))
            h, w = sizes[lvl]
            if math.ceil(math.sqrt((H * W) // (h * w))) > t.max_downsample:
                continue
            nd = (h // t.sy) * (w // t.sx)
            r = min(int(h * w * t.ratio), h * w - nd)
            if r <= 0:
                continue
            if nd < 1 or not L.lib().pp_tome_supported(h, w, c, t.sx, t.sy):
                raise L.PPError(f"token merging: {pre} ({h}x{w} tokens of {c} channels, {t.sy}x{t.sx} windows) is outside what the "
                                f"pp_tome kernels take (include/pp_hip.h, pp_tome_supported)")
            out[pre] = ToMeBlock(h, w, nd, r, off)
            off += nd
        return out, _align(off, 16)

    def _zero_conv_specs(self) -> List[Tuple[str, int]]:
        """(state-dict prefix, channels) of the 1x1 output convs (BrushNet 12+1+15, ControlNet 12+1)."""
        if self.kind == "unet":
            return []
        nm = "brushnet" if self.kind == "brushnet" else "controlnet"
        out = [(f"{nm}_down_blocks.0", self.boc[0])]
        k = 1
        for i, c in enumerate(self.boc):
            for _ in range(self.L):
                out.append((f"{nm}_down_blocks.{k}", c)); k += 1
            if i != len(self.boc) - 1:
                out.append((f"{nm}_down_blocks.{k}", c)); k += 1
        out.append((f"{nm}_mid_block", self.boc[-1]))
        if self.kind == "brushnet":
            k = 0
            for i, c in enumerate(reversed(self.boc)):
                for _ in range(self.L + 1):
                    out.append((f"brushnet_up_blocks.{k}", c)); k += 1
                if i != len(self.boc) - 1:
                    out.append((f"brushnet_up_blocks.{k}", c)); k += 1
        return out

    # ---------------------------------------------------------------- parameters
    def state_dict_spec(self) -> Dict[str, Tuple[int, ...]]:
        """diffusers-format parameter names -> shapes for this architecture (SURVEY.md section 8b "Weight naming")."""
        sp: Dict[str, Tuple[int, ...]] = {}
        boc, te = self.boc, self.boc[0] * 4

        def conv(name, cout, cin, k):
            sp[name + ".weight"] = (cout, cin, k, k)
            sp[name + ".bias"] = (cout,)

        def lin(name, cout, cin, bias=True):
            sp[name + ".weight"] = (cout, cin)
            if bias:
                sp[name + ".bias"] = (cout,)

        def norm(name, c):
            sp[name + ".weight"] = (c,)
            sp[name + ".bias"] = (c,)

        conv("conv_in_condition" if self.kind == "brushnet" else "conv_in", boc[0], self.cin0, 3)
        lin("time_embedding.linear_1", te, boc[0])
        lin("time_embedding.linear_2", te, te)
        if self.time_cond_proj_dim:
            lin("time_embedding.cond_proj", boc[0], self.time_cond_proj_dim, False)
        for pre, cin, cout in self._resnet_specs():
            norm(pre + ".norm1", cin); conv(pre + ".conv1", cout, cin, 3); lin(pre + ".time_emb_proj", cout, te)
            norm(pre + ".norm2", cout); conv(pre + ".conv2", cout, cout, 3)
            if cin != cout:
                conv(pre + ".conv_shortcut", cout, cin, 1)
        for i in range(len(boc) - 1):
            conv(f"down_blocks.{i}.downsamplers.0.conv", boc[i], boc[i], 3)
            if self.kind != "controlnet":
                c = list(reversed(boc))[i]
                conv(f"up_blocks.{i}.upsamplers.0.conv", c, c, 3)
        for pre, c in self._attn_specs():
            norm(pre + ".norm", c); conv(pre + ".proj_in", c, c, 1); conv(pre + ".proj_out", c, c, 1)
            tb = pre + ".transformer_blocks.0"
            for n in ("norm1", "norm2", "norm3"):
                norm(f"{tb}.{n}", c)
            for a, kd in (("attn1", c), ("attn2", self.ctx_dim)):
                lin(f"{tb}.{a}.to_q", c, c, False); lin(f"{tb}.{a}.to_k", c, kd, False); lin(f"{tb}.{a}.to_v", c, kd, False)
                lin(f"{tb}.{a}.to_out.0", c, c)
            lin(f"{tb}.ff.net.0.proj", 8 * c, c); lin(f"{tb}.ff.net.2", c, 4 * c)
        if self.kind == "unet":
            norm("conv_norm_out", boc[0]); conv("conv_out", self.out_channels, boc[0], 3)
        for pre, c in self._zero_conv_specs():
            conv(pre, c, c, 1)
        if self.kind == "controlnet":
            ce, ch = "controlnet_cond_embedding", self.cond_embed_channels
            conv(f"{ce}.conv_in", ch[0], self.conditioning_channels, 3)
            for i in range(len(ch) - 1):
                conv(f"{ce}.blocks.{2 * i}", ch[i], ch[i], 3)
                conv(f"{ce}.blocks.{2 * i + 1}", ch[i + 1], ch[i], 3)
            conv(f"{ce}.conv_out", boc[0], ch[-1], 3)
        return sp

    def synthetic_state_dict(self, device="cpu", seed: int = 0, meta: bool = False) -> Dict[str, torch.Tensor]:
        """Random-init weights of this architecture (there is no network for checkpoints): fan-in scaled normal for
        matrices, (1, 0) for norm affine, N(0, 0.02) for the zero-convs so that routing bugs cannot hide."""
        sp = self.state_dict_spec()
        if meta:
            return {k: torch.empty(v, device="meta") for k, v in sp.items()}
        g = torch.Generator(device=device).manual_seed(seed)
        zc = tuple(p for p, _ in self._zero_conv_specs()) + ("controlnet_cond_embedding.conv_out",)
        sd = {}
        for k, shp in sp.items():
            if k.endswith(".weight") and len(shp) == 1:
                sd[k] = torch.ones(shp, device=device)
            elif len(shp) == 1:
                sd[k] = torch.randn(shp, generator=g, device=device) * 0.02
                if ".norm" in k or k.startswith("conv_norm_out"):
                    sd[k] = torch.zeros(shp, device=device)
            else:
                fan_in = 1
                for d in shp[1:]:
                    fan_in *= d
                std = 0.02 if k.startswith(zc) else (1.0 / fan_in) ** 0.5
                sd[k] = torch.randn(shp, generator=g, device=device) * std
        return sd

    # ---------------------------------------------------------------- the packing table
    def pack_table(self) -> List[object]:
        """Every packed entry of this network in buffer order, as ONE recipe each: which diffusers tensors it is made of and
        how (PackRecipe: 16-bit matrices and the fp32 side vectors derived from them; PackVec: fp32 vectors copied from the
        state dict).  `load_state_dict` evaluates the table on the host, `repack` evaluates single recipes on the device
        (pp_lora_merge) into the slots the first one laid out.  Built once per `load_state_dict` (which also takes the
        time-embedding row offsets from it) and kept."""
        if getattr(self, "_table", None) is None:
            self._table, self.temb_off, self.temb_total = self._build_pack_table()
        return self._table

    def _build_pack_table(self):
        T: List[object] = []
        R, V = PackRecipe, PackVec

        def vec(name, key=None):
            T.append(V(name, "copy", (key or name,)))

        conv_in = "conv_in_condition" if self.kind == "brushnet" else "conv_in"
        T.append(R("conv_in.weight", [conv_in], cols="igemm", cin_pad=self.cin_pad))
        vec("conv_in.bias", conv_in + ".bias")
        for n in ("linear_1", "linear_2"):
            T.append(R(f"time_embedding.{n}.weight", [f"time_embedding.{n}"]))
            vec(f"time_embedding.{n}.bias")
        if self.time_cond_proj_dim:
            T.append(R("time_embedding.cond_proj.weight", ["time_embedding.cond_proj"]))
        # resnets
        tw, off = [], 0
        temb_off: Dict[str, int] = {}
        for pre, cin, cout in self._resnet_specs():
            for nrm in ("norm1", "norm2"):
                vec(f"{pre}.{nrm}.weight")
                vec(f"{pre}.{nrm}.bias")
                # (gamma, beta) interleaved per channel: what the fused norm -> SiLU -> conv loader DMAs per 64-channel chunk
                T.append(V(f"{pre}.{nrm}.gb", "gb", (f"{pre}.{nrm}.weight", f"{pre}.{nrm}.bias")))
            T.append(R(f"{pre}.conv1.weight", [f"{pre}.conv1"], cols="igemm"))
            vec(f"{pre}.conv1.bias")
            if cin != cout and self.merge_shortcut:
                # conv2(h) + conv_shortcut(x) = one implicit GEMM: the 1x1 shortcut is a K tail over the block input
                T.append(R(f"{pre}.conv2.weight", [f"{pre}.conv2"], cols="igemm", tail=f"{pre}.conv_shortcut"))
                T.append(V(f"{pre}.conv2.bias", "sum", (f"{pre}.conv2.bias", f"{pre}.conv_shortcut.bias")))
            else:
                T.append(R(f"{pre}.conv2.weight", [f"{pre}.conv2"], cols="igemm"))
                vec(f"{pre}.conv2.bias")
                if cin != cout:
                    T.append(R(f"{pre}.conv_shortcut.weight", [f"{pre}.conv_shortcut"]))
                    vec(f"{pre}.conv_shortcut.bias")
            tw.append(f"{pre}.time_emb_proj")
            temb_off[pre] = off
            off += cout
        temb_total = off
        T.append(R("temb_all.weight", tw))
        T.append(V("temb_all.bias", "cat", tuple(m + ".bias" for m in tw)))
        # samplers
        for i in range(len(self.boc) - 1):
            pre = f"down_blocks.{i}.downsamplers.0.conv"
            T.append(R(pre + ".weight", [pre], cols="igemm"))
            vec(pre + ".bias")
            if self.kind != "controlnet":
                pre = f"up_blocks.{i}.upsamplers.0.conv"
                T.append(R(pre + ".weight", [pre], cols="igemm"))
                vec(pre + ".bias")
        # transformers
        for pre, c in self._attn_specs():
            vec(f"{pre}.norm.weight")
            vec(f"{pre}.norm.bias")
            T.append(R(f"{pre}.proj_in.weight", [f"{pre}.proj_in"]))
            vec(f"{pre}.proj_in.bias")
            tb_ = f"{pre}.transformer_blocks.0"
            if self.merge_ff2_proj_out:
                # FF2 and proj_out are two linear maps with only a residual add between them:
                #   proj_out(FF2(g) + hs) = [g | hs] [W_po W_ff2 | W_po]^T + (W_po b_ff2 + b_po)
                # -> ONE GEMM over the K-concatenation of g and hs (same FLOPs, one launch and one hidden-state round
                # trip less per transformer); composed in fp32 at pack time.
                T.append(R(f"{pre}.ff2_proj_out.weight", [f"{pre}.proj_out"], compose=f"{tb_}.ff.net.2",
                           bias=f"{pre}.ff2_proj_out.bias", badd=f"{pre}.proj_out.bias"))
                if c == 320 and self.fuse_ff and self.fold_ln and not self.ff_w8:
                    # the same matrix with its hidden index permuted: second GEMM of the 4-wave fused feed-forward
                    T.append(R(f"{pre}.ff2_proj_out.weight_kp", [f"{pre}.proj_out"], compose=f"{tb_}.ff.net.2",
                               cols="kperm_geglu"))
            else:
                T.append(R(f"{pre}.proj_out.weight", [f"{pre}.proj_out"]))
                vec(f"{pre}.proj_out.bias")
            qkv = [f"{tb_}.attn1.to_q", f"{tb_}.attn1.to_k", f"{tb_}.attn1.to_v"]
            if self.fold_ln:
                # LayerNorm folded into the Linear that consumes it:  LN(x) W^T = rstd (x (g.W)^T - mean colsum) + W b
                def fold(name, mods, nrm, badd=None, il=False):
                    T.append(R(f"{name}.weight", mods, gamma=f"{tb_}.{nrm}", colsum=f"{name}.colsum", bias=f"{name}.bias",
                               badd=badd, row_order="geglu" if il else "plain"))

                fold(f"{tb_}.attn1.qkv", qkv, "norm1")
                if c == 320 and self.fuse_tfront:
                    # the same folded weight with its input index permuted: second GEMM of the fused front end (csrc/tfront.hip)
                    T.append(R(f"{tb_}.attn1.qkv.weight_kp", qkv, gamma=f"{tb_}.norm1", cols="kperm"))
                fold(f"{tb_}.attn2.to_q", [f"{tb_}.attn2.to_q"], "norm2")
                fold(f"{tb_}.ff1", [f"{tb_}.ff.net.0.proj"], "norm3", f"{tb_}.ff.net.0.proj.bias", il=True)
            else:
                for nrm in ("norm1", "norm2", "norm3"):
                    vec(f"{tb_}.{nrm}.weight")
                    vec(f"{tb_}.{nrm}.bias")
                T.append(R(f"{tb_}.attn1.qkv.weight", qkv))
                T.append(R(f"{tb_}.attn2.to_q.weight", [f"{tb_}.attn2.to_q"]))
                T.append(R(f"{tb_}.ff1.weight", [f"{tb_}.ff.net.0.proj"], row_order="geglu"))
                T.append(V(f"{tb_}.ff1.bias", "geglu", (f"{tb_}.ff.net.0.proj.bias",)))
            T.append(R(f"{tb_}.attn1.to_out.weight", [f"{tb_}.attn1.to_out.0"]))
            vec(f"{tb_}.attn1.to_out.bias", f"{tb_}.attn1.to_out.0.bias")
            T.append(R(f"{tb_}.attn2.kv.weight", [f"{tb_}.attn2.to_k", f"{tb_}.attn2.to_v"]))
            T.append(R(f"{tb_}.attn2.to_out.weight", [f"{tb_}.attn2.to_out.0"]))
            vec(f"{tb_}.attn2.to_out.bias", f"{tb_}.attn2.to_out.0.bias")
            if not self.merge_ff2_proj_out:
                T.append(R(f"{tb_}.ff2.weight", [f"{tb_}.ff.net.2"]))
                vec(f"{tb_}.ff2.bias", f"{tb_}.ff.net.2.bias")
        if self.kind == "unet":
            vec("conv_norm_out.weight")
            vec("conv_norm_out.bias")
            T.append(R("conv_out.weight", ["conv_out"], cols="igemm"))
            vec("conv_out.bias")
        for pre, c in self._zero_conv_specs():
            T.append(R(pre + ".weight", [pre]))
            vec(pre + ".bias")
        if self.kind == "controlnet":
            ce = "controlnet_cond_embedding"
            names = ["conv_in"] + [f"blocks.{i}" for i in range(2 * (len(self.cond_embed_channels) - 1))] + ["conv_out"]
            for n in names:
                T.append(R(f"{ce}.{n}.weight", [f"{ce}.{n}"], cols="direct"))
                vec(f"{ce}.{n}.bias")
        return T, temb_off, temb_total

    def pack_host(self, it, W) -> List[Tuple[str, torch.Tensor, torch.dtype]]:
        """One table item evaluated with torch on wherever `W(key)` (fp32 source tensor by diffusers key) lives:
        -> [(packed name, tensor, storage dtype)] in buffer order."""
        bf, f32 = self.dtype, torch.float32      # `bf`: the 16-bit storage format of matrix weights (bf16 or fp16)
        if isinstance(it, PackVec):
            k = it.keys
            if it.op == "copy":
                t = W(k[0])
            elif it.op == "sum":
                t = W(k[0]) + W(k[1])
            elif it.op == "cat":
                t = torch.cat([W(x) for x in k], 0)
            elif it.op == "gb":
                t = torch.stack([W(k[0]), W(k[1])], 1)
            else:
                t = _geglu_interleave(W(k[0]))
            return [(it.name, t, f32)]
        r = it

        def mat(m):
            w = W(m + ".weight")
            if r.cols == "igemm" and not r.compose:
                return _conv_igemm_cpad(w, r.cin_pad) if r.cin_pad else _conv_igemm(w)
            if r.cols == "direct":
                return _conv_direct(w)
            return w.reshape(w.shape[0], -1) if w.dim() == 4 else w

        if r.compose:
            w_po, w_f2 = mat(r.rows[0]), W(r.compose + ".weight")
            prod = w_po @ w_f2
            if r.cols == "kperm_geglu":
                prod = _kperm_geglu(prod)
            out = [(r.name, torch.cat([prod, w_po], 1), bf)]
            if r.bias:
                out.append((r.bias, w_po @ W(r.compose + ".bias") + W(r.badd), f32))
            return out
        ws = [mat(m) for m in r.rows]
        w = ws[0] if len(ws) == 1 else torch.cat(ws, 0)
        cs = t = None
        if r.gamma:
            g_, b_ = W(r.gamma + ".weight"), W(r.gamma + ".bias")
            wf = w * g_[None, :]
            if r.colsum:
                cs = wf.to(bf).float().sum(1)          # of the weights as the MFMA sees them
                t = w @ b_ if r.badd is None else w @ b_ + W(r.badd)
            w = wf
        if r.cols == "kperm":
            w = _kperm(w)
        if r.tail:
            wt = W(r.tail + ".weight")
            w = torch.cat([w, wt.reshape(wt.shape[0], -1)], 1)
        if r.row_order == "geglu":
            w = _geglu_interleave(w)
            if cs is not None:
                cs, t = _geglu_interleave(cs), _geglu_interleave(t)
        out = [(r.name, w, bf)]
        if cs is not None:
            out += [(r.colsum, cs, f32), (r.bias, t, f32)]
        return out

    def load_state_dict(self, sd: Dict[str, torch.Tensor], device, materialize: bool = True):
        """sd: diffusers-format state dict (fp32/any float, CPU or meta).  Packs into kernel layouts on `device`."""
        pk = ParamPack()

        def W(k):
            return sd[k].float() if sd[k].device.type != "meta" else sd[k]

        self._table = None                     # (the lab switches may have changed since the last load)
        for it in self.pack_table():
            for name, t, dt in self.pack_host(it, W):
                pk.add(name, t, dt)
        pk.to_device(device, materialize)
        self.params, self.P = pk, pk.ptr
        self.ip = []                           # (IP-Adapter entries lived behind the old buffer's own entries: gone with it)
        self._own_bytes = pk.total
        return self

    def recipes_of(self, modules) -> List["PackRecipe"]:
        """The recipes (in buffer order) whose packed entry depends on the weight of one of these source modules."""
        mods = set(modules)
        return [r for r in self.pack_table() if isinstance(r, PackRecipe) and mods & set(r.sources())]

    def repack(self, modules, merged: Dict[str, list], source: Dict[str, torch.Tensor], stream: Optional[int] = None,
               composed_out: Optional[dict] = None):
        """Rebuild, on the device and in place, every packed entry that depends on the weight of one of `modules`
        (diffusers module names, e.g. "mid_block.attentions.0.proj_in"), then `params.touch()`.
          merged: module -> [(up [N][r], down [r][K], coefficient), ...] fp32 device tensors: the low-rank terms folded into that
                  module's weight (W + sum c U D; a module that is not named is repacked as it is);
          source: diffusers key -> fp32 device tensor, at least the weights of every source module of the touched recipes,
                  the LayerNorm weight / bias of the folded ones and the biases their side vectors take in.
        The sums are formed in fp32 and rounded once, after the pack-time transformations (pp_lora_merge); a composed entry
        ([W_po W_ff2 | W_po]) goes through fp32 temporaries of its two merged factors (handed out through `composed_out`:
        recipe name -> (W_po', W_po' @ W_ff2'), for whoever wants to check them).  Returns the recipes it rebuilt."""
        if self.params is None or self.params.buf is None or self.params.buf.device.type != "cuda":
            raise L.PPError("SDNet.repack: the parameters must be packed on the GPU first (load_state_dict)")
        lib = L.lib()
        recipes = self.recipes_of(modules)
        keep = []                      # temporaries and argument records stay alive until every launch is queued
        cache: Dict[Tuple[str, str], Tuple[torch.Tensor, torch.Tensor]] = {}
        dev = self.params.buf.device
        if stream is None:             # (the fp32 temporaries are torch allocations: the launches go where torch orders them)
            stream = torch.cuda.current_stream(dev).cuda_stream

        def src(key):
            if key not in source:
                raise L.PPError(f"SDNet.repack: the fp32 source tensor {key!r} is missing")
            t = source[key]
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                raise L.PPError(f"SDNet.repack: source tensor {key!r} must be contiguous fp32 on {dev}")
            return t

        def launch(w, N, K, ads, out, out_dt, ldo, out_rows, out_cols, row_mode=0, row_off=0, col_mode=0, col_off=0, taps=0,
                   cin_pad=0, gamma=None, beta=None, badd=None, colsum=None, bias=None):
            if len(ads) > L.PP_LORA_MAX_ADAPTERS:
                raise L.PPError(f"at most {L.PP_LORA_MAX_ADAPTERS} adapters can be merged into one module "
                                f"({len(ads)} active)")
            a = L.PPLoraMergeArgs()
            a.N, a.K, a.w, a.ldw, a.n_adapters = N, K, w.data_ptr(), K, len(ads)
            for i, (up, down, coef) in enumerate(ads):
                rk = down.shape[0]
                if rk > L.PP_LORA_MAX_RANK:
                    raise L.PPError(f"adapter rank {rk} is above the kernel's limit of {L.PP_LORA_MAX_RANK}")
                if up.numel() != N * rk or down.numel() != rk * K or up.dtype != torch.float32 or \
                        down.dtype != torch.float32 or not up.is_contiguous() or not down.is_contiguous():
                    raise L.PPError(f"adapter factors do not fit a [{N}][{K}] weight: up {tuple(up.shape)}, down "
                                    f"{tuple(down.shape)} (contiguous fp32 expected)")
                a.rank[i], a.coef[i], a.up[i], a.down[i] = rk, float(coef), up.data_ptr(), down.data_ptr()
            ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
            a.gamma, a.beta, a.badd = ptr(gamma), ptr(beta), ptr(badd)
            a.out, a.ldo, a.out_rows, a.out_cols, a.out_dtype = out.data_ptr(), ldo, out_rows, out_cols, out_dt
            a.row_mode, a.row_off, a.col_mode, a.col_off, a.taps, a.cin_pad = row_mode, row_off, col_mode, col_off, taps, cin_pad
            a.colsum, a.bias = ptr(colsum), ptr(bias)
            keep.append((a, w, ads, gamma, beta, badd))
            L.check(lib.pp_lora_merge(C.byref(a), stream), "pp_lora_merge")

        dt16 = L.dtype_code(self.dtype)
        cmode = {"plain": L.PP_LORA_COLS_PLAIN, "igemm": L.PP_LORA_COLS_IGEMM, "kperm": L.PP_LORA_COLS_KPERM,
                 "kperm_geglu": L.PP_LORA_COLS_KPERM_GEGLU}
        for r in recipes:
            if r.cols == "direct":
                raise L.PPError(f"{r.name}: this layout is not rebuilt on the device (the network takes no adapters)")
            dst = self.params.tensor(r.name)
            R_, Ct = dst.shape
            if r.compose:
                po, f2 = r.rows[0], r.compose
                if (po, f2) not in cache:
                    w_po, w_f2 = src(po + ".weight"), src(f2 + ".weight")
                    Cc, F = w_po.shape[0], w_f2.shape[1]
                    t1 = torch.empty(Cc, Cc, dtype=torch.float32, device=dev)
                    t2 = torch.empty(Cc, F, dtype=torch.float32, device=dev)
                    launch(w_f2, Cc, F, merged.get(f2, ()), t2, L.PP_DT_F32, F, Cc, F)
                    if r.bias is None:
                        raise L.PPError(f"{r.name}: the first recipe of a composed pair carries the bias")
                    launch(w_po, Cc, Cc, merged.get(po, ()), t1, L.PP_DT_F32, Cc, Cc, Cc, beta=src(f2 + ".bias"),
                           badd=src(r.badd), bias=self.params.tensor(r.bias))
                    cache[(po, f2)] = (t1, t1 @ t2)
                t1, prod = cache[(po, f2)]
                if composed_out is not None:
                    composed_out[r.name] = (t1, prod)
                Cc, F = prod.shape
                launch(prod, Cc, F, (), dst, dt16, Ct, R_, Ct, col_mode=cmode[r.cols])
                launch(t1, Cc, Cc, (), dst, dt16, Ct, R_, Ct, col_off=F)
                continue
            gamma = src(r.gamma + ".weight") if r.gamma else None
            beta = src(r.gamma + ".bias") if r.gamma and r.colsum else None
            colsum = self.params.tensor(r.colsum) if r.colsum else None
            bias = self.params.tensor(r.bias) if r.colsum else None
            row_off, kd = 0, 0
            for m in r.rows:
                w = src(m + ".weight")
                N, K = w.shape[0], w.numel() // w.shape[0]
                taps = K // w.shape[1] if r.cols == "igemm" else 0
                cpad = (r.cin_pad or w.shape[1]) if r.cols == "igemm" else 0
                kd = taps * cpad if r.cols == "igemm" else K
                launch(w, N, K, merged.get(m, ()), dst, dt16, Ct, R_, Ct, row_off=row_off, col_mode=cmode[r.cols], taps=taps,
                       cin_pad=cpad, row_mode=L.PP_LORA_ROWS_GEGLU if r.row_order == "geglu" else L.PP_LORA_ROWS_PLAIN,
                       gamma=gamma, beta=beta, badd=src(r.badd)[row_off:row_off + N] if r.badd else None, colsum=colsum,
                       bias=bias)             # (the kernel indexes badd by the block's own rows)
                row_off += N
            if r.tail:
                w = src(r.tail + ".weight")
                N, K = w.shape[0], w.numel() // w.shape[0]
                launch(w, N, K, merged.get(r.tail, ()), dst, dt16, Ct, R_, Ct, col_off=kd)
        self.params.touch()
        self.repack_launches = len(keep)      # (temporaries are stream-ordered allocations: safe to let go once queued)
        return recipes

    # ---------------------------------------------------------------- IP-Adapter parameters (DESIGN.md "IP-Adapter")
    def ip_attn_order(self) -> List[str]:
        """The transformers in the order an IP-Adapter file numbers their cross-attentions: the order of the reference
        UNet's `attn_processors` -- down blocks, then UP blocks, then the mid block (its registration order) -- where
        _attn_specs() walks in execution order."""
        pres = [p for p, _ in self._attn_specs()]
        return [p for head in ("down_blocks.", "up_blocks.", "mid_block.") for p in pres if p.startswith(head)]

    def set_ip_adapters(self, adapters: Sequence[Dict[str, object]]):
        """Replace the IP-Adapter entries of the packed buffer.  adapters: per adapter {"proj.weight" [T * ctx][D], "proj.bias"
        [T * ctx], "norm.weight" [ctx], "norm.bias" [ctx], "kv": {transformer prefix: (to_k_ip [C][ctx], to_v_ip [C][ctx])}}
        (validated by the caller, models/unet_2d_condition.py); [] removes them.  Packed behind the network's own entries:
          ip_adapter.<i>.proj.weight   16-bit [T * ctx][D rounded up to 64] (zero columns: the GEMM contracts 64 at a time)
          ip_adapter.<i>.proj.bias, .norm.weight, .norm.bias   fp32
          ip_adapter.<i>.<transformer>.kv.weight   16-bit [2 C][ctx] = [to_k_ip; to_v_ip], as attn2.kv.weight
        A Plus adapter (ad["kind"] == "plus", ad["plus"] its ip_adapter.IPPlus) brings the Resampler's file keys instead of
        proj / norm and is packed as
          ip_adapter.<i>.resampler.latents   16-bit [Q][dim]
          ip_adapter.<i>.resampler.{proj_in,proj_out}.weight   16-bit (proj_in [dim][E rounded up to 64], zero columns), .bias
                                                               fp32;  .norm_out.{weight,bias}   fp32
          ip_adapter.<i>.resampler.layers.<l>.{to_q,to_kv,to_out,ff1,ff2}.weight   16-bit (to_kv = [K rows; V rows], as filed)
          ip_adapter.<i>.resampler.layers.<l>.{norm1,norm2,ff_norm}.{weight,bias}   fp32
        with the same kv.weight pairs.  Base and Plus adapters mix freely.
        They are no source of any PackRecipe: `repack` (LoRA) never touches them.  Every packed pointer moves."""
        if self.kind != "unet":
            raise L.PPError("IP-Adapters attach to the UNet's cross-attentions only")
        pk = self.params
        if pk is None or pk.buf is None:
            raise L.PPError("SDNet.set_ip_adapters: pack the network's own parameters first (load_state_dict)")
        if not self.ip and not adapters:
            return self
        pk.forget("ip_adapter.", self._own_bytes)
        ip = []
        for i, ad in enumerate(adapters):
            if ad.get("kind") == "plus":
                sp = ad["plus"]
                R = f"ip_adapter.{i}.resampler"
                pk.add(f"{R}.latents", ad["latents"].float()[0], self.dtype)
                w_in = torch.zeros(sp.dim, _align(sp.D, 64))          # (zero columns up to the GEMM's 64, as a base proj.weight)
                w_in[:, :sp.D] = ad["proj_in.weight"].float()
                for n, w in (("proj_in", w_in), ("proj_out", ad["proj_out.weight"].float())):
                    pk.add(f"{R}.{n}.weight", w, self.dtype)
                    pk.add(f"{R}.{n}.bias", ad[f"{n}.bias"].float(), torch.float32)
                for wb in ("weight", "bias"):
                    pk.add(f"{R}.norm_out.{wb}", ad[f"norm_out.{wb}"].float(), torch.float32)
                for l in range(sp.depth):
                    for dst, src in (("to_q", "0.to_q"), ("to_kv", "0.to_kv"), ("to_out", "0.to_out"), ("ff1", "1.1"), ("ff2", "1.3")):
                        pk.add(f"{R}.layers.{l}.{dst}.weight", ad[f"layers.{l}.{src}.weight"].float(), self.dtype)
                    for dst, src in (("norm1", "0.norm1"), ("norm2", "0.norm2"), ("ff_norm", "1.0")):
                        for wb in ("weight", "bias"):
                            pk.add(f"{R}.layers.{l}.{dst}.{wb}", ad[f"layers.{l}.{src}.{wb}"].float(), torch.float32)
                ip.append(sp)
            else:
                w = ad["proj.weight"].float()
                D = w.shape[1]
                T = w.shape[0] // self.ctx_dim
                wp = torch.zeros(w.shape[0], _align(D, 64))
                wp[:, :D] = w
                pk.add(f"ip_adapter.{i}.proj.weight", wp, self.dtype)
                for n in ("proj.bias", "norm.weight", "norm.bias"):
                    pk.add(f"ip_adapter.{i}.{n}", ad[n].float(), torch.float32)
                ip.append((T, D))
            for pre, _ in self._attn_specs():
                wk, wv = ad["kv"][pre]
                pk.add(f"ip_adapter.{i}.{pre}.kv.weight", torch.cat([wk.float(), wv.float()], 0), self.dtype)
        pk.regrow(self._own_bytes)
        self.P = pk.ptr
        self.ip = ip
        return self

    # ---------------------------------------------------------------- plan pieces
    def _resnet(self, pb: Builder, pre: str, x: Act, cout: int, temb_all: int, x2: Optional[Act] = None,
                res2: int = 0) -> Act:
        P = self.P
        cin = x.C + (x2.C if x2 is not None else 0)
        out = pb.new_act(x.B, x.H, x.W, cout)
        m = pb.mark()
        def gn(nrm):
            return (P[f"{pre}.{nrm}.weight"], P[f"{pre}.{nrm}.bias"], P[f"{pre}.{nrm}.gb"], self.eps, self.groups)

        h = pb.conv3x3(x, P[f"{pre}.conv1.weight"], cout, P[f"{pre}.conv1.bias"], x2=x2,
                       rowvec=temb_all + 4 * self.temb_off[pre], name="conv3x3", gn_in=gn("norm1"))
        pb.tap_inner(pre + ".conv1", h)
        if cin != cout and self.merge_shortcut:
            pb.conv3x3(h, P[f"{pre}.conv2.weight"], cout, P[f"{pre}.conv2.bias"], res2=res2, out=out, x3=x, x4=x2,
                       name="conv3x3", gn_in=gn("norm2"))
            pb.release(m)
            pb.taps.append((pre, out))
            return out
        if cin != cout:
            sc = pb.linear(x.ptr, x.rows, x.C, P[f"{pre}.conv_shortcut.weight"], cout, P[f"{pre}.conv_shortcut.bias"],
                           x2=(x2.ptr if x2 is not None else 0), K2=(x2.C if x2 is not None else 0), name="conv1x1")
        else:
            assert x2 is None
            sc = x.ptr
        pb.conv3x3(h, P[f"{pre}.conv2.weight"], cout, P[f"{pre}.conv2.bias"], res1=sc, res2=res2, out=out,
                   name="conv3x3", gn_in=gn("norm2"))
        pb.release(m)
        pb.taps.append((pre, out))
        return out

    def xattn_form(self, lib, c: int, hw: int, B: int, nctx: int) -> XAttnForm:
        """The form of the cross-attention sub-block of a transformer of width c whose level has hw positions per batch item,
        at full batch B: the ONE place that reads the fuse_xattn* switches and probes pp_xattn_block_supported (DESIGN.md
        "Cross-attention forms").  build_setup folds by it, the step plan runs what was folded, twin_prefix_ok asks it."""
        if not (self.fuse_xattn and not self.ip and lib.pp_xattn_block_supported(128, c, 128, nctx, self.heads)):
            return XAttnForm.CHAIN
        wide = self.fuse_xattn_wide and c <= self.xattn_wide_max_c
        if self.fuse_xattn_2g and c > 320 and hw > 0 and hw % 64 == 0 and not wide:
            return XAttnForm.TWO_GEMM          # whole 64-row GEMM tiles per batch item
        if not (hw > 0 and lib.pp_xattn_block_supported(B * hw, c, hw, nctx, self.heads)):
            return XAttnForm.CHAIN
        if c == 320 and self.fold_ln and self.fuse_xattn_pre:
            return XAttnForm.BLOCK_PRE
        return XAttnForm.BLOCK if (c == 320 or wide) else XAttnForm.CHAIN

    def xattn_forms(self, lib, B: int, H: int, W: int, nctx: int) -> Dict[str, Tuple[XAttnForm, int]]:
        """transformer -> (form, positions per batch item) for a step over H x W latents at batch B."""
        nl = len(self.boc)
        sizes = level_sizes(H, W, nl)
        out = {}
        for pre, c in self._attn_specs():
            part = pre.split(".")
            lvl = int(part[1]) if part[0] == "down_blocks" else (nl - 1 if part[0] == "mid_block" else nl - 1 - int(part[1]))
            hw = sizes[lvl][0] * sizes[lvl][1]
            out[pre] = (self.xattn_form(lib, c, hw, B, nctx), hw)
        return out

    def _transformer(self, pb: Builder, pre: str, x: Act, kv: Tuple[int, int, int, int], res2: int = 0,
                     twin: bool = False) -> Act:
        """kv = (k_ptr, ldk, vt_ptr, ldvt) of the hoisted cross-attention K / V^T; nk = ctx tokens in self._nctx.
        twin: x is ONE half of a CFG pair whose halves are identical up to here (build_step): norm / proj_in / attn1 run on
        that half, the fused cross-attention block -- the first consumer that mixes the prompt in -- reads it with batch-wrap
        addressing, and everything behind it (and the returned Act) is the full batch."""
        t = _TransformerBlock(self, pb, pre, x, twin)
        out = pb.new_act(2 * x.B if twin else x.B, x.H, x.W, x.C)
        m = pb.mark()
        hs, a = t.self_attention()
        hs, st = t.cross_attention(hs, a, self.xa.get(pre), kv)
        out.producer = t.feed_forward(hs, st, out.ptr, res2)
        pb.release(m)
        pb.taps.append((pre, out))
        return out

    def _resampler(self, pb: Builder, R: str, sp, x_in: int, N: int, S: int, lat0: int) -> int:
        """IP-Adapter Plus's image projection over N = B n images (DESIGN.md "IP-Adapter"): x_in = hidden states [N S][E rounded up to
        64] (zero pad columns), lat0 = the latents repeated N times [N Q][dim] (only read) -> the tokens [N Q][ctx].  proj_in; per layer LayerNorm1(x),
        LayerNorm2(l), to_q, to_kv over the image rows and over the latent rows (two buffers: the two segments
        pp_perceiver_attn reads), the attention, to_out + l, LayerNorm, W1 with GELU, W2 + l; proj_out, norm_out."""
        P = self.P
        Q, E, dim, inner, ff = sp.T, sp.D, sp.dim, sp.heads * 64, sp.ff
        # Every buffer is allocated once and reused by all layers; none is ever released: what the runtimes allocate behind the
        # setup plan lives for the whole call (tables made once per plan among it), and this plan runs again at every call.
        la, lb = pb.alloc(N * Q * dim * 2), pb.alloc(N * Q * dim * 2)      # the residual stream, ping-pong
        x, xn = pb.alloc(N * S * dim * 2), pb.alloc(N * S * dim * 2)
        ln, h, q, a = (pb.alloc(N * Q * c * 2) for c in (dim, dim, inner, inner))
        kvx, kvl, g = pb.alloc(N * S * 2 * inner * 2), pb.alloc(N * Q * 2 * inner * 2), pb.alloc(N * Q * ff * 2)
        pb.linear(x_in, N * S, _align(E, 64), P[f"{R}.proj_in.weight"], dim, P[f"{R}.proj_in.bias"], out=x, name="linear")
        l = lat0
        for j in range(sp.depth):
            Lp = f"{R}.layers.{j}"
            pb.layernorm(x, N * S, dim, P[f"{Lp}.norm1.weight"], P[f"{Lp}.norm1.bias"], out=xn)
            pb.layernorm(l, N * Q, dim, P[f"{Lp}.norm2.weight"], P[f"{Lp}.norm2.bias"], out=ln)
            pb.linear(ln, N * Q, dim, P[f"{Lp}.to_q.weight"], inner, out=q, name="linear")
            pb.linear(xn, N * S, dim, P[f"{Lp}.to_kv.weight"], 2 * inner, out=kvx, name="linear")
            pb.linear(ln, N * Q, dim, P[f"{Lp}.to_kv.weight"], 2 * inner, out=kvl, name="linear")
            pb.perceiver_attn(q, inner, kvx, 2 * inner, S, kvl, 2 * inner, Q, N, sp.heads, Q, out=a)
            pb.linear(a, N * Q, inner, P[f"{Lp}.to_out.weight"], dim, res1=l, out=lb, name="linear")
            pb.layernorm(lb, N * Q, dim, P[f"{Lp}.ff_norm.weight"], P[f"{Lp}.ff_norm.bias"], out=h)
            pb.linear(h, N * Q, dim, P[f"{Lp}.ff1.weight"], ff, act=L.PP_ACT_GELU, out=g, name="linear")
            pb.linear(g, N * Q, ff, P[f"{Lp}.ff2.weight"], dim, res1=lb, out=la, name="linear")
            l = la
        y = pb.linear(l, N * Q, dim, P[f"{R}.proj_out.weight"], self.ctx_dim, P[f"{R}.proj_out.bias"], name="linear")
        e = pb.layernorm(y, N * Q, self.ctx_dim, P[f"{R}.norm_out.weight"], P[f"{R}.norm_out.bias"])
        # The split-K workspaces of the GEMMs above (W2 contracts ff = 3072) sat on top of the arena and are dirty from the
        # first run on.  What build_setup allocates next counts on the arena's zeros where no launch ever writes -- the pad
        # columns of V^T, which the attention multiplies by a zero probability -- so it starts above everything used here.
        pb.arena.off = max(pb.arena.off, pb.arena.peak)
        return e

    # ---------------------------------------------------------------- setup plan: step-invariant work
    def build_setup(self, pb: Builder, B: int, nctx: int, ehs: int, cond: Optional[Act] = None, *,
                    hw0: Tuple[int, int], ip_in: Sequence[Tuple[int, int]] = (), ip_scales=(), ip_row_w=None):
        """Cross-attention K and V^T for every transformer from encoder_hidden_states (bf16 [B*nctx][ctx_dim] at
        `ehs`); for ControlNet also the conditioning embedding of `cond` (NHWC bf16 image).  hw0 = (H, W) of the latents the
        step plan will be built for (xattn_forms: which cross-attention operands are folded, and in which layout).
        ip_in (a UNet with IP-Adapters, one entry per adapter): (pointer, n) of the call's image embeds, 16-bit [B][n][D rounded
        up to 64] with zero pad columns; ip_scales: the adapters' ctypes.c_float scale cells.  The image tokens
        e_i = LayerNorm(reshape(proj(embeds))) [B][n T][ctx] and, per transformer, K_i = to_k_ip(e_i) and V_i = to_v_ip(e_i),
        row-major [B][n T][C] each, are step-invariant: computed here, read by the step plan's pp_ip_attn_add launches.  For a
        Plus adapter the entry is (pointer, n, S, latents pointer): the 16-bit hidden states [B n S][E rounded up to 64] and the adapter's latents
        repeated B n times [B n Q][dim] (NetRuntime.set_ip_embeds fills both), and e_i comes out of the Resampler
        (_resampler: 10 depth + 3 launches).  While
        adapters are loaded every cross-attention is XAttnForm.CHAIN (self.xa stays empty): to_q -> attention -> to_out.
        ip_row_w (ip_adapter_masks bound): {queries per item of a cross-attention level: one fp32 [queries] buffer per adapter},
        the per-row weights the step plan's masked pp_ip_attn_add launches read (NetRuntime.set_ip_masks fills them)."""
        self._nctx = nctx
        self.ip_row_w = dict(ip_row_w or {})
        if len(ip_in) != len(self.ip) or len(ip_scales) != len(self.ip):
            raise L.PPError(f"{len(self.ip)} IP-Adapters are loaded, the setup plan was given {len(ip_in)} image-embed buffers")
        self.ip_kv, self.ip_scale_cells = {}, list(ip_scales)
        ip_tok = []
        for i, (spec, entry) in enumerate(zip(self.ip, ip_in)):
            (T, D), (src, n) = spec[:2], entry[:2]
            if n < 1 or n * T > L.PP_IP_MAX_TOKENS:
                raise L.PPError(f"IP-Adapter {i}: {n} images of {T} tokens, pp_ip_attn_add takes 1..{L.PP_IP_MAX_TOKENS} tokens")
            Pn = f"ip_adapter.{i}"
            if len(spec) > 2:
                ip_tok.append((self._resampler(pb, f"{Pn}.resampler", spec, src, B * n, entry[2], entry[3]), n * T))
                continue
            y = pb.linear(src, B * n, _align(D, 64), self.P[f"{Pn}.proj.weight"], T * self.ctx_dim, self.P[f"{Pn}.proj.bias"],
                          name="linear")
            e = pb.layernorm(y, B * n * T, self.ctx_dim, self.P[f"{Pn}.norm.weight"], self.P[f"{Pn}.norm.bias"])
            ip_tok.append((e, n * T))
        self.ip_tok = ip_tok               # per adapter (e_i [B][n T][ctx], n T): what the K_i / V_i GEMMs below read
        ldvt = _align(nctx, 8)
        forms = self.xattn_forms(pb.lib, B, hw0[0], hw0[1], nctx)
        self.kv, self.xa = {}, {}
        for pre, c in self._attn_specs():
            tb = f"{pre}.transformer_blocks.0"
            vt = pb.alloc(B * c * ldvt * 2)
            k = pb.linear(ehs, B * nctx, self.ctx_dim, self.P[f"{tb}.attn2.kv.weight"], 2 * c, out_vt=vt,
                          vt_col0=c, vt_ld=ldvt, rows_per_batch=nctx, name="linear")
            self.kv[pre] = (k, c, vt, ldvt)
            for i, (e, nk_ip) in enumerate(ip_tok):
                w = self.P[f"ip_adapter.{i}.{pre}.kv.weight"]
                k_ip = pb.linear(e, B * nk_ip, self.ctx_dim, w, c, name="linear")
                v_ip = pb.linear(e, B * nk_ip, self.ctx_dim, w + c * self.ctx_dim * 2, c, name="linear")
                self.ip_kv.setdefault(pre, []).append((k_ip, v_ip, nk_ip))
            # (no folded operands for a step geometry none of the folded forms takes -- they were dead weight
            #  in the arena and in the setup plan)
            form, hw = forms[pre]
            if form is not XAttnForm.CHAIN:
                tbq = f"{tb}.attn2.to_q"
                S = self.heads * 80
                gt, ht = pb.alloc(B * S * c * 2), pb.alloc(B * c * S * 2)
                gcs, gb = pb.alloc(B * S * 4), pb.alloc(B * S * 4)
                fold = self.fold_ln
                # BLOCK_PRE: attn1.to_out runs in front of the sub-block in the same launch, whose logits then take their B
                # operand from that GEMM's accumulators -> G^T with its channel index permuted (kperm = 1)
                pb.plan.add("xattn_fold", pb.lib.pp_xattn_fold, k, c, vt, ldvt, B, nctx, self.heads, c,
                            self.P[f"{tbq}.weight"], self.P[f"{tbq}.colsum"] if fold else None,
                            self.P[f"{tbq}.bias"] if fold else None, self.P[f"{tb}.attn2.to_out.weight"],
                            float(c // self.heads) ** -0.5, gt, gcs, gb, ht, form.value, pb.dt)
                self.xa[pre] = XAttnFold(gt, gcs, gb, ht, form.value, B * hw, hw)
        # Upsample2D convs in their sub-pixel form (PPGemmArgs.subpix): the folded weights are a cache derived from the packed
        # conv weight, rebuilt with everything else here whenever ParamPack.version has moved (NetRuntime.set_context)
        self.upfold = {}
        sizes = level_sizes(hw0[0], hw0[1], len(self.boc))
        if UPCONV_SUBPIX and self.kind in ("unet", "brushnet") and not (pb.gemm_tile or pb.gemm_splitk):
            rev = list(reversed(self.boc))
            for i in range(len(rev) - 1):
                lvl = len(rev) - 1 - i
                (h, w), (ht, wt), c = sizes[lvl], sizes[lvl - 1], rev[i]      # (a cropped target keeps the nine-tap `up` request)
                if pb.lib.pp_upconv_subpix_supported_to(B, h, w, ht, wt, c, c, pb.dt) >= UPCONV_SUBPIX_FROM:
                    pre = f"up_blocks.{i}.upsamplers.0.conv"
                    self.upfold[pre] = pb.alloc(16 * c * c * 2)
                    pb.plan.add("upconv_fold", pb.lib.pp_upconv_fold, self.P[pre + ".weight"], c, c, pb.dt, self.upfold[pre])
        self.cond_emb = None
        if self.kind == "controlnet":
            assert cond is not None
            ce = "controlnet_cond_embedding"
            chans = self.cond_embed_channels
            lib = pb.lib

            def dconv(x: Act, name: str, cout: int, stride: int, silu: int) -> Act:
                ho, wo = (x.H - 1) // stride + 1, (x.W - 1) // stride + 1
                o = pb.new_act(x.B, ho, wo, cout)
                pb.plan.add("conv3x3_direct", lib.pp_conv3x3_direct, x.ptr, x.B, x.H, x.W, x.C,
                            self.P[f"{ce}.{name}.weight"], self.P[f"{ce}.{name}.bias"], cout, stride, silu, None, o.ptr,
                            pb.dt)
                return o

            e = dconv(cond, "conv_in", chans[0], 1, 1)
            for i in range(len(chans) - 1):
                e = dconv(e, f"blocks.{2 * i}", chans[i], 1, 1)
                e = dconv(e, f"blocks.{2 * i + 1}", chans[i + 1], 2, 1)
            self.cond_emb = dconv(e, "conv_out", self.boc[0], 1, 0)

    # ---------------------------------------------------------------- step plan
    def twin_prefix_ok(self, lib, B: int, H: int, W: int, nctx: int, brush: bool = False) -> bool:
        """Can build_step(twin=True) run the CFG-identical prefix of this network on one half of the batch?  Needs the
        fused cross-attention block at the first level (it is the launch that reads the half batch with wrap addressing)
        and an input that nothing prompt-dependent touches before it: no BrushNet adds inside the down path."""
        return (TWIN_PREFIX and not brush and B >= 2 and B % 2 == 0 and self.L >= 1 and self.boc[0] == 320 and
                self.down_types[0] == "CrossAttnDownBlock2D" and (H * W) % 128 == 0 and        # (down_blocks.0.attentions.0:)
                self.xattn_form(lib, 320, H * W, B, nctx) in (XAttnForm.BLOCK, XAttnForm.BLOCK_PRE))

    def build_step(self, pb: Builder, x_in: Act, t_dev: int, add_down: Optional[List[int]] = None,
                   add_mid: int = 0, add_up: Optional[List[int]] = None, ctrl_down: Optional[List[int]] = None,
                   ctrl_mid: int = 0, scale: float = 1.0, pad_uncond: bool = False, twin: bool = False,
                   freeu: int = 0, b1_eff: int = 0, tome: Optional[Dict[str, object]] = None,
                   pag: Optional[PAG] = None, depth: int = 0,
                   cached: Optional[Dict[str, object]] = None) -> Dict[str, object]:
        """Append one forward pass.  x_in: NHWC bf16 input (already channel-concatenated).  Returns outputs:
        unet -> {"eps": ptr fp32 NCHW}; brushnet -> {"down": [Act], "mid": Act, "up": [Act]}; controlnet likewise.
        pad_uncond (side networks): the pipelines' guess mode runs the side branch on the conditional half of a CFG pair
        only and hands the UNet `cat([zeros_like(d), d])` (pipeline_PowerPaint_Brushnet_CA.py:1421-1425,
        pipeline_PowerPaint_ControlNet.py:1697-1702): the residuals are written into the second half of tensors with
        twice the batch whose first half one launch per step zeroes.
        twin: the caller GUARANTEES that batch items [B/2, B) of x_in (and of the ControlNet conditioning) equal items
        [0, B/2) -- the loop builds the pair as `torch.cat([latents] * 2)` (pipeline_PowerPaint.py:990-996) over CFG-duplicated
        mask / masked-image latents.  The two halves of the forward pass are then bit-identical until the prompt enters at the
        first cross-attention (unet_2d_condition.py:1183-1236): conv_in, down_blocks.0.resnets.0 and the first transformer's
        norm / proj_in / self-attention run on ONE half (conv_in stores its rows twice -- the skip tensor's consumers in the
        up path see the full batch -- and the fused cross-attention block and the transformer's last GEMM read the half
        batch with wrap addressing).  Where twin_prefix_ok() says no, the flag changes nothing.
        freeu (unet): device pointer to fp32 (b1, s1, b2, s2) -- FreeU (unet_2d_blocks.py:2563-2587, 2706-2730 of the
        reference) runs in front of every resnet of up blocks 0 and 1, one pp_freeu launch each (Builder.freeu); it sees the
        hidden tensor with the BrushNet adds in (they ride the producers' epilogues, unet_2d_blocks.py:2629-2630) and the skip
        tensors with the ControlNet residuals on (unet_2d_condition.py:1263-1272).  0: no FreeU, the plan of a UNet without it.
        b1_eff (a UNet with time_cond_proj_dim): device pointer to the fp32 effective bias of time_embedding.linear_1,
        b1 + W1 (Wc c) for the call's guidance embedding c -- `linear_1(t_emb + cond_proj(c))` of diffusers' TimestepEmbedding
        (unet_2d_condition.py:1156) with the c-dependent term, constant over a call, taken out of the step
        (NetRuntime.set_timestep_cond fills it).  0: the parameter's own bias.
        pag (unet): perturbed-attention guidance -- in the transformers pag.layers the self-attention of the LAST pag.n batch
        items is the identity (`_TransformerBlock.attend`: the attention launch on the leading items, one pp_attn_identity_v
        launch for the rest); the CFG twin prefix is not taken.  None: the plan of a UNet without it.
        depth = k > 0 (DeepCache, DESIGN.md "DeepCache"; k = cache_branch_id + 1): with S[0..n-1] the skip tensors in the order
        the down path makes them and U[0..n-1] the up layers in execution order, `c` is the hidden tensor handed to U[n-1-k],
        every side-network add on it included.  Without `cached` this is the FULL form: today's walk, launch for launch, which
        also returns where c lives ("cache": Act; with FreeU at that layer the scaled hidden tensor goes to a copy, so that c
        itself survives).  With `cached` = the outputs the full form returned this is the SHALLOW form of the same walk: the
        down loop stops behind S[k], the mid block is left out, the up loop starts at U[n-1-k] on an Act for c that has no
        producer (its norm takes the statistics launch), and the results -- eps, or the zero convs of the live positions --
        land where the full form puts them, so whoever is wired to the one is wired to the other."""
        P, lib = self.P, pb.lib
        B, H, W = x_in.B, x_in.H, x_in.W
        n = self.skip_count()
        shallow = cached is not None
        if depth and not 1 <= depth <= n - 1:
            raise L.PPError(f"DeepCache: cache_branch_id {depth - 1} is outside 0..{n - 2} of this {self.kind} ({n} skip tensors)")
        if shallow and not depth:
            raise L.PPError("build_step(cached=...) is the shallow form of a depth > 0 walk")
        if depth and ((tome and tome.get("layout")) or pag is not None):
            raise L.PPError("DeepCache together with token merging (ToMe) or perturbed-attention guidance (PAG) is not implemented")
        first_up = n - 1 - depth if depth else 0      # index of the first up layer the shallow form runs
        walk = {"down": ["conv_in"], "up": [], "cache": None}
        if pag is not None:
            known = [p for p, _ in self._attn_specs()]
            if self.kind != "unet":
                raise L.PPError("perturbed-attention guidance perturbs the UNet only, never BrushNet or ControlNet")
            if not 0 < pag.n < B or not pag.layers or any(p not in known for p in pag.layers):
                raise L.PPError(f"perturbed-attention guidance: {pag.n} perturbed items of a batch of {B} in {list(pag.layers)} "
                                f"is no setting of this network")
            if tome and tome.get("layout"):
                raise L.PPError("token merging (ToMe) together with perturbed-attention guidance (PAG) is not implemented")
        self._pag_step = pag
        boc = self.boc
        # token merging (NetRuntime._build): layout (tome_layout), the window table (pointer, row stride, rows), the cell that
        # holds the pointer to the device word naming the row, per block the persistent (best_dst, score, pos) buffers, and
        # (filled in here) the batch each block runs on
        self._tome_step = tome
        if self.hypertile is not None and tome and tome.get("layout"):
            raise L.PPError("HyperTile together with token merging (ToMe) on the same network is not implemented")
        self._ht_step = self.hypertile_layout(H, W) or None
        brush = add_down is not None
        add_down = list(add_down) if brush else None
        add_up = list(add_up) if brush else None
        # (a forced tile / split-K factor -- NetRuntime.gemm_tile / gemm_splitk, a measurement knob -- may send conv_in off
        #  the single-pass staged epilogue that stores the twin copy: the flag then changes nothing, as everywhere it cannot run)
        # (IP-Adapters: the prefix ends in the fused cross-attention block, which is not taken while one is loaded)
        # (perturbed-attention guidance: the batch is no pair of identical halves)
        twin = bool(twin) and not pad_uncond and not self.ip and pag is None and not (pb.gemm_tile or pb.gemm_splitk) and \
            self.twin_prefix_ok(lib, B, H, W, self._nctx, brush)

        def pop(lst):
            return lst.pop(0) if lst is not None else 0

        # 1. time embedding (identical for every batch row: timesteps.expand(B))
        tsin = pb.alloc(boc[0] * 4)
        t1 = pb.alloc(boc[0] * 4 * 4)
        temb = pb.alloc(boc[0] * 4 * 4)
        temb_all = pb.alloc(self.temb_total * 4)
        te = boc[0] * 4
        pb.plan.add("timestep_embedding", lib.pp_timestep_embedding, t_dev, 1, boc[0], tsin)
        pb.plan.add("linear_skinny", lib.pp_linear_skinny, tsin, 1, boc[0], P["time_embedding.linear_1.weight"],
                    b1_eff or P["time_embedding.linear_1.bias"], te, t1, te, 0, L.PP_ACT_SILU, pb.dt)
        pb.plan.add("linear_skinny", lib.pp_linear_skinny, t1, 1, te, P["time_embedding.linear_2.weight"],
                    P["time_embedding.linear_2.bias"], te, temb, te, 0, 0, pb.dt)
        pb.plan.add("linear_skinny", lib.pp_linear_skinny, temb, 1, te, P["temb_all.weight"], P["temb_all.bias"],
                    self.temb_total, temb_all, self.temb_total, L.PP_ACT_SILU, 0, pb.dt)
        pb.taps.append(("temb_all", TapF32(temb_all, (self.temb_total,))))

        # 2. conv_in: the implicit-GEMM conv over the zero-padded input (4 / 9 real channels in one 64-deep K chunk per
        # tap: 6x the algorithmic MACs, still 4x faster than the scalar direct conv at 64x64 -- 9 short K steps on the
        # matrix cores -- and its epilogue carries the GroupNorm statistics of resnets.0.norm1 and the side-branch add)
        if x_in.C != self.cin_pad:
            raise L.PPError(f"network input buffer has {x_in.C} channels, conv_in expects {self.cin_pad} (zero-padded)")

        def conv_in(add_ptr) -> Act:
            x = Act(x_in.ptr, B // 2, H, W, x_in.C) if twin else x_in
            o = pb.conv3x3(x, P["conv_in.weight"], boc[0], P["conv_in.bias"], res2=add_ptr or 0, name="conv3x3", dup=twin)
            pb.plan.count("conv3x3", -2.0 * x.B * H * W * boc[0] * 9 * (x_in.C - self.cin0))   # (count the real MACs)
            return o

        if freeu and self.kind != "unet":
            raise L.PPError("FreeU is a feature of the UNet's up blocks (the side networks have no such method)")
        if self.kind == "controlnet":
            s = conv_in(self.cond_emb.ptr)
            skips = [s]
            pb.taps.append(("conv_in", s))
        else:
            s = conv_in(None)
            skips = [s]                       # captured BEFORE the BrushNet add (unet_2d_condition.py:1220-1223)
            pb.taps.append(("conv_in", s))
            if brush:
                s = conv_in(pop(add_down))
                pb.taps.append(("conv_in.add_sample", s))
        if twin:                              # the half the prefix goes on with (skips[0] stays the full, twice-stored tensor)
            s = Act(s.ptr, B // 2, s.H, s.W, s.C, producer=s.producer)

        # 3. down
        for i, typ in enumerate(self.down_types):
            for j in range(self.L):
                if shallow and len(skips) > depth:        # (the shallow form: S[k] is made, nothing below it runs)
                    break
                pre = f"down_blocks.{i}.resnets.{j}"
                has_attn = typ == "CrossAttnDownBlock2D"
                r2 = pop(add_down)
                s = self._resnet(pb, pre, s, boc[i], temb_all, res2=0 if has_attn else r2)
                if has_attn:
                    ap = f"down_blocks.{i}.attentions.{j}"
                    s = self._transformer(pb, ap, s, self.kv[ap], res2=r2, twin=twin and i == 0 and j == 0)
                skips.append(s)
                walk["down"].append(pre)
            if i != len(boc) - 1 and not (shallow and len(skips) > depth):
                pre = f"down_blocks.{i}.downsamplers.0.conv"
                s = pb.conv3x3(s, P[pre + ".weight"], boc[i], P[pre + ".bias"], stride=2, res2=pop(add_down),
                               name="conv3x3")
                skips.append(s)
                pb.taps.append((f"down_blocks.{i}.downsamplers.0", s))
                walk["down"].append(f"down_blocks.{i}.downsamplers.0")

        # 4. mid
        if not shallow:
            s = self._resnet(pb, "mid_block.resnets.0", s, boc[-1], temb_all)
            s = self._transformer(pb, "mid_block.attentions.0", s, self.kv["mid_block.attentions.0"])
            mid_res = add_mid if brush else (ctrl_mid if ctrl_down is not None else 0)
            s = self._resnet(pb, "mid_block.resnets.1", s, boc[-1], temb_all, res2=mid_res)
        prev_name = "mid_block"               # the module whose output the next up layer takes (names the cache point)

        def zero_convs(feats: List[Optional[Act]]) -> List[Act]:
            """One zero conv per tensor of `feats`, in _zero_conv_specs order.  Shallow form: a position that is not live holds
            None and gets no launch; the live ones write the full form's output tensors (`cached`)."""
            specs = self._zero_conv_specs()
            mult = 2 if pad_uncond else 1
            if shallow:
                outs = list(cached["down"]) + [cached["mid"]] + list(cached.get("up", []))
                pb.plan.zero_conv_pos = [p for p, f in enumerate(feats) if f is not None]
            else:
                outs = [pb.new_act(mult * f.B, f.H, f.W, c) for (_, c), f in zip(specs, feats)]
            if pad_uncond:           # one zeroing launch over every (contiguous) run of padded outputs that gets written
                run = None
                for p, (f, o) in enumerate(zip(list(feats) + [None], outs + [None])):
                    if f is not None:
                        run = (run[0] if run else o.ptr, o.ptr + o.rows * o.C * 2)
                    elif run:
                        pb.plan.add("zero_u64", lib.pp_zero_u64, run[0], (run[1] - run[0] + 7) // 8)
                        run = None
            for (pre, c), f, o in zip(specs, feats, outs):
                if f is None:
                    continue
                pb.linear(f.ptr, f.rows, c, P[pre + ".weight"], c, P[pre + ".bias"], scale=scale,
                          out=o.ptr + (f.rows * c * 2 if pad_uncond else 0), name="zero_conv")
                pb.taps.append((pre, o))
            return outs

        if self.kind == "controlnet":
            pb.plan.walk = walk
            if shallow:              # the zero convs 0..k; no mid residual (the UNet's shallow form does not read it)
                outs = zero_convs(skips + [None] * (n - len(skips)) + [None])
                return {"down": outs[:-1], "mid": outs[-1]}
            outs = zero_convs(skips + [s])
            return {"down": outs[:-1], "mid": outs[-1]}

        if ctrl_down is not None:  # stock-UNet ControlNet residuals on the skip tensors (unet_2d_condition.py:1263-1272)
            new = []
            for sk, cp in zip(skips, ctrl_down):
                o = pb.new_act(sk.B, sk.H, sk.W, sk.C)
                pb.add(sk.ptr, cp, o.ptr, sk.rows * sk.C)
                pb.taps.append((f"skip_add.{len(new)}", o))
                new.append(o)
            skips = new

        brush_down: List[Optional[Act]] = list(skips) + [None] * (n - len(skips))
        brush_mid = None if shallow else s
        brush_up: List[Optional[Act]] = []

        # 5. up
        rev = list(reversed(boc))
        u = 0                                # index of the up layer: U[u] takes S[n-1-u]
        cache_act = None
        for i, typ in enumerate(self.up_types):
            has_attn = typ == "CrossAttnUpBlock2D"
            for j in range(self.L + 1):
                live = not shallow or u >= first_up
                r2 = pop(add_up)
                u += 1
                if not live:                 # (the shallow form: this layer's output is not needed, c lies behind it)
                    brush_up.append(None)
                    prev_name = f"up_blocks.{i}.resnets.{j}"
                    continue
                at_cache = bool(depth) and u - 1 == first_up
                if at_cache:                 # c: what this layer is handed
                    walk["cache"] = prev_name
                    if shallow:
                        c0 = cached["cache"]
                        s = Act(c0.ptr, c0.B, c0.H, c0.W, c0.C)
                    cache_act = s
                sk = skips.pop()
                assert sk.H == s.H and sk.W == s.W, "skip / hidden size mismatch (odd latent size?)"
                if freeu and i < 2:         # (resolution_idx 0 takes (b1, s1), 1 takes (b2, s2); later up blocks are untouched)
                    # (c must survive the launch: the shallow evaluations behind this one read it again)
                    s, sk = pb.freeu(s, sk, freeu + 8 * i, self.groups, h_out=pb.new_act(s.B, s.H, s.W, s.C) if at_cache else None)
                s = self._resnet(pb, f"up_blocks.{i}.resnets.{j}", s, rev[i], temb_all, x2=sk,
                                 res2=0 if has_attn else r2)
                if has_attn:
                    ap = f"up_blocks.{i}.attentions.{j}"
                    s = self._transformer(pb, ap, s, self.kv[ap], res2=r2)
                brush_up.append(s)
                prev_name = f"up_blocks.{i}.resnets.{j}"
                walk["up"].append(prev_name)
            if i != len(boc) - 1 and shallow and u - 1 < first_up:      # the upsampler behind a layer that did not run
                pop(add_up)
                brush_up.append(None)
                prev_name = f"up_blocks.{i}.upsamplers.0"
            elif i != len(boc) - 1:
                walk["up"].append(f"up_blocks.{i}.upsamplers.0")
                prev_name = f"up_blocks.{i}.upsamplers.0"
                pre = f"up_blocks.{i}.upsamplers.0.conv"
                # the upsampler resizes to the size of the skip tensor the next block pops: 2 h or, behind an odd level of the
                # down path, 2 h - 1 per axis (`upsample_size`, unet_2d_condition.py:1311-1312; BrushNet_CA.py:874)
                tgt = (skips[-1].H, skips[-1].W)
                if pre in self.upfold and tgt == (2 * s.H, 2 * s.W):
                    s = pb.conv3x3_up_subpix(s, self.upfold[pre], rev[i], P[pre + ".bias"], res2=pop(add_up))
                else:
                    s = pb.conv3x3(s, P[pre + ".weight"], rev[i], P[pre + ".bias"], up=True, up_size=tgt,
                                   res2=pop(add_up), name="conv3x3")
                pb.taps.append((f"up_blocks.{i}.upsamplers.0", s))
                brush_up.append(s)

        if self.kind == "brushnet":
            outs = zero_convs(brush_down + [brush_mid] + brush_up)
            nd = len(brush_down)
            pb.plan.walk = walk
            return dict({"down": outs[:nd], "mid": outs[nd], "up": outs[nd + 1:]}, **({"cache": cache_act} if depth else {}))

        # 6. out: conv_norm_out + SiLU + conv_out -- one launch when the GroupNorm statistics arrive from the producer's
        # epilogue (the normalised 64x64x320 activation is then never written), else norm launch(es) + conv
        eps = cached["eps"] if shallow else pb.alloc(B * self.out_channels * H * W * 4)
        acc = 0
        if self.fuse_conv_out and lib.pp_gn_conv3x3_smallcout_supported(boc[0], self.out_channels, self.groups):
            acc = pb._subscribe_gn_stats(s, None, self.groups)
        if acc:
            pb.plan.add("conv_out", lib.pp_gn_conv3x3_smallcout, s.ptr, B, H, W, boc[0], self.groups, self.eps,
                        P["conv_norm_out.weight"], P["conv_norm_out.bias"], acc, P["conv_out.weight"],
                        P["conv_out.bias"], self.out_channels, eps, pb.dt)
        else:
            h = pb.groupnorm(s, P["conv_norm_out.weight"], P["conv_norm_out.bias"], self.eps, True, groups=self.groups)
            pb.plan.add("conv_out", lib.pp_conv3x3_smallcout, h.ptr, B, H, W, boc[0], P["conv_out.weight"],
                        P["conv_out.bias"], self.out_channels, eps, pb.dt)
        pb.plan.count("conv_out", 2.0 * B * H * W * self.out_channels * 9 * boc[0])
        pb.taps.append(("eps", TapF32(eps, (B, self.out_channels, H, W))))
        pb.plan.walk = walk
        return dict({"eps": eps}, **({"cache": cache_act} if depth else {}))
