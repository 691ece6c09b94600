"""The HIP execution engine for MobileNetV2UNet / UNet / LightUNet.

A model (seg_amd/unet.py) is compiled once per input shape into a *program*:
a flat list of ops over named NHWC fp32 buffers.  The forward walks the list;
the backward walks it in reverse with mirrored gradient buffers.  The whole
network is one torch.autograd.Function, so `loss.backward()` works exactly as
in the reference loop (src/train.py:36-39) while every FLOP runs in
libsegamd.so (include/segamd.h).

Buffers / layout (DESIGN.md "Data layout in HBM"):
  * every activation is a [pixels][ld] row tensor, ld = round_up(C, 4);
  * the decoder concat `torch.cat([skip, up(x)], 1)` (src/unet.py:103) is a
    single buffer: the encoder writes its skip output into channels [0, Cs),
    the bilinear upsample writes [Cs, Cs+Cu) -- no copy;
  * each conv keeps its raw (pre-BN) output `y` for the BN backward; the
    normalised/activated output is the next op's input.
Gradients of a buffer region are written by the first consumer in reverse
order and accumulated by later ones; a residual (InvertedResidual
`x + conv(x)`) hands its upstream gradient to the first writer of dx as a
fused addend.

Fine-tuning (seg_amd/freeze.py): each BatchNorm layer runs in its own module's mode -- train: batch statistics;
eval: frozen on its running statistics, which it then leaves alone -- and the backward runs only what a parameter
with requires_grad needs: grad_frontier() says per op whether it owes parameter gradients and whether anything
upstream of its input trains.  Both patterns are part of a recorded plan's key (plan_signature).

Backward schedule: one path per decision.  ConvOp.backward is the BatchNorm backward (ConvOp._bn_backward: its four
forms), the residual hand-off, the data gradient on the main stream and then the parameter gradients, whose placement
-- behind a side-stream fork now, or deferred to run beside the encoder's memory-bound backward -- Run.param_grads
alone decides.  A frozen conv runs only its data gradient; an op behind the gradient frontier runs nothing.

Routes: which kernel runs a conv is decided once per program and direction, in one
place.  pick_routes() gives every ConvOp a Route for its forward, data gradient and
weight gradient (op.route_f / route_d / route_w): the kernel family, the resolved C
entry point, the roofline timer kind, the BN-statistics tile geometry, the workspace,
the split count and the packed weight it reads.  The picker is a pure function of the
shapes, the conv math, the engine switches below and the library's host-side queries
(no tensor, no device call; tests/test_engine_routes.py runs it without a GPU).
Program._build_pack allocates the packed weights the routes name, and the walk only
reads routes: ConvOp._launch holds the one argument list per family that the forward
and the data gradient share.  A new kernel is wired in by adding its case to the
picker and, if its argument list is new, to _launch.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
from types import SimpleNamespace
from typing import NamedTuple

import torch
from torch import nn

from ._lib import call, query as _query

# Host-only size / plan queries of the C ABI are pure functions of their integer
# arguments: memoised, so a training step does not pay a ctypes call for each of them.
# (Not the implicit GEMM's tile-dependent queries -- seg_conv_igemm_tiles / _row_tiles / _bnout_ok, igemm2's
# plan: a forced tile (force_igemm_tile) changes them)
_PURE_QUERIES = {"seg_chan_workspace_floats", "seg_conv_wgrad_splits", "seg_conv_wgrad_splits_bf16", "seg_dw_wgrad_blocks",
                 "seg_conv_igemm_splits", "seg_ce_workspace_floats", "seg_conv_wino_row_tiles", "seg_conv_wino_tile_rows",
                 "seg_conv_halo_row_tiles", "seg_conv_wino_wgrad_splits", "seg_conv_wino_wgrad16_splits",
                 "seg_mbconv_ok"}
_QCACHE = {}


def query(name, *args):
    if name not in _PURE_QUERIES:
        return _query(name, *args)
    key = (name, args)
    r = _QCACHE.get(key)
    if r is None:
        r = _QCACHE[key] = _query(name, *args)
    return r
from .mobilenet import ConvBNReLU6, InvertedResidual

ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2
IGNORE_INDEX = -100
_ROW_TILES = {}  # (M, Cout) -> (row tiles, tile height) of seg_conv_igemm


_IG2 = {}  # (M, Cout, Cin, ks) -> (tile rows, row tiles, splits, workspace floats) or None
_TILE_GEN = 0  # bumped by force_tiles; part of Program.pack's key, so the next walk picks every route again


class Route(NamedTuple):
    """How one direction of one conv runs (pick_routes); immutable, holds no tensor."""
    family: str                  # pw | halo | wino | wino_fused | igemm2 | igemm | dw; weight gradients: dw | wino |
                                 # wino16 | wgrad2 | igemm
    name: str                    # C entry point, storage / math / weight-format suffixes applied
    timer: str | None            # roofline timer kind (bench.py selects on these); None: an untimed launch
    mode: int | None = None      # packed weight it reads: seg_pack_job layout (0 forward, 1 data gradient, 2 depthwise,
                                 # 3 / 4 their Winograd U; | 16 = bf16), None = no pack of its own (a 1x1 conv's
                                 # weight as it is; the depthwise data gradient reads the forward's)
    ldk: int = 0                 # ... and its row stride
    tiles: tuple | None = None   # forward into a BatchNorm: (row tiles, rows per tile) of the statistics partials
    work: int = 0                # workspace floats
    zero: bool = False           # ... zero-filled before the launch
    splits: int = 0              # weight gradient: split-K slabs / blocks of partials the reduce sums
    bnout: str | None = None     # implicit-GEMM data gradient: its entry point that also emits BN-backward partials
    fallback: "Route | None" = None  # data gradient: the route when the addend is not 16-byte aligned at walk time


def _pw_pick(op, v: int):
    """(forward, data gradient) of a 1x1 conv on the thin-K kernel (seg_conv_pw): K <= 32 with
    K % 8 == 0, N <= 192, rows in 16-byte vectors of v elements."""
    if not PW or op.kind != "igemm" or op.ks != 1 or op.stride != 1:
        return False, False
    i, y = op.inp, op.y
    # measured per launch (bf16io, tools/tapeprof.py): 1.2-1.8x faster than the implicit GEMM on the
    # full- and half-resolution layers, 5-20 % slower on the 65k-row ones (one tile per block)
    if y.M < PW_MIN_ROWS:
        return False, False
    rows = lambda *ts: all(t.ld % v == 0 and t.off % v == 0 for t in ts)  # noqa: E731
    fwd = 8 <= op.cin_pad <= 32 and op.cin_pad % 8 == 0 and op.cout <= 192 and rows(i, y)
    kin = r4(op.cout)
    bwd = not op.first and 8 <= kin <= 32 and kin % 8 == 0 and op.cin <= 192 and rows(i) and kin % v == 0
    return fwd, bwd


def igemm2_plan(M: int, cout: int, cin: int, ks: int):
    """seg_conv_igemm2_plan (memoised): None when the deep-conv kernel does not apply."""
    key = (M, cout, cin, ks)
    if key not in _IG2:
        out = (ctypes.c_long * 4)()
        ok = query("seg_conv_igemm2_plan", M, cout, cin, ks, ctypes.addressof(out))
        _IG2[key] = tuple(out) if ok else None
    return _IG2[key]


def force_tiles(igemm: int | None = None, igemm2: int | None = None) -> None:
    """Tuning hook: force the implicit GEMM's (seg_igemm_force_tile) and / or igemm2's (seg_igemm2_force_tile) tile
    table entry (-1 = the cost model again), and drop every memoised tile-dependent plan (row tiles, igemm2 plans) and
    every program's routes, so the next program walk picks and sizes its workspaces for the tile actually launched
    (ADVICE r4).  Plans recorded before the change keep their tapes: release_plans() / a fresh Predictor re-record
    them."""
    global _TILE_GEN
    _TILE_GEN += 1
    if igemm is not None:
        _query("seg_igemm_force_tile", int(igemm))
    if igemm2 is not None:
        _query("seg_igemm2_force_tile", int(igemm2))
    _ROW_TILES.clear()
    _IG2.clear()
    _QCACHE.clear()


def r8(c: int) -> int:
    return (c + 7) & ~7


def r4(c: int) -> int:
    return (c + 3) & ~3


class KernelTimer:
    """Opt-in HIP-event timing of the dense MFMA convolution launches (used by
    bench.py for the roofline figure).  Each timed launch is bracketed by two
    events on the stream it runs on (torch's current stream)."""

    def __init__(self, kinds=None, max_replays=64):
        self.records = []  # (kind, flops, start_event, end_event) of immediate launches
        # only these launch kinds are bracketed (None: all): every event pair is a marker
        # packet on the queue, ~3 % of the step when all ~130 conv launches are timed
        self.kinds = kinds
        # launch tapes armed for this timer (Plan._arm_timer): each times its selected
        # entries over up to max_replays replays with events inside libsegamd
        self.tapes = []
        self.max_replays = max_replays

        self.collected = []

    def collect(self, tape):
        """Move a tape's timings into this timer (the tape is being re-armed)."""
        if tape in self.tapes:
            torch.cuda.synchronize()
            self.collected += tape.elapsed()
            self.tapes.remove(tape)

    def elapsed(self):
        """[(kind, flops, seconds)] -- call after synchronising."""
        out = [(k, f, a.elapsed_time(b) * 1e-3) for k, f, a, b in self.records] + self.collected
        for t in self.tapes:
            out += t.elapsed()
        return out


TIMER: KernelTimer | None = None

def _stat_ptrs(st, C):
    """Device pointers of the mean / invstd / scale / shift rows of a saved [4][C] BN
    statistics tensor (no per-call view tensors on the host path)."""
    b = st.data_ptr()
    return b, b + 4 * C, b + 8 * C, b + 12 * C


def _timed_call(kind, flops, name, *args):
    if TIMER is None or (TIMER.kinds is not None and kind not in TIMER.kinds):
        return call(name, *args)
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    call(name, *args)
    b.record()
    TIMER.records.append((kind, flops, a, b))


class Act:
    """NHWC view: channels [off, off+C) of buffer `buf` ([N*H*W][ld])."""
    __slots__ = ("buf", "off", "ld", "C", "N", "H", "W")

    def __init__(self, buf, off, ld, C, N, H, W):
        self.buf, self.off, self.ld, self.C, self.N, self.H, self.W = buf, off, ld, C, N, H, W

    @property
    def M(self):
        return self.N * self.H * self.W

    def key(self):
        return (self.buf, self.off, self.C)

    def slice(self, off, C):
        return Act(self.buf, self.off + off, self.ld, C, self.N, self.H, self.W)


# ----------------------------------------------------------------------------- ops

IMAGE = "image"   # buffer holding the NHWC4 copy of the NCHW model input


class ConvOp:
    """conv (igemm | dw) -> [BN -> act (+residual)]."""

    def __init__(self, kind, conv: nn.Conv2d, bn, act, inp, out, y, res, xform=None):
        self.kind, self.conv, self.bn, self.act = kind, conv, bn, act
        self.inp, self.out, self.y, self.res = inp, out, y, res
        # lazy BN: this op's BN + act is applied by its (only) consumer on load, out is y;
        # xform: the producer op whose BN + act this op applies to its input on load
        self.lazy = False
        self.xform = xform
        # forward / data gradient (None: the first conv) / weight gradient Route (pick_routes) and the packed
        # weights the first two read (Program._build_pack, in the Route's layout; None: its mode is None)
        self.route_f = self.route_d = self.route_w = None
        self.wk_f = self.wk_d = None
        # BN-folded inference weights (Program.fold): fk [Cout][Cin/g][ks][ks], fb [r4(Cout)], fk_pack [Cout][ldk_f]
        self.fk = self.fb = self.fk_pack = None
        self.ldk_f = 0
        self.ks = conv.kernel_size[0]
        self.stride = conv.stride[0]
        self.pad = conv.padding[0]
        self.cin = conv.in_channels
        self.cin_pad = r4(self.cin)  # GEMM K runs are float4 channel groups (the image: 3 -> 4)
        self.cout = conv.out_channels
        self.first = inp.buf == IMAGE  # no data gradient for the model input

    def flops(self) -> int:
        """Algorithmic FLOPs of this conv's forward (2 * MACs; dgrad and wgrad each equal it)."""
        groups = self.conv.groups
        return 2 * self.y.M * self.cout * (self.cin // groups) * self.ks * self.ks

    def params(self):
        ps = [self.conv.weight]
        if self.conv.bias is not None:
            ps.append(self.conv.bias)
        if self.bn is not None:
            ps += [self.bn.weight, self.bn.bias]
        return ps

    def _launch(self, rt, r, sp, sld, g, K, wk, dp, o, C, bias, addp, add_ld, statp, xf, stride, s):
        """Route `r` of a dense conv: rows of src (pointer sp, row stride sld, image geometry g, K channels) x packed
        weight -> rows of dst (pointer dp, geometry o, C channels) (+ bias) (+ addend) (+ BN statistics partials).  The
        argument list of every kernel family, once: the forward calls it with x -> y, the data gradient with dY -> dx
        (the transposed conv on the data-gradient pack).  xf: the (scale, shift, act) of a lazy producer BN, or None."""
        wp = wk.data_ptr() if r.mode is not None else self.conv.weight.data_ptr()  # [Cout][Cin][1][1] is a pack already
        head = (sp, sld, g.N, g.H, g.W, K, wp, r.ldk, bias, dp, o.ld)
        work = rt.tmp(r.work, zero=r.zero) if r.family in ("wino", "igemm2") else None
        if r.family == "pw":  # thin-K 1x1 (its producer's lazy BN, if any, on load)
            args = (sp, sld, g.M, K, wp, r.ldk, bias, dp, o.ld, C, addp, add_ld, statp, *(xf or (None, None, 0)))
        elif r.family in ("halo", "wino_fused"):
            args = (*head, C, addp, add_ld, statp)
        elif r.family == "wino":  # 16 GEMMs + output transform through the M workspace
            args = (*head, C, addp, add_ld, statp, work.data_ptr())
        elif r.family == "igemm2":  # bf16io LDS-DMA implicit GEMM (deep 3x3 convs); split-K through the workspace
            args = (*head, C, self.ks, addp, add_ld, statp, work.data_ptr())
        else:  # the implicit GEMM; seg_conv_igemm_bf16 is also the folded forward's: + act, residual, its row stride
            args = (*head, o.H, o.W, C, self.ks, stride, self.pad, addp, add_ld, statp, *(xf or ()),
                    *((ACT_NONE, None, 1) if r.name == "seg_conv_igemm_bf16" else ()))
        rt.tcall(r.timer, self.flops(), r.name, *args, s)

    # -- forward
    def forward(self, rt):
        s, y, i, r = rt.stream, self.y, self.inp, self.route_f
        stat = None
        # this layer's BatchNorm mode, read once per recorded plan (its signature is part of the plan's key): batch
        # statistics, or frozen on the running ones (seg_amd.freeze, model.eval())
        train = rt.bn_train[id(self)] = self.bn is not None and self.bn.training
        if self.kind == "dw":
            rt.call(r.name, rt.ptr(i), i.ld, i.N, i.H, i.W, i.C, *self._in_xform(rt),
                    self.wk_f.data_ptr(), rt.ptr(y), y.ld, y.H, y.W, self.stride, s)
        else:
            if train:  # BN statistics fused into the conv epilogue, one row per tile (r.tiles)
                stat = rt.tmp(r.tiles[0] * 2 * self.cout)
            self._launch(rt, r, rt.ptr(i), i.ld, i, self.cin_pad, self.wk_f, rt.ptr(y), y, self.cout,
                         self.conv.bias.data_ptr() if self.conv.bias is not None else None, None, 0,
                         stat.data_ptr() if stat is not None else None,
                         self._in_xform(rt) if self.xform is not None else None, self.stride, s)
        if self.bn is not None:
            self._bn_forward(rt, train, stat)

    def _bn_forward(self, rt, train, stat):
        """This op's BatchNorm after its conv: the [4][C] mean / invstd / scale / shift of the batch (train; `stat`:
        the conv epilogue's tile partials, None after a depthwise conv) or of the running statistics, saved for the
        backward, then BN + act (+ residual) y -> out unless the consumer applies them on load (lazy)."""
        s, y = rt.stream, self.y
        bn, C, M = self.bn, self.cout, y.M
        st = torch.empty(4 * C, device=rt.device, dtype=torch.float32)
        mean, invstd, scale, shift = _stat_ptrs(st, C)
        if train:
            if bn.momentum is None:
                raise NotImplementedError("BatchNorm2d(momentum=None) (cumulative average) is not supported")
            rm = bn.running_mean.data_ptr() if bn.track_running_stats else None
            rv = bn.running_var.data_ptr() if bn.track_running_stats else None
            nbt = bn.num_batches_tracked.data_ptr() if bn.track_running_stats else None
            if stat is None:
                work = rt.tmp(query("seg_chan_workspace_floats", M, C))
                rt.call(rt.k("seg_bn_stats"), rt.ptr(y), y.ld, M, C, bn.weight.data_ptr(), bn.bias.data_ptr(), bn.eps,
                     bn.momentum, rm, rv, nbt, work.data_ptr(), mean, invstd,
                     scale, shift, s)
            else:
                # many-tile layers (a non-zero workspace size): 16 tiles merged per row before the per-channel finalize
                ntiles, tile_rows = self.route_f.tiles
                nw = query("seg_bn_stats_tiles_work_floats", ntiles, C)
                ws = (rt.tmp(nw).data_ptr(),) if nw else ()
                rt.call("seg_bn_stats_tiles_ws" if nw else "seg_bn_stats_tiles", stat.data_ptr(), ntiles, tile_rows, M,
                        C, bn.weight.data_ptr(), bn.bias.data_ptr(), bn.eps, bn.momentum, rm, rv, nbt, mean, invstd,
                        scale, shift, *ws, s)
        else:
            if bn.running_mean is None:
                raise NotImplementedError("eval-mode BatchNorm2d without running statistics")
            rt.call("seg_bn_eval_coef", bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                 bn.running_var.data_ptr(), bn.eps, C, scale, shift, s)
        rt.saved[id(self)] = st
        if self.lazy:
            return
        o, r = self.out, self.res
        rt.call(rt.k("seg_bn_apply"), rt.ptr(y), y.ld, M, C, scale, shift, self.act,
             rt.ptr(r) if r is not None else None, r.ld if r is not None else 0, rt.ptr(o), o.ld, s)

    # -- inference (BatchNorm folded into the conv: Program.fold)
    def forward_folded(self, rt):
        """act(conv(x, W') + b') (+ residual) in one launch; W', b' from seg_bn_fold_batch.
        A lazy producer writes its activated output into its `y` buffer (= `out`), so its
        depthwise consumer reads it without the on-load BN transform."""
        s, i, o = rt.stream, self.inp, self.out
        act = self.act if self.bn is not None else ACT_NONE
        if self.kind == "dw":
            rt.call("seg_dw_fwd_bias_act", rt.ptr(i), i.ld, i.N, i.H, i.W, i.C, self.fk_pack.data_ptr(),
                 self.fb.data_ptr(), act, rt.ptr(o), o.ld, o.H, o.W, self.stride, s)
            return
        if self.fk_pack is None:
            ldk, wk = self.cin, self.fk.data_ptr()
        else:
            ldk, wk = self.ldk_f, self.fk_pack.data_ptr()
        r = self.res
        bias = self.fb.data_ptr() if self.fb is not None else None
        M = o.N * o.H * o.W
        # (splits, tile, output tiles) of seg_conv_igemm_plan_b1; split-K combined inside the launch
        # (seg_conv_igemm_*_ic); workspace and tile counters persistent across graph replays (allocated by the
        # warm-up launch, before any capture)
        bufs = rt._mb.get(("ic", id(self)))
        if bufs is None:
            plan = (ctypes.c_int * 3)()
            query("seg_conv_igemm_plan_b1", M, self.cout, self.cin_pad, self.ks, ctypes.addressof(plan))
            splits, tile, ntl = plan
            bufs = rt._mb[("ic", id(self))] = (
                torch.empty(splits * M * self.cout if splits > 1 else 1, device=rt.device, dtype=torch.float32),
                torch.zeros(4 * ntl, device=rt.device, dtype=torch.int32), splits, tile)
        work, cnt, splits, tile = bufs
        rt.call(_FOLDED_CONV[rt.prog.math] + "_ic", rt.ptr(i), i.ld, i.N, i.H, i.W, self.cin_pad, wk, ldk, bias,
                rt.ptr(o), o.ld, o.H, o.W, self.cout, self.ks, self.stride, self.pad,
                rt.ptr(r) if r is not None else None, r.ld if r is not None else 0, act, work.data_ptr(), splits, tile,
                cnt.data_ptr(), s)

    def _in_xform(self, rt):
        """(scale, shift, act) of the producer's lazy BN for this op's input loads, or (None, None, 0)."""
        xf = self.xform
        if xf is None:
            return None, None, 0
        st, C = rt.saved[id(xf)], xf.cout
        return st[2 * C:3 * C].data_ptr(), st[3 * C:4 * C].data_ptr(), xf.act

    # -- backward
    def _bnout(self, rt, i):
        """BN-backward partials from this data gradient's epilogue (seg_conv_igemm_bnout*), when its output
        region is exactly the output of a train-mode BatchNorm layer P: the extra arguments, or None.  P's
        backward uses them if no other write reached the buffer afterwards (Run.wgen)."""
        if not BNOUT:
            return None
        p = rt.prog.bn_owner().get(i.key())
        if p is None or id(p) not in rt.saved or not rt.bn_train[id(p)]:  # frozen statistics: no reduction to feed
            return None
        v = 16 // rt.es
        py = p.y
        if py.ld % v or py.off % v or rt.ptr(py) % 16:
            return None
        if not query("seg_conv_igemm_bnout_ok", i.M, self.cin, int(rt.io)):
            return None
        tiles, _ = rt.row_tiles(i.M, self.cin)
        if tiles > BNOUT_MAX_TILES:
            return None
        C = p.cout
        mean, invstd, scale, shift = _stat_ptrs(rt.saved[id(p)], C)
        part = rt.tmp(tiles * 2 * C)
        rt.bn_parts[id(p)] = [part, tiles, None]
        return (rt.ptr(py), py.ld, scale, shift, mean, p.act, part.data_ptr()), p

    def backward(self, rt):
        s = rt.stream
        # grad_frontier: does anything upstream of the input / of the residual want this op's data gradient
        _, dgrad, rgrad = rt.need[rt.cur_op]
        dgrad = dgrad and not self.first
        cw, cb = self.conv.weight, self.conv.bias
        conv_grads = cw.requires_grad or (cb is not None and cb.requires_grad)
        dA = rt.grad_of(self.out)
        if self.bn is not None:
            dY = self._bn_backward(rt, dA, dgrad or conv_grads)  # None: only the affine gradients (nothing reads dY)
            if self.res is not None and rgrad:
                rt.add_pending(self.res, dA)
            if dY is None:  # a frozen conv under a trainable BatchNorm affine pair, nothing trainable upstream
                rt.params_done(self.params(), s)
                return
        else:
            dY = dA
        dYp = rt.ptr(dY) if dY.buf.startswith("#") else rt.gptr(dY)
        if not conv_grads:  # a frozen conv: no side-stream work, only what is upstream of it
            rt.params_done(self.params(), s)
            if dgrad:
                self._dgrad(rt, dY, dYp, s)
            return
        # parameter gradients: on the side stream when overlapping (they only read dY and x,
        # and nothing on the main stream's data-gradient chain waits for them)
        # gradient tensors handed back to autograd are allocated on the main stream
        # (they outlive the backward; the side stream only writes into them)
        for p in (cw, cb):
            if p is not None and p.requires_grad:
                rt.grad_param(p)
        if dgrad:  # the data gradient first: the side stream's weight gradient then runs beside
            self._dgrad(rt, dY, dYp, s)  # the next layer's memory-bound BN backward, not this dgrad
        rt.param_grads(self, dY, dYp)

    def _bn_backward(self, rt, dA, want_dy):
        """This op's BatchNorm + act backward: the affine gradients the layer owes and, if want_dy, dY (the gradient
        of the conv's raw output y, in a buffer of its own) from dA; returns dY or None.  Four forms: frozen
        statistics, the reduction alone, finalize + apply on a data gradient's tile partials (ConvOp._bnout), and
        the fused reduction + apply."""
        s, y, bn = rt.stream, self.y, self.bn
        C, M = self.cout, y.M
        mean, invstd, scale, shift = _stat_ptrs(rt.saved[id(self)], C)
        g_w = rt.grad_param(bn.weight) if bn.weight.requires_grad else None
        g_b = rt.grad_param(bn.bias) if bn.bias.requires_grad else None
        # bench.py's "bn_bwd" family: algorithmic bytes of a BatchNorm backward = dA and y read once, dY written
        # once (3 |Y|), credited to the launch that writes dY
        abytes = 3 * M * C * rt.es
        bp = rt.bn_parts.pop(id(self), None)
        dY = Act(rt.tmp_buf(M * r4(C)), 0, r4(C), C, y.N, y.H, y.W) if want_dy else None
        if not rt.bn_train[id(self)]:
            # frozen statistics: one pass (seg_bn_frozen_backward), no reduction at all with a frozen affine pair
            red = g_w is not None or g_b is not None
            if red or want_dy:
                work = rt.tmp(query("seg_chan_workspace_floats", M, C)) if red else None
                rt.tcall("bn_bwd", abytes if want_dy else 0, rt.k("seg_bn_frozen_backward"), rt.gptr(dA), dA.ld,
                         rt.ptr(y), y.ld, M, C, scale, shift, bn.running_mean.data_ptr(),
                         bn.running_var.data_ptr(), bn.eps, self.act, g_w, g_b,
                         work.data_ptr() if red else None, rt.ptr(dY) if want_dy else None,
                         dY.ld if want_dy else 0, s)
        elif not want_dy:
            if g_w is not None or g_b is not None:  # the reduction half alone
                work = rt.tmp(query("seg_chan_workspace_floats", M, C) + 3 * C)
                rt.call(rt.k("seg_bn_bwd_coef"), rt.gptr(dA), dA.ld, rt.ptr(y), y.ld, M, C, bn.weight.data_ptr(),
                        mean, invstd, scale, shift, self.act, g_w, g_b, work.data_ptr(),
                        work.data_ptr() + 4 * query("seg_chan_workspace_floats", M, C), s)
        elif bp is not None and bp[2] == rt.wgen.get(self.out.buf):
            # the reduction's partials came out of the epilogue of the data gradient that completed dA (nothing
            # wrote the buffer since): finalize them, then the apply
            coef = rt.tmp(3 * C)
            rt.tcall("bn_bwd", 0, "seg_bn_bwd_finalize_tiles", bp[0].data_ptr(), bp[1], M, C,
                     bn.weight.data_ptr(), invstd, g_w, g_b, coef.data_ptr(), s)
            rt.tcall("bn_bwd", abytes, rt.k("seg_bn_bwd_apply"), rt.gptr(dA), dA.ld, rt.ptr(y), y.ld, M, C, mean,
                     scale, shift, self.act, coef.data_ptr(), rt.ptr(dY), dY.ld, s)
        else:
            work = rt.tmp(query("seg_chan_workspace_floats", M, C) + 3 * C)
            rt.tcall("bn_bwd", abytes, rt.k("seg_bn_backward"), rt.gptr(dA), dA.ld, rt.ptr(y), y.ld, M, C,
                     bn.weight.data_ptr(), mean, invstd, scale, shift, self.act,
                     g_w, g_b, work.data_ptr(), rt.ptr(dY), dY.ld, s)
        return dY

    def _param_grads(self, rt, dY, dYp, s):
        """Bias gradient (column sum of dY), weight gradient (split-K slabs + fixed-order
        reduce) and the DDP readiness hook, all on stream `s`."""
        y, M = self.y, self.y.M
        if self.conv.bias is not None and self.conv.bias.requires_grad:
            if self.bn is not None and ZERO_BN_BIAS and rt.bn_train[id(self)]:
                # conv -> train-mode BatchNorm (src/unet.py:58-59,61-62): the bias shifts its whole channel by
                # a constant that the batch mean removes again, so d loss / d bias = sum_p dY[p][c] = 0
                # exactly (the reference computes that sum and gets fp32 rounding noise, ~1e-9 relative)
                rt.zero_param_grad(self.conv.bias, s)
            else:
                work = rt.tmp(query("seg_chan_workspace_floats", M, r4(self.cout)))
                rt.call(rt.k("seg_colsum"), dYp, dY.ld, M, self.cout, work.data_ptr(), rt.grad_param(self.conv.bias),
                        0, s)
        if self.conv.weight.requires_grad:
            gw = rt.grad_param(self.conv.weight)
            i, r = self.inp, self.route_w
            slabs = rt.tmp(r.work)  # r.splits slabs of partial sums, summed in a fixed order by the reduce
            part = slabs.data_ptr()
            if r.family == "dw":
                rt.call(r.name, dYp, dY.ld, rt.ptr(i), i.ld, i.N, i.H, i.W, i.C, *self._in_xform(rt), y.H, y.W,
                        self.stride, part, s)
                rt.call("seg_conv_wgrad_reduce", part, r.splits, gw, self.cout, 1, 3, 1, 0, s)
            elif r.family == "igemm":  # with a lazy producer (_xf): X = its BN + act, formed on load
                rt.tcall(r.timer, self.flops(), r.name, dYp, dY.ld, rt.ptr(i), i.ld, i.N, i.H, i.W, self.cin_pad, y.H,
                         y.W, self.cout, self.ks, self.stride, self.pad, part, r.splits,
                         *(self._in_xform(rt) if self.xform is not None else ()), s)
                rt.call("seg_conv_wgrad_reduce", part, r.splits, gw, self.cout, self.cin, self.ks, 0, 0, s)
            else:  # 3x3: Winograd F(3x3,2x2) (wino, wino16) / the persistent LDS-halo kernel, one slab per block
                rt.tcall(r.timer, self.flops(), r.name, dYp, dY.ld, rt.ptr(i), i.ld, y.N, y.H, y.W, self.cin_pad,
                         self.cout, part, *(() if r.family == "wgrad2" else (r.splits,)), s)
                if r.family == "wgrad2":
                    rt.call("seg_conv_wgrad_reduce", part, r.splits, gw, self.cout, self.cin, 3, 0, 0, s)
                else:
                    rt.call("seg_conv_wino_wgrad_reduce", part, r.splits, gw, self.cout, self.cin, self.cin_pad, 0, s)
        rt.params_done(self.params(), s)

    def _dgrad(self, rt, dY, dYp, s):
        """Data gradient into the input's gradient region (first writer / fused addend)."""
        y, i = self.y, self.inp
        if self.kind == "dw":
            acc = rt.begin_write_accumulate(i)
            rt.call(self.route_d.name, dYp, dY.ld, y.N, y.H, y.W, self.cout, self.wk_f.data_ptr(), rt.gptr(i),
                    i.ld, i.H, i.W, self.stride, acc, s)
        else:
            if self.stride != 1:
                raise NotImplementedError("data gradient of a strided dense conv")
            kin = r4(self.cout)  # dY channels padded to 4 (the C=10 head)
            add_ptr, add_ld = rt.begin_write_add(i)
            r = self.route_d
            # seg_conv_pw / seg_conv_igemm2 read the addend as 16-byte row vectors: else the implicit GEMM
            if r.fallback is not None and add_ptr is not None and (add_ld % (16 // rt.es) or add_ptr % 16):
                r = r.fallback
            bo = self._bnout(rt, i) if r.bnout is not None else None
            if bo is None:
                self._launch(rt, r, dYp, dY.ld, y, kin, self.wk_d, rt.gptr(i), i, self.cin, None, add_ptr, add_ld,
                             None, None, 1, s)
            else:  # + the BN-backward partials of the layer whose dA this completes
                rt.tcall(r.timer, self.flops(), r.bnout, dYp, dY.ld, y.N, y.H, y.W, kin, self.wk_d.data_ptr(), r.ldk,
                         rt.gptr(i), i.ld, self.cin, self.ks, add_ptr, add_ld, *bo[0], s)
                rt.mark_written(i)  # the partials are valid while this write is the buffer's last
                rt.bn_parts[id(bo[1])][2] = rt.wgen[i.buf]
                return
        rt.mark_written(i)


class UpsampleOp:
    """nn.Upsample(x2, bilinear, align_corners=False) into a concat slice (src/unet.py:97-103)."""

    def __init__(self, low, out):
        self.low, self.out = low, out

    def params(self):
        return []

    def forward(self, rt):
        l, o = self.low, self.out
        rt.call(rt.k("seg_upsample_fwd"), rt.ptr(l), l.ld, l.N, l.H, l.W, l.C, rt.ptr(o), o.ld, o.H, o.W, 0, rt.stream)

    def backward(self, rt):
        l, o = self.low, self.out
        d = rt.grad_of(o)
        acc = rt.begin_write_accumulate(l)
        rt.call(rt.k("seg_upsample_bwd"), rt.gptr(d), d.ld, 0, o.N, o.H, o.W, o.C, rt.gptr(l), l.ld, l.H, l.W, 0, acc,
             rt.stream)
        rt.mark_written(l)


class PoolOp:
    """nn.MaxPool2d(2) (src/unet.py:85)."""

    def __init__(self, inp, out):
        self.inp, self.out = inp, out

    def params(self):
        return []

    def forward(self, rt):
        i, o = self.inp, self.out
        rt.call(rt.k("seg_maxpool2_fwd"), rt.ptr(i), i.ld, i.N, i.H, i.W, i.C, rt.ptr(o), o.ld, rt.stream)

    def backward(self, rt):
        i, o = self.inp, self.out
        d = rt.grad_of(o)
        acc = rt.begin_write_accumulate(i)
        rt.call(rt.k("seg_maxpool2_bwd"), rt.ptr(i), i.ld, rt.gptr(d), d.ld, i.N, i.H, i.W, i.C, rt.gptr(i), i.ld, acc,
             rt.stream)
        rt.mark_written(i)


# ------------------------------------------------------------------------ program

class Program:
    def __init__(self, N, H, W, math="f32"):
        if math not in MATHS:
            raise ValueError(f"conv math must be one of {MATHS}, got {math!r}")
        self.N, self.H, self.W = N, H, W
        self.math = math     # "f32" | "bf16" (set_conv_math)
        self.bufs = {}       # name -> (rows, ld)
        self.ops = []
        self.logits = None   # Act of the (low-res for MobileNetV2UNet) logits
        self.out_hw = (H, W)
        self._n = 0
        self.image = self.new(3, H, W, name=IMAGE)  # NHWC4 copy of the input batch
        # memoised once the op list is complete (first walk)
        self._mb_groups = None   # mbconv_groups()
        self._bn_owner = None    # bn_owner()
        self._pack_key = None    # what the routes / packed weights / job table were built for (pack)
        self._fold_key = None    # ... and the folded inference weights (fold)
        self._fork_events = []   # events of an immediate backward's side-stream forks, reused step after step

    def wgrad_defer(self):
        """(from, at): the parameter gradients of ops >= from wait until the backward reaches op `at`, or None.
        bf16io default (DEFER_DECODER): the decoder's (from its first upsample on) until the encoder's last op --
        issued beside the encoder's memory-bound backward instead of the decoder's data-gradient convs
        (interleaved A/B, profiles/r06/ab_wgrad_defer.txt: bf16io +1.3 %, f32 -0.8 %)."""
        if WGRAD_DEFER is not None:
            return WGRAD_DEFER
        if not DEFER_DECODER or self.math != "bf16io":
            return None
        first_up = next((k for k, op in enumerate(self.ops) if isinstance(op, UpsampleOp)), None)
        return (first_up, first_up - 1) if first_up else None

    def mbconv_groups(self):
        """Folded forward: op index -> the (expand, depthwise, project) or (depthwise, project) ConvOps of a
        torchvision InvertedResidual that seg_mbconv_f16 runs as one launch (each intermediate activation
        consumed only inside the block: the lazy BN chain Program.make_lazy built)."""
        if self._mb_groups is not None:
            return self._mb_groups
        m, ops = {}, self.ops
        ok1 = (lambda op: isinstance(op, ConvOp) and op.kind == "igemm" and op.ks == 1 and op.stride == 1
               and op.bn is not None and op.conv.bias is None and op.cin_pad == op.cin)
        for k in range(len(ops) - 1):
            d, p = ops[k], ops[k + 1]
            if not (isinstance(d, ConvOp) and d.kind == "dw" and d.bn is not None and d.act == ACT_RELU6 and d.lazy
                    and ok1(p) and p.xform is d and p.act == ACT_NONE and p.inp is d.out):
                continue
            e = ops[k - 1] if k > 0 else None
            exp = (ok1(e) and e.act == ACT_RELU6 and e.lazy and e.res is None and d.xform is e and d.inp is e.out)
            cin = e.cin if exp else d.cout
            if p.res is not None and d.stride != 1:
                continue
            if not query("seg_mbconv_ok", cin, d.cout, p.cout, d.stride, int(exp)):
                continue
            if exp:
                m[k - 1] = (e, d, p)
            elif d.xform is None or d.xform.kind != "dw":
                m[k] = (d, p)
        self._mb_groups = m
        return m

    def stem_pre(self):
        """Folded fp16 forward: the stem ConvOp (features[0]: 3x3 stride-2 conv 3 -> 32, BN folded, ReLU6, the
        image its only input) when seg_stem_pre_f16 can run it on the frame directly, else None."""
        ops = self.ops
        if not ops:
            return None
        op = ops[0]
        if not (isinstance(op, ConvOp) and op.kind == "igemm" and op.ks == 3 and op.stride == 2 and op.pad == 1
                and op.cin == 3 and op.cin_pad == 4 and op.cout == 32 and op.bn is not None and op.res is None
                and op.inp is self.image and op.fk_pack is not None and op.ldk_f == 36 and op.out.ld % 4 == 0
                and 0 not in self.mbconv_groups()):
            return None
        if any(getattr(o, "inp", None) is self.image or getattr(o, "res", None) is self.image for o in ops[1:]):
            return None
        return op

    def pw2_head(self):
        """Folded forward: index of outconv's first 1x1 conv when seg_pw2_f16 runs the head (1x1 -> folded BN ->
        ReLU -> 1x1, the program's last two ops, the hidden activation consumed only by the last conv), else
        None."""
        ops = self.ops
        if len(ops) < 2:
            return None
        c1, c2 = ops[-2], ops[-1]
        pw = (lambda op: isinstance(op, ConvOp) and op.kind == "igemm" and op.ks == 1 and op.stride == 1
              and op.fk_pack is None and op.res is None and op.cin_pad == op.cin)
        if not (pw(c1) and pw(c2) and c2.inp is c1.out and c1.bn is not None and c2.bn is None
                and c1.act in (ACT_RELU, ACT_RELU6) and c1.inp.ld % 4 == 0
                and query("seg_pw2_ok", c1.cin, c1.cout, c2.cout)):
            return None
        return len(ops) - 2

    def bn_owner(self):
        """Activation key -> the ConvOp with a BatchNorm whose output it is (the BN-backward reduction target of a
        data gradient writing exactly that region; ConvOp._bnout)."""
        if self._bn_owner is None:
            self._bn_owner = {op.out.key(): op for op in self.ops if isinstance(op, ConvOp) and op.bn is not None}
        return self._bn_owner

    def new(self, C, H, W, name=None):
        name = name or f"t{self._n}"
        self._n += 1
        ld = r4(C)
        self.bufs[name] = (self.N * H * W, ld)
        return Act(name, 0, ld, C, self.N, H, W)

    def conv(self, kind, conv, bn, act, inp, out=None, res=None, xform=None):
        ks, st, pd = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        Hi, Wi = inp.H, inp.W
        Ho, Wo = (Hi + 2 * pd - ks) // st + 1, (Wi + 2 * pd - ks) // st + 1
        if out is None:
            out = self.new(conv.out_channels, Ho, Wo)
        y = self.new(conv.out_channels, Ho, Wo) if bn is not None else out
        self.ops.append(ConvOp(kind, conv, bn, act, inp, out, y, res, xform))
        return out

    def make_lazy(self, a: Act, pointwise=False):
        """If `a` is the private BN+act output of the last op, drop its buffer and let
        the consumer apply the BN on load; returns the producer op (or None).
        pointwise: the consumer is a 1x1 conv (seg_conv_igemm_xf / seg_conv_wgrad_xf:
        the uniform-tap loader, 8-channel groups) -- any conv producer; otherwise a
        depthwise consumer (seg_dw_fwd / seg_dw_wgrad) of a dense producer.  (3x3
        consumers re-read every input element once per tap: measured slower, round 3.)"""
        op = self.ops[-1] if self.ops else None
        kinds = ("igemm", "dw") if pointwise else ("igemm",)
        if pointwise and not (a.C % 8 == 0 and a.C >= 16):
            return None
        if not (isinstance(op, ConvOp) and op.kind in kinds and op.bn is not None and op.res is None
                and op.out is a and op.y is not a and a.off == 0 and a.ld == r4(a.C)
                and self.bufs.get(a.buf) == (a.M, a.ld) and not a.buf.startswith("cat")):
            return None
        del self.bufs[a.buf]
        op.out, op.lazy = op.y, True
        return op

    def pack(self, rt):
        """Repack every conv weight for this step (one seg_pack_batch launch on the run's
        stream).  The routes, the packed buffers and the device job table are built once and
        rebuilt only when a weight's storage moves (e.g. model.to()) or a tile is forced."""
        convs = [op for op in self.ops if isinstance(op, ConvOp)]
        key = (_TILE_GEN, *(op.conv.weight.data_ptr() for op in convs))
        if self._pack_key != key:
            self._build_pack(convs, key)
        if self._njobs:
            rt.call("seg_pack_batch", self._jobs.data_ptr(), self._njobs, self._pack_blocks, rt.stream)

    def _build_pack(self, convs, key):
        """Pick the routes, then allocate the packed weights they read and build the pack job table."""
        pick_routes(self)
        jobs = []
        for op in convs:
            w = op.conv.weight
            op.wk_f = op.wk_d = None
            for d, r in enumerate((op.route_f, op.route_d)):
                if r is None or r.mode is None:
                    continue
                lay = r.mode & 15
                rows = op.cin if lay in (1, 4) else op.cout  # [rows][ldk]; Winograd: one such matrix per point
                wk = torch.empty((16 if lay in (3, 4) else 1) * rows * r.ldk, device=w.device,
                                 dtype=torch.bfloat16 if r.mode & 16 else torch.float32)
                kin = 1 if lay == 2 else r4(op.cout) if d else op.cin_pad
                jobs.append((w.data_ptr(), wk.data_ptr(), op.cout, 1 if lay == 2 else op.cin, op.ks, r.ldk, r.mode,
                             kin))
                if d:
                    op.wk_d = wk
                else:
                    op.wk_f = wk
        self._jobs, self._njobs, self._pack_blocks = pack_table(jobs, convs[0].conv.weight.device)
        self._pack_key = key

    def fold(self, stream):
        """Eval: fold every BatchNorm into its conv (one seg_bn_fold_batch launch) and
        pack the folded weights (one seg_pack_batch launch).  Buffers and job tables
        are built once per weight storage; re-run after the weights or running
        statistics change (Predictor.refresh)."""
        convs = [op for op in self.ops if isinstance(op, ConvOp)]
        key = tuple(op.conv.weight.data_ptr() for op in convs)
        if self._fold_key != key:
            self._build_fold(convs, key)
        call("seg_bn_fold_batch", self._fjobs.data_ptr(), len(convs), self._fmax, stream)
        if self._fpjobs is not None:
            call("seg_pack_batch", self._fpjobs.data_ptr(), self._fpn, self._fpmax, stream)

    def _build_fold(self, convs, key):
        import numpy as np
        ft = np.dtype([("w", "<u8"), ("bias", "<u8"), ("gamma", "<u8"), ("beta", "<u8"), ("rm", "<u8"),
                       ("rv", "<u8"), ("w_out", "<u8"), ("b_out", "<u8"), ("cout", "<i4"), ("kper", "<i4"),
                       ("eps", "<f4"), ("pad", "<i4")])
        assert ft.itemsize == 80
        fjobs, pjobs, fmax, pmax = [], [], 0, 0
        for op in convs:
            w, b, bn = op.conv.weight, op.conv.bias, op.bn
            dev = w.device
            kper = w[0].numel()
            op.fk = torch.empty_like(w, memory_format=torch.contiguous_format)
            op.fb = torch.zeros(r4(op.cout), device=dev, dtype=torch.float32)
            if bn is not None and not (bn.track_running_stats and bn.running_mean is not None):
                raise NotImplementedError("eval BatchNorm2d without running statistics")
            ptr = (lambda t: t.data_ptr() if t is not None else 0)
            fjobs.append((w.data_ptr(), ptr(b), ptr(bn.weight) if bn is not None else 0,
                          ptr(bn.bias) if bn is not None else 0, ptr(bn.running_mean) if bn is not None else 0,
                          ptr(bn.running_var) if bn is not None else 0, op.fk.data_ptr(), op.fb.data_ptr(),
                          op.cout, kper, bn.eps if bn is not None else 0.0, 0))
            if bn is not None and (bn.weight is None or bn.bias is None):
                raise NotImplementedError("BatchNorm2d(affine=False) folding")
            fmax = max(fmax, op.cout * kper + op.cout)
            if op.kind == "dw":
                op.fk_pack = torch.empty(9 * op.cout, device=dev, dtype=torch.float32)
                pjobs.append((op.fk.data_ptr(), op.fk_pack.data_ptr(), op.cout, 1, 3, 9, 2, 1))
                pmax = max(pmax, 9 * op.cout)
            elif op.ks == 1 and op.cin_pad == op.cin:
                op.fk_pack = None
            else:
                op.ldk_f = r4(op.ks * op.ks * op.cin_pad)
                op.fk_pack = torch.empty(op.cout * op.ldk_f, device=dev, dtype=torch.float32)
                pjobs.append((op.fk.data_ptr(), op.fk_pack.data_ptr(), op.cout, op.cin, op.ks, op.ldk_f, 0,
                              op.cin_pad))
                pmax = max(pmax, op.cout * op.ldk_f)
        dev = convs[0].conv.weight.device
        self._fjobs = torch.from_numpy(np.array(fjobs, dtype=ft).view(np.uint8).copy()).to(dev)
        self._fmax = fmax
        if pjobs:
            self._fpjobs, self._fpn, self._fpmax = pack_table(pjobs, dev)
        else:
            self._fpjobs, self._fpn, self._fpmax = None, 0, 0
        self._fold_key = key

    def params(self):
        seen, ps = set(), []
        for op in self.ops:
            for p in op.params():
                if id(p) not in seen:
                    seen.add(id(p))
                    ps.append(p)
        return ps


_PACK_JOB = [("w", "<u8"), ("wk", "<u8"), ("cout", "<i4"), ("cin", "<i4"), ("ks", "<i4"), ("ldk", "<i4"),
             ("mode", "<i4"), ("kin", "<i4"), ("blk0", "<i4"), ("nblk", "<i4")]


def pack_table(jobs, device):
    """Device table of seg_pack_job for seg_pack_batch from (w, wk, cout, cin, ks, ldk, mode,
    kin_pad) tuples: each job gets ceil(elements / 256) blocks of the launch.
    Returns (table, njobs, total blocks)."""
    import numpy as np
    rows, blk = [], 0
    for (w, wk, cout, cin, ks, ldk, mode, kin) in jobs:
        elems = 9 * cout if mode == 2 else (cout if (mode & 15) in (0, 3) else cin) * ldk
        nblk = max(1, (elems + 255) // 256)
        rows.append((w, wk, cout, cin, ks, ldk, mode, kin, blk, nblk))
        blk += nblk
    t = np.array(rows, dtype=np.dtype(_PACK_JOB))
    assert t.dtype.itemsize == 48
    return torch.from_numpy(t.view(np.uint8).copy()).to(device), len(rows), blk


def pick_routes(prog: Program) -> None:
    """Give every ConvOp of `prog` its forward / data-gradient / weight-gradient Route.  A pure function of the
    program's shapes and conv math, the engine switches (SEG_*, the diagnostics constants) and the library's host-side
    queries: no tensor, no device call.  The one place where a kernel is wired to the layers it runs."""
    if prog.math == "f16":
        raise NotImplementedError("f16 conv math is the inference configuration (Predictor(model, math='f16')); "
                                  "train with 'f32' or 'bf16'")
    sfx = "_bf16io" if prog.math == "bf16io" else ""
    for op in prog.ops:
        if not isinstance(op, ConvOp):
            continue
        if op.kind == "dw":
            nblk = query("seg_dw_wgrad_blocks", op.y.N, op.y.H, op.y.W, op.cout)
            op.route_f = Route("dw", "seg_dw_fwd" + sfx, None, 2, 9)  # [9][C], read by the data gradient too
            op.route_d = Route("dw", "seg_dw_dgrad" + sfx, None, None, 9)
            op.route_w = Route("dw", "seg_dw_wgrad" + sfx, None, work=nblk * 9 * op.cout, splits=nblk)
        else:
            op.route_f = _pick_conv(prog.math, op, 0)
            op.route_d = None if op.first else _pick_conv(prog.math, op, 1)  # no data gradient for the model input
            op.route_w = _pick_wgrad(prog.math, op)


def _frontier(prog: Program) -> list:
    """Per op (parameter gradients, data gradient, residual gradient): see grad_frontier.  The third flag is the
    same question as the second, asked of a ConvOp's residual input."""
    wrote = []  # (buffer, first channel, end channel, something trainable at or upstream of the writer)

    def upstream(a):
        return a is not None and any(f for (b, lo, hi, f) in wrote if b == a.buf and lo < a.off + a.C and a.off < hi)

    out = []
    for op in prog.ops:
        pg = any(p.requires_grad for p in op.params())
        src = op.low if isinstance(op, UpsampleOp) else op.inp
        dg, rg = upstream(src), upstream(getattr(op, "res", None))
        o = op.out
        wrote.append((o.buf, o.off, o.off + o.C, pg or dg or rg))
        out.append((pg, dg, rg))
    return out


def grad_frontier(prog: Program) -> list:
    """What the backward owes each op of `prog`: [(parameter gradients, data gradient)].  A pure function of the
    program and its parameters' requires_grad flags (no tensor data, no device call).  `parameter gradients`: one of
    the op's own parameters requires a gradient.  `data gradient`: some op upstream of this op's input has such a
    parameter -- transitively, through concat slices (a reader of the whole buffer is downstream of every slice's
    writer), residuals, pools and upsamples.  The backward skips an op with neither, runs no data gradient (nor a
    BatchNorm layer's dY, if its conv wants no gradient either) for an op without the second, and feeds a residual
    only where something upstream of it trains."""
    return [(pg, dg) for pg, dg, _ in _frontier(prog)]


def plan_signature(prog: Program) -> tuple:
    """What a recorded plan bakes in besides the shapes: each BatchNorm layer's mode (batch or running statistics)
    and each parameter's requires_grad (the gradient frontier, the flat gradient slots).  Part of the plan's key, so
    freezing or unfreezing between steps records (or finds again) the plan for that pattern."""
    return (tuple(op.bn.training for op in prog.ops if isinstance(op, ConvOp) and op.bn is not None),
            tuple(p.requires_grad for p in prog.params()))


def _pick_conv(math, op, d):
    """Route of a dense conv's forward (d = 0: x [M][K = cin_pad] -> y [M][C = Cout]) or data gradient (d = 1: the
    transposed conv, dY [M][K = r4(Cout)] -> dx [M][C = Cin]).  Precedence: thin-K 1x1, Winograd (f32), LDS halo (f32:
    where Winograd declined), igemm2 (where the halo kernel declined), the implicit GEMM (any shape)."""
    y, i, ks = op.y, op.inp, op.ks
    io, bf = math == "bf16io", math != "f32"
    K, C = (r4(op.cout), op.cin) if d else (op.cin_pad, op.cout)
    kind, sfx = ("dgrad" if d else "fwd"), ("_bf16io" if io else "")
    dense3 = ks == 3 and op.stride == 1 and op.pad == 1
    # bf16io launches take bf16 packed weights (_w16: half the weight bytes every M tile / pixel tile re-reads)
    w16 = io and W16
    mode, ldk = d + (16 if w16 else 0), (r8 if w16 else r4)(ks * ks * K)
    if not d and not w16 and ks == 1 and K == op.cin:
        mode, ldk = None, op.cin  # [Cout][Cin][1][1] already is the forward's packed layout
    name = "seg_conv_igemm" + (sfx or ("_bf16" if bf else ""))
    if not d and op.xform is not None:  # a conv applying its producer's lazy BN on load
        name += "_xf"
    igemm = Route("igemm", name + ("_w16" if w16 else ""), f"igemm{ks}_{kind}", mode, ldk,
                  None if d else Run.row_tiles(y.M, C),
                  bnout="seg_conv_igemm_bnout" + sfx + ("_w16" if w16 else "") if d and (io or not bf) else None)
    r = igemm
    # seg_conv_wino_pick: 1 = the two-launch form, 2 = the fused kernel (no M workspace), if the rows allow it
    wino = (query("seg_conv_wino_pick", y.N, y.H, y.W, K, C)
            if dense3 and not bf and WINOGRAD and (WINOGRAD_DGRAD if d else WINOGRAD_FWD) else 0)
    wide = y.M > IGEMM2_MAX_ROWS  # igemm2 beyond it: only GEMMs whose N fills the 8-wave tiles (UNet's deep levels)
    if (w16 or not bf) and _pw_pick(op, 8 if io else 4)[d]:
        r = Route("pw", "seg_conv_pw" + sfx, f"igemm1_{kind}", mode, ldk, (query("seg_conv_pw_row_tiles", y.M), 128),
                  fallback=igemm if d else None)
    elif wino:
        tiles = (query("seg_conv_wino_row_tiles", y.N, y.H, y.W), query("seg_conv_wino_tile_rows"))
        src_ld = (r4(op.cout) if op.bn is not None else op.out.ld) if d else i.ld  # of dY: ConvOp.backward
        if wino == 2 and query("seg_conv_wino_fused_ok", y.N, y.H, y.W, src_ld):
            r = Route("wino_fused", "seg_conv_wino_fused", f"wino3_{kind}", 3 + d, K, tiles)
        else:
            r = Route("wino", "seg_conv_wino", f"wino3_{kind}", 3 + d, K, tiles, work=16 * (y.M // 4) * C)
    elif (dense3 and (not bf or (io and HALO_BF16 and K % 8 == 0))  # bf16io: 8-channel slots
            and query("seg_conv_halo_pick", y.N, y.H, y.W, K, C)):
        r = Route("halo", "seg_conv_halo" + sfx + ("_w16" if w16 else ""), f"igemm3_{kind}", mode, ldk,
                  (query("seg_conv_halo_row_tiles", y.N, y.H, y.W), 256))
    elif (w16 and IGEMM2 and dense3 and (not wide or (IGEMM2_WIDE and C % 128 == 0))
            and i.ld % 8 == 0 and i.off % 8 == 0 and y.ld % 8 == 0 and y.off % 8 == 0  # 16-byte rows
            and (op.cout % 8 == 0 if d else op.xform is None and K == op.cin)):
        plan = igemm2_plan(y.M, C, K, ks)
        if plan is not None:
            r = Route("igemm2", "seg_conv_igemm2_bf16io", f"igemm{ks}_{kind}", mode, ldk, (plan[1], plan[0]),
                      work=plan[3], zero=True, fallback=igemm if d else None)
    return r if not d and op.bn is not None else r._replace(tiles=None)


def _pick_wgrad(math, op):
    """Weight-gradient Route of a dense conv: Winograd F(3x3,2x2) (f32), the persistent LDS-halo kernel (narrow
    bf16io 3x3), else the split-K implicit GEMM."""
    y, i, ks, K, cout = op.y, op.inp, op.ks, op.cin_pad, op.cout
    io, bf = math == "bf16io", math != "f32"
    dense3 = ks == 3 and op.stride == 1 and op.pad == 1
    if dense3 and not bf and WINOGRAD and WINOGRAD_WGRAD and op.xform is None:
        # seg_conv_wino_wgrad_pick: 2 = the all-points kernel (seg_conv_wino_wgrad16), 1 = the per-point one
        p = query("seg_conv_wino_wgrad_pick", y.N, y.H, y.W, K, cout)
        if p:
            name = "seg_conv_wino_wgrad16" if p == 2 else "seg_conv_wino_wgrad"
            splits = query(name + "_splits", y.N, y.H, y.W, K, cout)
            return Route("wino16" if p == 2 else "wino", name, "wino3_wgrad", work=splits * 16 * cout * K,
                         splits=splits)
    if (io and WGRAD2 and dense3 and op.xform is None and K == op.cin and y.ld % 8 == 0 and i.ld % 8 == 0
            and i.off % 8 == 0 and query("seg_conv_wgrad2_ok", y.N, y.H, y.W, K, cout)):
        blocks = query("seg_conv_wgrad2_blocks", y.N, y.H, y.W)
        return Route("wgrad2", "seg_conv_wgrad2_bf16io", "igemm3_wgrad", work=blocks * cout * 9 * K, splits=blocks)
    splits = query("seg_conv_wgrad_splits_bf16" if bf else "seg_conv_wgrad_splits", y.M, cout, K, ks)
    name = "seg_conv_wgrad" + ("_bf16io" if io else "_bf16" if bf else "") + ("_xf" if op.xform is not None else "")
    return Route("igemm", name, f"igemm{ks}_wgrad", work=splits * cout * ks * ks * K, splits=splits)


def _cna(prog, m: ConvBNReLU6, inp, out=None, kind=None, xform=None):
    conv, bn = m[0], m[1]
    if kind is None:
        kind = "dw" if conv.groups > 1 else "igemm"
    return prog.conv(kind, conv, bn, ACT_RELU6, inp, out=out, xform=xform)


def _inverted_residual(prog, blk: InvertedResidual, inp, out=None):
    layers = list(blk.conv)
    x = inp
    if len(layers) == 4:  # expand ratio != 1
        x = _cna(prog, layers[0], x)
        layers = layers[1:]
    # the depthwise conv applies its producer's BN + ReLU6 on load (the expand conv,
    # or the stem for features[1]) unless that activation is also the residual
    xf = None if (blk.use_res_connect and x is inp) else prog.make_lazy(x)
    if xf is not None:
        x = xf.out
    x = _cna(prog, layers[0], x, kind="dw", xform=xf)
    # ... and the 1x1 project conv applies the depthwise conv's BN + ReLU6 the same way
    xf = prog.make_lazy(x, pointwise=True)
    if xf is not None:
        x = xf.out
    return prog.conv("igemm", layers[1], layers[2], ACT_NONE, x, out=out,
                     res=inp if blk.use_res_connect else None, xform=xf)


def _double_conv(prog, dc, inp, out=None):
    c = dc.conv
    x = prog.conv("igemm", c[0], c[1], ACT_RELU, inp)
    return prog.conv("igemm", c[3], c[4], ACT_RELU, x, out=out)


def _up(prog, u, low, cat):
    """cat = [skip (already written) | upsample(low)]; returns double_conv output."""
    cs = cat.C - low.C
    if u.conv.conv[0].in_channels != cat.C:
        raise ValueError("up block channel mismatch")
    prog.ops.append(UpsampleOp(low, cat.slice(cs, low.C)))
    return _double_conv(prog, u.conv, cat)


def _outconv(prog, oc, inp):
    c = oc.conv
    x = prog.conv("igemm", c[0], c[1], ACT_RELU, inp)
    xf = prog.make_lazy(x, pointwise=True) if c[3].kernel_size[0] == 1 else None
    if xf is not None:
        x = xf.out
    return prog.conv("igemm", c[3], None, ACT_NONE, x, xform=xf)


def build_mobilenet_unet(model, N, H, W, math="f32") -> Program:
    """Program for MobileNetV2UNet.forward (src/unet.py:32-51)."""
    if H % 32 or W % 32:
        raise ValueError(f"MobileNetV2UNet needs H, W divisible by 32 (got {H}x{W}); the reference fails "
                         "with a torch.cat size mismatch on such inputs")
    p = Program(N, H, W, math)
    ups = [model.up1, model.up2, model.up3, model.up4]
    skip_c = [u.conv.conv[0].in_channels for u in ups]  # concat widths
    # concat buffers, finest first: cat4 @ H/2 (up4), cat3 @ H/4, cat2 @ H/8, cat1 @ H/16
    cats = {}
    for k, (u, div) in enumerate(zip(ups, (16, 8, 4, 2))):
        cats[k] = p.new(skip_c[k], H // div, W // div, name=f"cat{4 - k}")
    stages = [model.down1, model.down2, model.down3, model.down4, model.down5]
    skip_target = {0: cats[3], 1: cats[2], 2: cats[1], 3: cats[0]}
    x = p.image
    for si, stage in enumerate(stages):
        blocks = list(stage)
        for bi, blk in enumerate(blocks):
            last = bi == len(blocks) - 1
            out = None
            if last and si in skip_target:
                oc = blk.out_channels
                out = skip_target[si].slice(0, oc)
            if isinstance(blk, InvertedResidual):
                x = _inverted_residual(p, blk, x, out=out)
            elif isinstance(blk, ConvBNReLU6):
                x = _cna(p, blk, x, out=out)
            else:
                raise TypeError(f"unexpected encoder block {type(blk).__name__}")
    for k, u in enumerate(ups):
        x = _up(p, u, x, cats[k])
    p.logits = _outconv(p, model.outc, x)
    fu = model.final_upsample
    if fu.scale_factor not in (2, 2.0) or not fu.align_corners:
        raise ValueError("final_upsample must be x2 bilinear align_corners=True")
    p.out_hw = (H, W)
    return p


def build_unet(model, N, H, W, math="f32") -> Program:
    """Program for UNet / LightUNet.forward (src/unet.py:137-147, :160-171)."""
    if H % 8 or W % 8:
        raise ValueError(f"UNet needs H, W divisible by 8 (got {H}x{W})")
    p = Program(N, H, W, math)
    b = model.inc.conv.conv[0].out_channels
    cat3 = p.new(model.up3.conv.conv[0].in_channels, H, W, name="cat3")          # [x1 | up(u2)]
    cat2 = p.new(model.up2.conv.conv[0].in_channels, H // 2, W // 2, name="cat2")  # [x2 | up(u1)]
    cat1 = p.new(model.up1.conv.conv[0].in_channels, H // 4, W // 4, name="cat1")  # [x3 | up(x4)]
    x1 = _double_conv(p, model.inc.conv, p.image, out=cat3.slice(0, b))
    d1 = model.down1.mpconv[1]
    pooled = p.new(x1.C, H // 2, W // 2)
    p.ops.append(PoolOp(x1, pooled))
    x2 = _double_conv(p, d1, pooled, out=cat2.slice(0, d1.conv[3].out_channels))
    d2 = model.down2.mpconv[1]
    pooled = p.new(x2.C, H // 4, W // 4)
    p.ops.append(PoolOp(x2, pooled))
    x3 = _double_conv(p, d2, pooled, out=cat1.slice(0, d2.conv[3].out_channels))
    d3 = model.down3.mpconv[1]
    pooled = p.new(x3.C, H // 8, W // 8)
    p.ops.append(PoolOp(x3, pooled))
    x4 = _double_conv(p, d3, pooled)
    x = _up(p, model.up1, x4, cat1)
    x = _up(p, model.up2, x, cat2)
    x = _up(p, model.up3, x, cat3)
    p.logits = _outconv(p, model.sem_out, x)
    p.out_hw = (H, W)
    return p


def build_program(model, N, H, W, math="f32") -> Program:
    from .unet import MobileNetV2UNet, UNet, LightUNet
    if isinstance(model, MobileNetV2UNet):
        prog = build_mobilenet_unet(model, N, H, W, math)
    elif isinstance(model, (UNet, LightUNet)):
        prog = build_unet(model, N, H, W, math)
    else:
        raise TypeError(f"no HIP program for {type(model).__name__}")
    return prog


# Conv arithmetic of a model's programs.  "f32" (default): exact fp32 products on the
# f32 MFMA (plus Winograd / LDS-halo kernels where they measured faster), the
# reference's own arithmetic.  "bf16": the bf16 configurations (BASELINE configs[2],
# [4]; the reference's equivalent is torch.autocast(dtype=torch.bfloat16) around the
# forward) -- every dense / pointwise conv, forward and both gradients, multiplies
# bf16-rounded operands on the bf16 MFMA with fp32 accumulation; activations, BN,
# depthwise convs, the loss and the optimizer stay fp32.
MATHS = ("f32", "bf16", "bf16io", "f16")
# "bf16io": bf16 conv math AND bf16 activation / gradient storage (every tensor between
# kernels is bf16 in HBM, halving the memory-bound passes; BN statistics, partial sums,
# parameter gradients, the loss and Adam stay fp32) -- the _bf16io entry points.
# "f16" is the fp16 inference configuration (BASELINE configs[3]): the BN-folded eval
# forward (Predictor) with fp16 conv operands; training programs refuse it.
_FOLDED_CONV = {"f32": "seg_conv_igemm_act", "bf16": "seg_conv_igemm_bf16", "f16": "seg_conv_igemm_f16"}


def set_conv_math(model, math: str):
    """Select the conv arithmetic ("f32" | "bf16") of `model` (or a DataParallel wrapper's module)."""
    if math not in MATHS:
        raise ValueError(f"conv math must be one of {MATHS}, got {math!r}")
    model = getattr(model, "module", model)
    model.__dict__["_segamd_math"] = math
    return model


# ------------------------------------------------------------------------ runtime

class Run:
    """State of one forward (and its backward): buffers, saved BN statistics,
    gradient buffers and which gradient regions have been written.

    Two ways to execute the walk: immediately (every launch is a ctypes call on the
    current stream -- the Predictor's folded eval forward, captured in a hipGraph), or
    recorded (`rec` set: every launch, event pair and memset becomes an entry of a
    launch tape, seg_amd/tape.py; all buffers are then persistent so the tape can be
    replayed step after step)."""

    def __init__(self, prog: Program, image: torch.Tensor, training: bool, rec=None, side=None):
        self.prog, self.image, self.training = prog, image, training
        self.device = image.device
        self.stream = torch.cuda.current_stream(self.device).cuda_stream
        self.rec = rec
        # activation / gradient storage: fp32, or bf16 for math "bf16io" (the _bf16io kernels)
        self.io = prog.math == "bf16io"
        self.store = torch.bfloat16 if self.io else torch.float32
        self.es = 2 if self.io else 4
        self.bufs = {n: torch.empty(rows * ld, device=self.device, dtype=self.store)
                     for n, (rows, ld) in prog.bufs.items()}
        self.saved = {}
        self.bn_train = {}    # id(op) -> its BatchNorm ran on batch statistics (ConvOp.forward; False: frozen / none)
        self.need = None      # _frontier(prog), taken when the backward starts
        self.bn_parts = {}    # id(op) -> [tile partials, tiles, write generation]: its BN-backward reduction from
                              # the epilogue of the data gradient that completed its dA (seg_conv_igemm_bnout*)
        self.wgen = {}        # gradient buffer name -> write generation (every write to the buffer bumps it)
        self._mb = {}         # folded forward: op index -> (partials, tile counters) of a fused inverted residual
        self.gbufs = {}
        self.keep = []        # workspaces of a recorded run (persistent: the tape points at them)
        self.written = {}     # grad buffer name -> list of (lo, hi) channel ranges
        self.pending = {}     # Act.key() -> addend Act (residual upstream gradient)
        self.grads = {}       # id(param) -> grad tensor
        self.flat = None      # recorded run: one flat fp32 buffer holding every parameter gradient (Plan.forward)
        self.flat_slots = {}  # ... id(param) -> (offset, elements) in it
        self.sync = None
        self._tmp_n = 0
        self.side = side      # side stream of the parameter gradients (recorded backward)
        self.main = None      # immediate backward with overlap (backward_from_logits): torch's current stream,
        self._side_ctx = None  # and the side stream's context that every fork re-enters
        self._n_fork = 0      # side-stream forks so far (index into the program's event pool)
        self.cur_op = -1      # index of the op whose backward is running
        self.deferred = []    # (op, dY, dY ptr) whose parameter gradients wait for flush_deferred
        self.defer = prog.wgrad_defer()  # (from, at) of the deferred parameter gradients, or None
        # the fused loss's forward (_loss_forward), read by its backward
        self.target = self.weight = self.stats = None  # labels, class weights, the [loss, count, ...] buffer
        self.loss = None        # its kernel family, options and buffers (a Loss)
        self.teacher = None     # a DistillLoss: the teacher's low-resolution logits (fp32 NHWC rows)

    @property
    def ohem(self):
        """(tau, workspace) of an OhemCELoss's forward, else None."""
        L = self.loss
        return (L.opt[0], L.work) if L is not None and L.fam is LOSS_FAMILIES["ohem"] else None

    def k(self, name: str) -> str:
        """C-ABI entry point of an activation kernel for this run's storage type."""
        return name + "_bf16io" if self.io else name

    # launches
    def call(self, name, *args):
        if self.rec is not None:
            self.rec.call(name, args)
        else:
            call(name, *args)

    def tcall(self, kind, flops, name, *args):
        """A launch of the roofline kernel families (bench.py times them)."""
        if self.rec is not None:
            self.rec.call(name, args, timer=(kind, flops))
        else:
            _timed_call(kind, flops, name, *args)

    def zero_param_grad(self, p: torch.Tensor, stream) -> None:
        """An all-zero gradient for parameter `p`.  A recorded run's gradient slot is persistent and
        nothing else writes it, so it is zeroed once, now (on the current stream, ahead of every
        replay), and the tape gets no entry; an immediate run zeroes its fresh tensor on the current stream
        (`stream`: inside the fork context).  Under DataParallel the slot is a view into an
        all-reduced gradient bucket into which a synchronised backward folds any `.grad` a rank
        still holds, so a recorded run re-zeroes it every step (a tape memset on `stream`) -- a
        once-only zero would keep that fold and double it on every later step."""
        self.grad_param(p)
        g = self.grads[id(p)]
        g.zero_()
        if self.rec is not None and self.sync is not None:
            self.rec.memset2d(g.data_ptr(), g.numel() * 4, 0, g.numel() * 4, 1, stream)

    def zero(self, a: Act):
        """Zero-fill the gradient region of `a` (a channel slice of a row buffer)."""
        self.wgen[a.buf] = self.wgen.get(a.buf, 0) + 1
        if self.rec is not None:
            self.rec.memset2d(self.gptr(a), a.ld * self.es, 0, a.C * self.es, a.M, self.stream)
        else:
            self.gbuf(a.buf).view(-1, a.ld)[:, a.off:a.off + a.C].zero_()

    # pointers
    def ptr(self, a: Act) -> int:
        if a.buf.startswith("#"):
            return self.gbufs[a.buf].data_ptr() + self.es * a.off
        return self.bufs[a.buf].data_ptr() + self.es * a.off

    def gptr(self, a: Act) -> int:
        if a.buf.startswith("#"):
            return self.gbufs[a.buf].data_ptr() + self.es * a.off
        return self.gbuf(a.buf).data_ptr() + self.es * a.off

    def gbuf(self, name):
        g = self.gbufs.get(name)
        if g is None:
            g = self.gbufs[name] = torch.empty_like(self.bufs[name])
        return g

    def tmp(self, n: int, zero: bool = False) -> torch.Tensor:
        """A float32 workspace; zero=True for the channel reductions' workspaces, whose ticket
        words (the in-launch finalize, csrc/bn.hip) must be zero before their first use."""
        t = (torch.zeros if zero else torch.empty)(max(int(n), 1), device=self.device, dtype=torch.float32)
        if self.rec is not None:
            self.keep.append(t)
        return t

    @staticmethod
    def row_tiles(M: int, C: int):
        key = (M, C)
        r = _ROW_TILES.get(key)
        if r is None:
            rows = ctypes.c_int(0)
            n = query("seg_conv_igemm_row_tiles", M, C, ctypes.addressof(rows))
            r = _ROW_TILES[key] = (n, rows.value)
        return r

    def tmp_buf(self, n: int) -> str:
        name = f"#tmp{self._tmp_n}"
        self._tmp_n += 1
        self.gbufs[name] = torch.empty(max(int(n), 1), device=self.device, dtype=self.store)
        return name

    # streams
    def fork(self):
        """(context, stream handle) for work that may run beside the main stream: with
        overlap on, the side stream first waits for everything issued so far on the main
        stream; temporaries allocated inside the context belong to the side stream."""
        if self.side is None:
            return contextlib.nullcontext(), self.stream
        if self.rec is not None:
            ev = self.rec.event()
            self.rec.record(ev, self.stream)
            self.rec.wait(self.side.cuda_stream, ev)
            return contextlib.nullcontext(), self.side.cuda_stream
        # events are reused step after step (a wait binds to the record before it)
        pool = self.prog._fork_events
        if self._n_fork == len(pool):
            pool.append(torch.cuda.Event())
        ev = pool[self._n_fork]
        self._n_fork += 1
        ev.record(self.main)
        self.side.wait_event(ev)
        return self._side_ctx, self.side.cuda_stream

    def param_grads(self, op, dY, dYp):
        """Where the parameter gradients of the running op go: beside the main stream now (behind a fork), or, for
        the ops of the deferred range (Program.wgrad_defer), later, beside the memory-bound part of the backward
        (flush_deferred; dY stays valid, it is persistent within the run)."""
        if self.defer is not None and self.side is not None and self.cur_op >= self.defer[0]:
            self.deferred.append((op, dY, dYp))
            return
        ctx, sw = self.fork()
        with ctx:
            op._param_grads(self, dY, dYp, sw)

    def flush_deferred(self):
        """Issue the deferred parameter gradients on the side stream, in backward order, behind one fork."""
        if not self.deferred:
            return
        ctx, sw = self.fork()
        with ctx:
            for op, dY, dYp in self.deferred:
                op._param_grads(self, dY, dYp, sw)
        self.deferred = []

    def join(self):
        if self.side is None:
            return
        if self.rec is not None:
            ev = self.rec.event()
            self.rec.record(ev, self.side.cuda_stream)
            self.rec.wait(self.stream, ev)
        else:
            self.main.wait_stream(self.side)

    # gradient-region bookkeeping
    def _covered(self, a: Act) -> bool:
        lo, hi = a.off, a.off + a.C
        for (l, h) in self.written.get(a.buf, ()):
            if l <= lo and hi <= h:
                return True
        return False

    def mark_written(self, a: Act):
        self.written.setdefault(a.buf, []).append((a.off, a.off + a.C))
        self.wgen[a.buf] = self.wgen.get(a.buf, 0) + 1

    def grad_of(self, a: Act) -> Act:
        """Gradient region of activation `a` (zero-filled if nobody wrote it)."""
        if not self._covered(a):
            add = self.pending.pop(a.key(), None)
            if add is not None:
                self.call(self.k("seg_add"), self.gptr(add), add.ld, None, 0, a.M, a.C, self.gptr(a), a.ld, self.stream)
            else:
                self.zero(a)
            self.mark_written(a)
        return a

    def add_pending(self, target: Act, addend: Act):
        if self._covered(target):
            self.call(self.k("seg_add"), self.gptr(target), target.ld, self.gptr(addend), addend.ld, target.M, target.C,
                      self.gptr(target), target.ld, self.stream)
            self.wgen[target.buf] = self.wgen.get(target.buf, 0) + 1
        else:
            self.pending[target.key()] = addend

    def begin_write_add(self, a: Act):
        """For writers with a fused addend: returns (add_ptr, add_ld)."""
        if self._covered(a):
            return self.gptr(a), a.ld
        add = self.pending.pop(a.key(), None)
        if add is not None:
            return self.gptr(add), add.ld
        return None, 0

    def begin_write_accumulate(self, a: Act) -> int:
        """For writers with only an accumulate flag: materialise a pending addend first."""
        if self._covered(a):
            return 1
        add = self.pending.pop(a.key(), None)
        if add is not None:
            self.call(self.k("seg_add"), self.gptr(add), add.ld, None, 0, a.M, a.C, self.gptr(a), a.ld, self.stream)
            self.mark_written(a)
            return 1
        return 0

    def grad_param(self, p: torch.Tensor) -> int:
        g = self.grads.get(id(p))
        if g is None:
            g = self.sync.grad_storage(p) if self.sync is not None else None
            if g is None and self.flat is not None:
                o, n = self.flat_slots[id(p)]
                g = self.flat[o:o + n].view_as(p)
            if g is None:
                g = torch.empty_like(p)
            self.grads[id(p)] = g
        return g.data_ptr()

    def params_done(self, ps, stream=None):
        """The gradients of `ps` are complete on `stream` (DataParallel bucket readiness)."""
        if self.sync is None:
            return
        ready = [p for p in ps if id(p) in self.grads]
        if self.rec is None:
            self.sync.on_ready(ready)
            return
        sync = self.sync
        st = self.side if (self.side is not None and stream == self.side.cuda_stream) else None
        done = sync.plan_ready(ready)  # the buckets this point completes; a host stop only then
        if not done:
            return

        def on_ready():  # host callback between tape segments
            if st is None:
                sync.launch_ready(done)
            else:
                with torch.cuda.stream(st):
                    sync.launch_ready(done)
        self.rec.stop(on_ready)

    # drivers
    def forward(self):
        global LAST_RUN
        x, img = self.image, self.prog.image
        self.prog.pack(self)
        self.call(self.k("seg_nchw_to_nhwc"), x.data_ptr(), img.N, 3, img.H, img.W, self.ptr(img), img.ld, self.stream)
        for k, op in enumerate(self.prog.ops):
            if self.rec is not None:
                self.rec.label = f"{k}:fwd"
            op.forward(self)
        if DEBUG_KEEP_RUN:
            LAST_RUN = self

    def forward_folded(self, start=0):
        """Eval forward with every BatchNorm folded (Program.fold must have run): one
        launch per conv, or per inverted residual with fp16 conv math (seg_mbconv_f16).  The
        NHWC4 input rows must already be in the image buffer (start = 0), or ops[:start] have
        run (the stem fused with the preprocess, Program.stem_pre)."""
        ops = self.prog.ops
        f16 = self.prog.math == "f16"
        groups = self.prog.mbconv_groups() if MBCONV and f16 else {}
        head = self.prog.pw2_head() if PW2 and f16 else None
        k = start
        while k < len(ops):
            g = groups.get(k)
            if g is not None:
                self._mbconv(k, g)
                k += len(g)
                continue
            if k == head:
                c1, c2 = ops[k], ops[k + 1]
                x, o = c1.inp, c2.out
                call("seg_pw2_f16", self.ptr(x), x.ld, x.N * x.H * x.W, c1.cin, c1.fk.data_ptr(),
                     c1.fb.data_ptr() if c1.fb is not None else None, c1.cout, c1.act, c2.fk.data_ptr(),
                     c2.fb.data_ptr() if c2.fb is not None else None, c2.cout, self.ptr(o), o.ld, self.stream)
                k += 2
                continue
            op = ops[k]
            if isinstance(op, ConvOp):
                op.forward_folded(self)
            else:
                op.forward(self)
            k += 1

    def _mbconv(self, k, g):
        """One fused inverted residual (expand?, depthwise, project) of the folded forward."""
        e, d, p = (g[0], g[1], g[2]) if len(g) == 3 else (None, g[0], g[1])
        x = e.inp if e is not None else d.inp
        o, r = p.out, p.res
        bufs = self._mb.get(k)
        if bufs is None:  # persistent across graph replays: allocated by the warm-up launch, before any capture
            ncnt = ctypes.c_int(0)
            nw = query("seg_mbconv_work_floats", x.N, x.H, x.W, d.cout, p.cout, d.stride, ctypes.addressof(ncnt))
            bufs = self._mb[k] = (torch.empty(max(nw, 1), device=self.device, dtype=torch.float32),
                                  torch.zeros(max(ncnt.value, 1), device=self.device, dtype=torch.int32))
        call("seg_mbconv_f16", self.ptr(x), x.ld, x.N, x.H, x.W, x.C, e.fk.data_ptr() if e is not None else None,
             e.fb.data_ptr() if e is not None else None, d.cout, d.fk_pack.data_ptr(), d.fb.data_ptr(), d.stride,
             p.fk.data_ptr(), p.fb.data_ptr(), p.cout, self.ptr(r) if r is not None else None,
             r.ld if r is not None else 0, self.ptr(o), o.ld, bufs[0].data_ptr(), bufs[1].data_ptr(), self.stream)

    def backward_from_logits(self):
        global LAST_RUN
        if self.rec is None and OVERLAP:
            self.main = torch.cuda.current_stream(self.device)
            self.side = _side_stream(self.device)
            self._side_ctx = torch.cuda.StreamContext(self.side)  # re-entered by every fork
        self.need = _frontier(self.prog)
        try:
            for k in range(len(self.prog.ops) - 1, -1, -1):
                self.cur_op = k
                if self.defer is not None and k == self.defer[1]:
                    self.flush_deferred()
                if not any(self.need[k]):  # behind the gradient frontier: nothing here or upstream trains
                    continue
                if self.rec is not None:
                    self.rec.label = f"{k}:bwd"
                self.prog.ops[k].backward(self)
            self.flush_deferred()
        finally:
            self.join()
        if DEBUG_KEEP_RUN:
            LAST_RUN = self


# Engine switches: the ones a test, bench.py, the Predictor or INTEGRATION.md uses.  Environment switches (SEG_*) are
# the A/B knobs of measured design choices, read at import; the module constants below them are diagnostics the tests
# flip directly (monkeypatch), not user settings.  (The switches of finished experiments are gone with the paths only
# they selected; DESIGN.md keeps their measurements.)
#
# Parameter gradients (weight / bias / BN-affine readiness) run on a second HIP stream
# beside the data-gradient chain: the compute-bound 3x3 weight gradients overlap the
# memory-bound BatchNorm / depthwise / 1x1 kernels of the main stream.  Results are the
# same either way (the kernels and their reduction orders do not change).  A layer's fork comes after its data
# gradient (ConvOp.backward; measured against forking first: f32 +1.5 %, bf16io +-0).
OVERLAP = os.environ.get("SEG_OVERLAP", "1") == "1"
# Winograd F(2x2,3x3) for the deep f32 3x3 convs (read when a program's weights are first
# packed); SEG_WINO=0 routes them to the LDS-halo / implicit-GEMM kernels instead.
WINOGRAD = os.environ.get("SEG_WINO", "1") == "1"
# LDS-halo direct 3x3 conv for the narrow convs in the bf16io configuration; SEG_HALO_BF16=0 turns it off.
HALO_BF16 = os.environ.get("SEG_HALO_BF16", "1") == "1"
# ... and their weight gradients on the persistent LDS-halo kernel (seg_conv_wgrad2_bf16io); SEG_WGRAD2=0 = off
WGRAD2 = os.environ.get("SEG_WGRAD2", "1") == "1"
# BatchNorm-backward reduction from the epilogue of the implicit-GEMM data gradient that completes a BN layer's dA
# (seg_conv_igemm_bnout*: no reduction pass over dA; the finalize reads the tile partials); SEG_BNOUT=0 = off.  Up to
# BNOUT_MAX_TILES row tiles (the finalize's serial tile loop), i.e. the small-image layers where the three-launch
# BN backward is latency-bound
BNOUT = os.environ.get("SEG_BNOUT", "1") == "1"
BNOUT_MAX_TILES = int(os.environ.get("SEG_BNOUT_MAX_TILES", "1024"))
# the bias gradient of a conv followed by train-mode BatchNorm is exactly zero: write zeros instead of
# reducing dY (SEG_ZERO_BN_BIAS=0 keeps the reduction, whose result is rounding noise)
ZERO_BN_BIAS = os.environ.get("SEG_ZERO_BN_BIAS", "1") == "1"
# thin-K 1x1 convs (K <= 32) on seg_conv_pw instead of the generic implicit GEMM; SEG_PW=0 = off
PW = os.environ.get("SEG_PW", "1") == "1"
PW_MIN_ROWS = int(os.environ.get("SEG_PW_MIN_ROWS", "262144"))
# bf16io deep 3x3 convs on the 8-wave LDS-DMA implicit GEMM (seg_conv_igemm2_bf16io, csrc/igemm2.hip); SEG_IGEMM2=0
# = off
IGEMM2 = os.environ.get("SEG_IGEMM2", "1") == "1"
# ... on images of at most this many output rows: measured per launch on UNet 512x1024 bf16io, igemm2 is 5-25 %
# slower than the 4-wave implicit GEMM at 262k-4M rows and 1-6 % faster at 65k (profiles/r03k)
IGEMM2_MAX_ROWS = int(os.environ.get("SEG_IGEMM2_MAX_ROWS", "65536"))
# ... and beyond that on the convs whose GEMM N is a multiple of 128 (the 8-wave tiles without padding): measured per
# launch at HEAD of round 4 on UNet 512x1024 bf16io, side stream off, 1-10 % faster than the 4-wave implicit GEMM on
# every such launch (profiles/r04ig/); SEG_IGEMM2_WIDE=0 = off
IGEMM2_WIDE = os.environ.get("SEG_IGEMM2_WIDE", "1") == "1"
# bf16io implicit GEMMs on bf16-packed weights (seg_conv_igemm_bf16io_w16); SEG_W16=0 keeps the fp32 packs
W16 = os.environ.get("SEG_W16", "1") == "1"
# SEG_WGRAD_DEFER=from:at (A/B): the parameter gradients of program ops >= `from` are issued on the side stream only
# when the backward reaches op `at` (all of them behind one fork), instead of right after each layer's data gradient
_wd = os.environ.get("SEG_WGRAD_DEFER", "")
WGRAD_DEFER = tuple(int(v) for v in _wd.split(":")) if _wd else None
# bf16io: the decoder's parameter gradients deferred until the backward reaches the encoder (Program.wgrad_defer);
# SEG_DEFER_DECODER=0 = off
DEFER_DECODER = os.environ.get("SEG_DEFER_DECODER", "1") == "1"

# Diagnostics (tests flip these): the Winograd transforms one at a time (parity attribution,
# tests/test_gpu_unet_cfg5.py) ...
WINOGRAD_WGRAD = True  # the F(3x3,2x2) weight gradients (seg_conv_wino_wgrad_pick: all-points or per-point kernel)
WINOGRAD_FWD = True    # the F(2x2,3x3) forward
WINOGRAD_DGRAD = True  # ... and data-gradient transforms
# ... and the fp16 inference (Predictor, BASELINE configs[3]) fusions against their unfused launches: each inverted
# residual of the folded forward as one launch (seg_mbconv_f16), the stem forming the preprocessed frame on load
# (seg_stem_pre_f16), outconv's 1x1 -> BN -> ReLU -> 1x1 head in one launch (seg_pw2_f16).  (The other folded convs
# always run on seg_conv_igemm_plan_b1's tile / split count, the batch-1 decoder convs' plan.)
MBCONV = True
STEM_PRE = True
PW2 = True
_SIDE = {}


def _side_stream(device):
    st = _SIDE.get(device)
    if st is None:
        st = _SIDE[device] = torch.cuda.Stream(device, priority=0)
    return st


DEBUG_KEEP_RUN = False  # diagnostics: keep the last Run (buffers + gradient buffers)
LAST_RUN = None


def debug_preactivations(model) -> dict:
    """Diagnostics (needs DEBUG_KEEP_RUN = True before the forward): every activation
    layer's post-BatchNorm pre-activation z = y * scale + shift of the last run, as fp64
    NCHW CPU tensors keyed by the conv's module path + "." (the parity tests compare them
    with the oracle and take the ReLU/ReLU6 masks from them)."""
    run = LAST_RUN
    if run is None:
        raise RuntimeError("set engine.DEBUG_KEEP_RUN = True before the forward")
    model = getattr(model, "module", model)
    names = {}
    for n, m in model.named_modules():
        names.setdefault(id(m), n)
    out = {}
    for op in run.prog.ops:
        if isinstance(op, ConvOp) and op.bn is not None and op.act != ACT_NONE:
            y, C = op.y, op.cout
            t = run.bufs[y.buf].view(-1, y.ld)[:, y.off:y.off + C].double()
            st = run.saved[id(op)].double()
            z = t * st[2 * C:3 * C] + st[3 * C:4 * C]
            out[names[id(op.conv)] + "."] = z.view(y.N, y.H, y.W, C).permute(0, 3, 1, 2).cpu()
    return out


_PROGRAM_CACHE_ATTR = "_segamd_programs"


def debug_pool_positions(model) -> dict:
    """Diagnostics (DEBUG_KEEP_RUN, like debug_preactivations): the 2x2-window position (0..3, row-major; first
    maximum, the kernel's and aten's tie rule) every max-pool of the last run chose, from the values the kernel read,
    keyed "down1.", "down2.", ... in forward order (UNet's `down` blocks, src/unet.py:85) -- the parity checker routes
    the fp64 oracle's max-pool gradients through them (oracle/budget.py)."""
    run = LAST_RUN
    if run is None:
        raise RuntimeError("set engine.DEBUG_KEEP_RUN = True before the forward")
    out, k = {}, 0
    for op in run.prog.ops:
        if isinstance(op, PoolOp):
            i = op.inp
            a = run.bufs[i.buf].view(-1, i.ld)[:, i.off:i.off + i.C].float().cpu()
            a = a.view(i.N, i.H // 2, 2, i.W // 2, 2, i.C).permute(0, 5, 1, 3, 2, 4).reshape(i.N, i.C, i.H // 2,
                                                                                           i.W // 2, 4)
            k += 1
            out[f"down{k}."] = a.argmax(-1)
    return out


def get_program(model, N, H, W, math=None) -> Program:
    cache = model.__dict__.setdefault(_PROGRAM_CACHE_ATTR, {})
    math = math or model.__dict__.get("_segamd_math", "f32")
    key = (N, H, W, math)
    prog = cache.get(key)
    if prog is None:
        prog = cache[key] = build_program(model, N, H, W, math)
    return prog


def _check_input(x: torch.Tensor):
    if not x.is_cuda:
        raise RuntimeError("segamd models run on the MI355X HIP path only; move the model and input to 'cuda' "
                           "(there is no CPU execution path)")
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"expected float32 input [N,3,H,W], got {tuple(x.shape)} {x.dtype}")
    if x.requires_grad:
        raise NotImplementedError("gradient w.r.t. the input image is not supported")


REDUCTIONS = {"mean": 0, "sum": 1}  # the C ABI's `reduction` (include/segamd.h: seg_cew_*)


class Ohem(NamedTuple):
    """A seg_amd.OhemCELoss's two options in loss_options' fourth slot: the seg_ohem_* kernels."""
    thresh: float
    min_kept: float  # an int: pixels, or a fraction of the batch's N * Ho * Wo (losses.resolve_min_kept)


class Distill(NamedTuple):
    """A seg_amd.DistillLoss's four options and the teacher tensor's geometry in loss_options' fourth slot: the
    seg_kd_* kernels.  Ht / Wt are 0 until the teacher tensor is known (check_teacher_logits)."""
    ce: float
    kd: float
    temperature: float
    kd_ignored: bool
    Ht: int = 0
    Wt: int = 0


class Binary(NamedTuple):
    """A seg_amd.BinarySegLoss's scalars in loss_options' fourth slot: the seg_bce_* kernels.  threshold is read by
    "metrics" mode only (the confusion matrix's z > zthr)."""
    bce: float
    dice: float
    focal_gamma: float
    dice_smooth: float
    pos_weight: float
    threshold: float = 0.5


def check_teacher_logits(teacher_logits, N, C, device):
    """(Ht, Wt) of a teacher's low-resolution logits as the seg_kd_* kernels take them: a contiguous float32
    [N, Ht, Wt, round4(C)] tensor on `device` (model.forward_low_logits' result); ValueError otherwise."""
    ldt = (C + 3) & ~3
    t = teacher_logits
    if t is None:
        raise ValueError("kd > 0 needs teacher_logits (the teacher's forward_low_logits(x))")
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or t.device != device
            or not t.is_contiguous() or t.shape[0] != N or t.shape[3] != ldt or t.shape[1] < 1 or t.shape[2] < 1):
        what = f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"teacher_logits must be a contiguous float32 [{N}, Ht, Wt, {ldt}] tensor on {device} "
                         f"(NHWC rows of {C} classes), got {what}")
    if t.requires_grad:
        raise ValueError("teacher_logits must not require a gradient: the teacher gets none")
    return int(t.shape[1]), int(t.shape[2])


def loss_options(weight, label_smoothing, reduction, C, device, ce=1.0, dice=0.0, focal_gamma=0.0, dice_smooth=1.0,
                 ohem_thresh=None, ohem_min_kept=None, kd=0.0, kd_temperature=1.0, kd_ignored=True, binary=False,
                 pos_weight=1.0, threshold=0.5):
    """The checked (weight, label_smoothing, reduction, sl) of a fused loss over C classes on `device`; ValueError
    for what the kernels do not take.  nn.CrossEntropyLoss's options for class-index targets, reduction "none" apart,
    and seg_amd.SegLoss's: sl is None for plain cross-entropy (ce = 1, no Dice term, no focal exponent: the seg_ce_* /
    seg_cew_* kernels, bitwise what they were), else (ce, dice, focal_gamma, dice_smooth) for the seg_sl_* kernels.
    With ohem_thresh / ohem_min_kept (a seg_amd.OhemCELoss's thresh and min_kept, both or neither) sl is an Ohem: the
    seg_ohem_* kernels, which take class weights and nothing else.  With kd != 0 (a seg_amd.DistillLoss's kd,
    temperature and kd_ignored) sl is a Distill: the seg_kd_* kernels, class weights and ce beside them and nothing
    else; the teacher tensor's geometry is filled in by the caller (check_teacher_logits).  With binary=True (a
    seg_amd.BinarySegLoss: ce is its bce coefficient, dice, focal_gamma and dice_smooth keep their names, pos_weight
    and threshold are its own) sl is a Binary: the seg_bce_* kernels over a model whose logits have one channel; class
    weights, label smoothing, any reduction but the mean, OHEM and kd are then a ValueError."""
    from .losses import (check_binary_combination, check_binary_options, check_distill_options, check_ohem_options,
                         check_seg_loss_options)
    if binary:
        check_binary_combination(weight, label_smoothing, reduction, ohem_thresh, ohem_min_kept, kd)
        if C != 1:
            raise ValueError(f"binary=True needs a model with one output channel, this one has {C}")
        bce, dice, focal_gamma, pos_weight, dice_smooth, threshold = check_binary_options(
            ce, dice, focal_gamma, pos_weight, dice_smooth, threshold)
        return None, 0.0, "mean", Binary(bce, dice, focal_gamma, dice_smooth, pos_weight, threshold)
    if kd != 0.0:
        sl = Distill(*check_distill_options(ce, kd, kd_temperature, label_smoothing, reduction, dice, focal_gamma,
                                            ohem_thresh, ohem_min_kept), bool(kd_ignored))
    else:
        ce, dice, focal_gamma, dice_smooth = check_seg_loss_options(ce, dice, focal_gamma, label_smoothing,
                                                                    dice_smooth)
        sl = None if (ce == 1.0 and dice == 0.0 and focal_gamma == 0.0) else (ce, dice, focal_gamma, dice_smooth)
        if ohem_thresh is not None or ohem_min_kept is not None:
            sl = Ohem(*check_ohem_options(ohem_thresh, ohem_min_kept, label_smoothing, reduction, ce, dice,
                                          focal_gamma))
    if sl is not None and not isinstance(sl, (Ohem, Distill)) and reduction != "mean":
        raise ValueError(f"a Dice or focal term (or ce != 1) is defined for reduction 'mean' only, got {reduction!r}")
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction must be 'mean' or 'sum' for the fused loss, got {reduction!r}")
    eps = float(label_smoothing)
    if not 0.0 <= eps <= 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1], got {label_smoothing!r}")
    if weight is not None:
        if not isinstance(weight, torch.Tensor) or weight.dtype != torch.float32 or tuple(weight.shape) != (C,) \
                or weight.device != device or not weight.is_contiguous():
            what = (f"{tuple(weight.shape)} {weight.dtype} on {weight.device}" if isinstance(weight, torch.Tensor)
                    else type(weight).__name__)
            raise ValueError(f"weight must be a contiguous float32 [{C}] tensor on {device}, got {what}")
        weight = weight.detach()
    return weight, eps, reduction, sl


def _plain_loss(weight, label_smoothing, reduction):
    return weight is None and label_smoothing == 0.0 and reduction == "mean"


class LossFamily(NamedTuple):
    """One kernel family of the fused loss (csrc/loss.hip): seg_<stem>_upsample_loss / _eval / _grad and what differs
    between the families' calls.  fwd / grad return a call's arguments up to (work, stats) / (grad_out, stats) and
    whatever the ABI puts right behind them, from the argument groups of _loss_args and the family's options;
    _loss_forward appends (confusion,) stream, _loss_backward the gradient buffer, (its leading dimension,) stream."""
    stem: str
    nstats: int   # floats of the stats buffer; [loss, D or #valid, #out-of-range labels] lead in every family
    has_eval: bool
    nchw: object  # None, or the suffix behind _bf16io of the twin whose gradient is fp32 NCHW instead of bf16 rows
    ac: int       # of the seg_upsample_bwd behind the gradient: 2 = the transpose of the kd kernels' own blend (lin_ac)
    fwd: object
    grad: object
    plane: bool = False  # the gradient is fp32 NCHW in BOTH maths, under the family's plain _grad name (no ldh)
    ev: object = None    # what an _eval call puts between the stats and the confusion matrix (bce: zthr)


def _kd_head(a, o):  # the teacher's rows sit before the labels
    return a.head + (a.teacher.data_ptr(), a.teacher.shape[3], o.Ht, o.Wt) + a.labels


def _kd_opts(a, o):
    return (a.w, o.ce, o.kd, o.temperature, int(o.kd_ignored))


def _bce_opts(o):
    return (o.pos_weight, o.bce, o.dice, o.focal_gamma)


def _bce_zthr(o):
    from .losses import logit_threshold
    return (logit_threshold(o.threshold),)


# opt: cew (eps, reduction), sl (eps, ce, dice, focal_gamma, dice_smooth), ohem (tau, min_kept), kd a Distill,
# bce a Binary
LOSS_FAMILIES = {f.stem: f for f in (
    LossFamily("ce", 3, True, None, 1,
               lambda a, o: a.head + a.labels + a.out,
               lambda a, o: a.head + a.labels + a.out),
    LossFamily("cew", 4, True, None, 1,
               lambda a, o: a.head + a.labels + (a.w, o[0], REDUCTIONS[o[1]]) + a.out,
               lambda a, o: a.head + a.labels + (a.w, o[0]) + a.out),
    LossFamily("sl", 6, True, None, 1,  # the table of Dice coefficients behind the stats
               lambda a, o: a.head + a.labels + (a.w,) + tuple(o) + a.out + (a.table.data_ptr(),),
               lambda a, o: a.head + a.labels + (a.w,) + tuple(o[:4]) + a.out + (a.table.data_ptr(),)),
    LossFamily("ohem", 6, True, "", 1,  # the gradient reads the per-pixel losses back from the workspace
               lambda a, o: a.head + a.labels + (a.w,) + tuple(o) + a.out,
               lambda a, o: a.head + a.labels + (a.w, o[0], a.work.data_ptr()) + a.out),
    LossFamily("kd", 6, False, "_nchw", 2,
               lambda a, o: _kd_head(a, o) + _kd_opts(a, o) + a.out,
               lambda a, o: _kd_head(a, o) + _kd_opts(a, o) + a.out),
    # one logit: stats end in the Dice gradient's a and b; one float of gradient per pixel, so the plane always
    LossFamily("bce", 8, True, None, 2,
               lambda a, o: a.head + a.labels + _bce_opts(o) + (o.dice_smooth,) + a.out,
               lambda a, o: a.head + a.labels + _bce_opts(o) + a.out,
               True, _bce_zthr),
)}


class Loss(NamedTuple):
    """A fused loss's forward as its backward needs it (Run.loss)."""
    fam: LossFamily
    opt: tuple             # the family's options (LOSS_FAMILIES)
    work: torch.Tensor     # the forward's workspace
    table: object = None   # sl: the per-class Dice gradient coefficients, written by the loss's finalize


def _loss_args(run, ignore_index, out):
    """The argument groups of a fused-loss call at the run's current labels, class weights and teacher; out: the
    (work, stats) of a forward or the (grad_out, stats) of a gradient call."""
    prog, lo, L = run.prog, run.prog.logits, run.loss
    Ho, Wo = prog.out_hw
    return SimpleNamespace(head=(run.ptr(lo), lo.ld, prog.N, lo.H, lo.W, lo.C),
                           labels=(run.target.data_ptr(), Ho, Wo, ignore_index),
                           w=run.weight.data_ptr() if run.weight is not None else 0,
                           teacher=run.teacher, work=L.work, table=L.table,
                           out=(out.data_ptr(), run.stats.data_ptr()))


def _loss_forward(run, t, ignore_index, confusion=None, weight=None, label_smoothing=0.0, reduction="mean", sl=None):
    """Fused final upsample + CrossEntropy over the run's low-res logits: stats = [loss, count, #bad labels].
    confusion (int64 [C, C], "metrics" mode): the same pass also adds every valid pixel to
    confusion[label, argmax] (seg_ce_upsample_eval).  With class weights, label smoothing or reduction "sum"
    (loss_options) the seg_cew_* kernels run instead: stats = [loss, D, #bad labels, #valid], same first three slots.
    sl = (ce, dice, focal_gamma, dice_smooth) of a seg_amd.SegLoss: the seg_sl_* kernels, stats = [loss, D, #bad
    labels, #valid, F, Dice] and the table of per-class Dice gradient coefficients their gradient kernel reads.
    sl = Ohem(thresh, min_kept) of a seg_amd.OhemCELoss: the seg_ohem_* kernels, stats = [loss, D, #bad labels,
    #valid, #kept, cut]; their workspace starts with the per-pixel losses (4 B per pixel), which the gradient
    kernel reads back.
    sl = Distill(ce, kd, temperature, kd_ignored, Ht, Wt) of a seg_amd.DistillLoss: the seg_kd_* kernels over
    run.teacher (fp32 NHWC rows [N, Ht, Wt, round4(C)], a tape external like the class weights), stats = [loss, D,
    #bad labels, #valid, CE, KD].
    sl = Binary(bce, dice, focal_gamma, dice_smooth, pos_weight, threshold) of a seg_amd.BinarySegLoss: the seg_bce_*
    kernels over the model's one logit, stats = [loss, #valid, #bad labels, #valid, F, Dice, a, b]; confusion is then
    int64 [2, 2], confusion[label, z > zthr]."""
    prog, s = run.prog, run.stream
    Ho, Wo = prog.out_hw
    pixels = prog.N * Ho * Wo
    run.target, run.weight = t, weight
    if isinstance(sl, Distill):
        fam, opt = LOSS_FAMILIES["kd"], sl
    elif isinstance(sl, Binary):
        fam, opt = LOSS_FAMILIES["bce"], sl
    elif isinstance(sl, Ohem):
        from .losses import resolve_min_kept
        # tau: float64 here, a float in the kernels
        fam, opt = LOSS_FAMILIES["ohem"], (-math.log(sl.thresh), resolve_min_kept(sl.min_kept, pixels))
    elif sl is not None:
        fam, opt = LOSS_FAMILIES["sl"], (label_smoothing,) + tuple(sl)
    elif not _plain_loss(weight, label_smoothing, reduction):
        fam, opt = LOSS_FAMILIES["cew"], (label_smoothing, reduction)
    else:
        fam, opt = LOSS_FAMILIES["ce"], ()
    if confusion is not None and not fam.has_eval:
        raise ValueError("validation does not distil: evaluate the criterion's hard() term")
    run.stats = run.tmp(fam.nstats)
    table = run.tmp(64) if fam.stem == "sl" else None
    work = run.tmp(query(f"seg_{fam.stem}_workspace_floats", pixels))
    run.loss = Loss(fam, opt, work, table)
    args = fam.fwd(_loss_args(run, ignore_index, work), opt)
    if confusion is None:
        run.call(run.k(f"seg_{fam.stem}_upsample_loss"), *args, s)
    else:
        extra = fam.ev(opt) if fam.ev is not None else ()
        run.call(run.k(f"seg_{fam.stem}_upsample_eval"), *args, *extra, confusion.data_ptr(), s)
    return run.stats


def _loss_backward(run, g, ignore_index):
    """Gradient of the fused loss (g: [1] fp32 upstream gradient) through the whole program."""
    prog, lo, s = run.prog, run.prog.logits, run.stream
    N = prog.N
    Ho, Wo = prog.out_hw
    fam, opt = run.loss.fam, run.loss.opt
    # the bf16io twins of ohem and kd: the full-resolution gradient in fp32 NCHW, as behind the model's logits (bf16
    # rows would round every term of the low-resolution gradient's sums); bce: the plane in both maths (fam.plane)
    nchw = fam.plane or (run.io and fam.nchw is not None)
    if nchw:
        dhigh = torch.empty(max(N * lo.C * Ho * Wo, 1), device=run.device, dtype=torch.float32)
    else:
        dhigh = torch.empty(max(N * Ho * Wo * lo.ld, 1), device=run.device, dtype=run.store)
    run.keep.append(dhigh)
    ldh = () if nchw else (lo.ld,)
    run.call(run.k(f"seg_{fam.stem}_upsample_grad") + (fam.nchw if nchw and not fam.plane else ""),
             *fam.grad(_loss_args(run, ignore_index, g), opt), dhigh.data_ptr(), *ldh, s)
    run.call(run.k("seg_upsample_bwd"), dhigh.data_ptr(), 0 if nchw else lo.ld, int(nchw), N, Ho, Wo, lo.C,
             run.gptr(lo), lo.ld, lo.H, lo.W, fam.ac, 0, s)
    run.mark_written(lo)
    run.backward_from_logits()


class Plan:
    """One (input shape, mode) of a model compiled to two launch tapes (seg_amd/tape.py):
    the forward (weight repack, NCHW -> NHWC, every op, the fused loss or the NCHW logits;
    mode "metrics": the fused loss + confusion matrix of validation, and no backward tape)
    and the backward (loss / logits gradient, every op in reverse, parameter gradients on
    the side stream, DataParallel bucket all-reduces at host-callback stops).  Recorded
    by the first step -- a normal program walk with every launch captured instead of
    issued -- and replayed by the following ones with the caller's input / target /
    class-weight / output / upstream-gradient pointers patched in (label smoothing, the
    reduction, a SegLoss's four scalars, an OhemCELoss's two and a DistillLoss's four with the teacher tensor's geometry
    are part of the plan's key; the teacher's logits are an external like the class weights, patched per replay; the
    weight VALUES are read by the kernels each step; a SegLoss's stats and coefficient table are persistent buffers of the plan).  Buffers, workspaces, saved BN
    statistics and the flat parameter-gradient buffer are persistent (allocated while
    recording, ~13 GB at bs=32 256x512 fp32 -- nothing is recomputed).

    The replay issues the same launches on the same two streams as an eager walk, so
    results are bitwise those of the eager engine (tests/test_gpu_tape.py)."""

    def __init__(self, prog, training, mode, ignore_index, sync, needs_grad, device, label_smoothing=0.0,
                 reduction="mean", sl=None):
        self.prog, self.training, self.mode, self.ignore_index = prog, training, mode, ignore_index
        self.label_smoothing, self.reduction, self.sl = label_smoothing, reduction, sl
        self.sync, self.needs_grad, self.device = sync, needs_grad, device
        self.side = _side_stream(device) if (OVERLAP and needs_grad) else None
        self.run = self.fwd = self.bwd = None
        self.t = None            # the last forward's labels (loss mode)
        self.w = None            # the last forward's class weights (None: unweighted)
        self.tl = None           # the last forward's teacher logits (a DistillLoss; None otherwise)
        self.busy = False        # a forward whose backward has not run yet
        self.timer = None        # the KernelTimer the tapes' timing is armed for
        self.fp = None           # _fingerprint(prog) the tapes were recorded against

    def _streams(self):
        main = torch.cuda.current_stream(self.device).cuda_stream
        return main, (self.side.cuda_stream if self.side is not None else main)

    def _arm_timer(self, tape):
        if TIMER is not self.timer:
            for t in (self.fwd, self.bwd):
                if t is not None:
                    if self.timer is not None:
                        self.timer.collect(t)
                    t.time([], 0)
            self.timer = TIMER
        if TIMER is not None and tape not in TIMER.tapes:
            tape.time(TIMER.kinds, TIMER.max_replays)
            TIMER.tapes.append(tape)

    def forward(self, x, t, confusion=None, weight=None, teacher=None):
        from .tape import Recorder
        main, side = self._streams()
        N, _, H, W = x.shape
        Ho, Wo = self.prog.out_hw
        out = None
        if self.mode == "logits":
            out = torch.empty((N, self.prog.logits.C, Ho, Wo), device=x.device, dtype=torch.float32)
        elif self.mode == "low":  # the low-resolution logits as caller-owned fp32 NHWC rows (run_low_logits)
            lo = self.prog.logits
            out = torch.empty((N, lo.H, lo.W, (lo.C + 3) & ~3), device=x.device, dtype=torch.float32)
        if self.fwd is None:
            rec = Recorder({side: 1, main: 0})
            rec.external("x", x.data_ptr())
            if t is not None:
                rec.external("t", t.data_ptr())
            if out is not None:
                rec.external("out", out.data_ptr())
            if confusion is not None:
                rec.external("confusion", confusion.data_ptr())
            if weight is not None:
                rec.external("w", weight.data_ptr())
            if teacher is not None:
                rec.external("tl", teacher.data_ptr())
            run = Run(self.prog, x, self.training, rec=rec, side=self.side)
            run.sync = self.sync
            run.teacher = teacher
            if self.needs_grad:
                ps = [p for p in self.prog.params() if p.requires_grad]
                off = 0
                for p in ps:
                    run.flat_slots[id(p)] = (off, p.numel())
                    off += p.numel()
                run.flat = torch.empty(max(off, 1), device=x.device, dtype=torch.float32)
            run.forward()
            lo = self.prog.logits
            if self.mode == "logits":
                run.call(run.k("seg_upsample_to_nchw"), run.ptr(lo), lo.ld, N, lo.H, lo.W, lo.C, out.data_ptr(), Ho,
                         Wo, 1, run.stream)
            elif self.mode == "low":
                run.call(run.k("seg_low_logits_f32"), run.ptr(lo), lo.ld, N * lo.H * lo.W, lo.C, out.data_ptr(),
                         out.shape[3], run.stream)
            else:
                _loss_forward(run, t, self.ignore_index, confusion, weight, self.label_smoothing, self.reduction,
                              self.sl)
            run.rec = None
            self.run, self.fwd = run, rec.build()
        self._arm_timer(self.fwd)
        # the backward tape reads the labels, the weights and the teacher's logits: keep them alive until then
        self.t, self.w, self.tl = t, weight, teacher
        self.fwd.bind(x=x.data_ptr(), t=t.data_ptr() if t is not None else 0,
                      out=out.data_ptr() if out is not None else 0,
                      confusion=confusion.data_ptr() if confusion is not None else 0,
                      w=weight.data_ptr() if weight is not None else 0,
                      tl=teacher.data_ptr() if teacher is not None else 0)
        self.fwd.run(main, side)
        if DEBUG_KEEP_RUN:
            global LAST_RUN
            LAST_RUN = self.run
        return out

    def backward(self, gout):
        from .tape import Recorder
        run = self.run
        main, side = self._streams()
        if self.mode == "logits":
            g = gout.contiguous()
        else:
            g = gout.reshape(1).to(torch.float32).contiguous()
        if self.bwd is None:
            rec = Recorder({side: 1, main: 0})
            if self.sync is not None:
                self.sync.begin_record()
            rec.external("gout", g.data_ptr())
            if self.t is not None:
                rec.external("t", self.t.data_ptr())
                run.target = self.t
            if self.w is not None:
                rec.external("w", self.w.data_ptr())
                run.weight = self.w
            if self.tl is not None:
                rec.external("tl", self.tl.data_ptr())
                run.teacher = self.tl
            run.rec = rec
            if self.mode == "logits":
                prog, lo = self.prog, self.prog.logits
                Ho, Wo = prog.out_hw
                run.call(run.k("seg_upsample_bwd"), g.data_ptr(), 0, 1, prog.N, Ho, Wo, lo.C, run.gptr(lo), lo.ld,
                         lo.H, lo.W, 1, 0, run.stream)
                run.mark_written(lo)
                run.backward_from_logits()
            else:
                _loss_backward(run, g, self.ignore_index)
            run.rec = None
            self.bwd = rec.build()
        self._arm_timer(self.bwd)
        self.bwd.bind(gout=g.data_ptr(), t=self.t.data_ptr() if self.t is not None else 0,
                      w=self.w.data_ptr() if self.w is not None else 0,
                      tl=self.tl.data_ptr() if self.tl is not None else 0)
        self.bwd.run(main, side)
        if DEBUG_KEEP_RUN:
            global LAST_RUN
            LAST_RUN = run
        if self.sync is not None:
            self.sync.finish_gradient_sync()  # stream-ordered wait on the last all-reduces


def _fingerprint(prog):
    """Storage pointers of every tensor a plan's tapes point into: conv / BN parameters and
    BN running statistics.  A change (load_state_dict(assign=True), p.data = ..., .half(),
    DataParallel's flat BN buffers) invalidates the recorded tapes."""
    out = []  # read from the modules each time: a rebinding replaces the tensor object
    for op in prog.ops:
        if isinstance(op, ConvOp):
            c, b = op.conv, op.bn
            out += [c.weight.data_ptr(), c.bias.data_ptr() if c.bias is not None else 0]
            if b is not None:
                out += [t.data_ptr() if t is not None else 0
                        for t in (b.weight, b.bias, b.running_mean, b.running_var, b.num_batches_tracked)]
    return tuple(out)


# Launch plans kept per model (each holds its buffers: ~13 GB at bs=32 256x512 fp32, half in
# bf16io).  Least recently used plans beyond this are dropped; release_plans() drops all.
MAX_PLANS = int(os.environ.get("SEG_MAX_PLANS", "4"))


def release_plans(model):
    """Drop every recorded plan (tapes + persistent buffers) of `model`; the next step
    re-records.  Frees the plan memory, e.g. after evaluating at another resolution."""
    model = getattr(model, "module", model)
    model.__dict__.pop("_segamd_plans", None)


def _plan(model, prog, mode, ignore_index, sync, needs_grad, device, opts=(None, 0.0, "mean", None)):
    """opts: loss_options().  The weight tensor itself is no part of the key (only whether there is one): its
    pointer is patched into the tapes per replay, so new weight values or a new weight tensor need no new plan."""
    cache = model.__dict__.setdefault("_segamd_plans", {})
    weight, eps, reduction, sl = opts
    # a DataParallel wrapper re-plans its buckets when the requires_grad pattern changes (its generation): the tapes
    # of an earlier generation point into buckets that are gone
    key = (id(prog), mode, model.training, ignore_index, (id(sync), sync.generation) if sync is not None else None,
           needs_grad, OVERLAP, (eps, reduction, weight is None, sl), plan_signature(prog))
    fp = _fingerprint(prog)
    plan = cache.pop(key, None)  # re-inserted below: dict order = least recently used first
    if plan is None or plan.sync is not sync or plan.fp != fp:
        if plan is not None and plan.busy:
            raise RuntimeError("segamd: parameters or buffers were rebound between a forward and its backward")
        plan = Plan(prog, model.training, mode, ignore_index, sync, needs_grad, device, eps, reduction, sl)
        plan.fp = fp
    cache[key] = plan
    while len(cache) > max(MAX_PLANS, 1):
        old = next(k for k in cache)
        if cache[old].busy:  # its backward is still to come: keep it (and stop evicting)
            break
        del cache[old]
    if plan.busy:
        # a second forward before this plan's backward ran: a one-off plan keeps the first
        # forward's activations intact (recorded and run once, then dropped)
        plan = Plan(prog, model.training, mode, ignore_index, sync, needs_grad, device, eps, reduction, sl)
        plan.fp = fp
    return plan


def _publish_stats(model, stats):
    """A fused loss has run: remember its stats buffer for bad_label_count / check_targets, start
    the host copy of the out-of-range label count, and return the loss as a tensor of its own."""
    model.__dict__["_segamd_last_stats"] = stats
    out = stats[0].clone()  # the stats buffer is rewritten by the next step
    # the out-of-range label count, copied to the host as soon as the loss kernel has run:
    # train_one_epoch reads it before optimizer.step() without waiting for the backward
    # (on the stats tensor's device and stream: the model need not be on the current device)
    dev = stats.device
    host = model.__dict__.get("_segamd_bad_host")
    if host is None or host[2] != dev:
        host = (torch.zeros(1, dtype=torch.float32).pin_memory(), torch.cuda.Event(), dev)
        model.__dict__["_segamd_bad_host"] = host
    with torch.cuda.device(dev):
        host[0].copy_(stats[2:3], non_blocking=True)
        host[1].record(torch.cuda.current_stream(dev))
    return out


class _SegFunction(torch.autograd.Function):
    """Whole-network forward/backward as one autograd node (replaying the plan's tapes)."""

    @staticmethod
    def forward(ctx, model, mode, x, target, ignore_index, sync, opts, *params):
        x = x.contiguous()
        N, _, H, W = x.shape
        prog = get_program(model, N, H, W)
        Ho, Wo = prog.out_hw
        t = None
        if mode == "loss":
            t = target.contiguous()
            if t.dtype != torch.int64 or tuple(t.shape) != (N, Ho, Wo):
                raise ValueError(f"target must be int64 [{N},{Ho},{Wo}], got {tuple(t.shape)} {t.dtype}")
        needs_grad = any(ctx.needs_input_grad[7:])
        teacher = None
        if mode == "loss":
            weight, eps, reduction, sl = opts[:4]
            tl = opts[4] if len(opts) > 4 else None  # run_loss: a DistillLoss's teacher logits
            opts = loss_options(weight, eps, reduction, prog.logits.C, x.device, *(sl or ()))
            if isinstance(opts[3], Distill):
                Ht, Wt = check_teacher_logits(tl, N, prog.logits.C, x.device)
                opts = (*opts[:3], opts[3]._replace(Ht=Ht, Wt=Wt))
                teacher = tl
            elif tl is not None:
                raise ValueError("teacher_logits given without kd > 0")
        plan = _plan(model, prog, mode, ignore_index, sync, needs_grad, x.device, opts)
        out = plan.forward(x, t, weight=opts[0], teacher=teacher)
        if mode == "loss":
            out = _publish_stats(model, plan.run.stats)
        else:  # an unfused criterion checks its own labels: no stale flag from an earlier fused loss
            model.__dict__.pop("_segamd_last_stats", None)
            model.__dict__.pop("_segamd_bad_host", None)
        if needs_grad:
            plan.busy = True
            ctx.plan, ctx.params = plan, params
        else:
            ctx.plan = None
        return out

    @staticmethod
    def backward(ctx, gout):
        plan = ctx.plan
        if plan is None:
            raise RuntimeError("segamd: backward called on a forward that saved nothing")
        try:
            plan.backward(gout)
        finally:
            plan.busy = False
        run = plan.run
        if run.sync is not None:  # DataParallel: copies of the averaged buckets, never the buckets
            grads = run.sync.autograd_grads(ctx.params)
        else:
            # one copy of the flat gradient buffer (the next backward rewrites it): a .grad
            # never aliases engine memory, and AccumulateGrad adopts the views as they are
            flat = run.flat.clone()
            grads = []
            for p in ctx.params:
                slot = run.flat_slots.get(id(p)) if id(p) in run.grads else None
                grads.append(flat[slot[0]:slot[0] + slot[1]].view_as(p) if slot else None)
        grads = [g if ctx.needs_input_grad[7 + k] else None for k, g in enumerate(grads)]
        ctx.plan = ctx.params = None
        return (None, None, None, None, None, None, None, *grads)


def bad_label_count(model):
    """Device tensor [1] (fp32): the number of labels outside [0, C) other than
    ignore_index seen by `model`'s last fused loss, or None (no fused loss yet).  Reading it
    is one host sync; train_one_epoch reads it (summed over ranks) before optimizer.step()."""
    model = getattr(model, "module", model)
    st = model.__dict__.get("_segamd_last_stats")
    return None if st is None else st[2:3].clone()


def label_flag(model):
    """Device tensor [1] (fp32) that is non-zero iff the last fused loss saw a label outside [0, C) other than
    ignore_index -- on ANY rank under seg_amd.ddp.DataParallel (the count rides in the last gradient bucket's
    all-reduce: valid in stream order after finish_gradient_sync, no extra collective); None when there is no fused
    loss to check (or, under DataParallel, when this step's buckets did not go out)."""
    sync = getattr(model, "label_flag", None)
    if sync is not None:  # DataParallel
        return sync()
    model = getattr(model, "module", model)
    st = model.__dict__.get("_segamd_last_stats")
    return None if st is None else st[2:3]


def bad_label_count_host(model):
    """The out-of-range label count of `model`'s last fused loss as a host int, or None: waits
    only for that forward's loss kernel (an event recorded behind its device-to-host copy), not
    for the backward queued after it, so the host keeps running ahead of the GPU."""
    model = getattr(model, "module", model)
    host = model.__dict__.get("_segamd_bad_host")
    if host is None or model.__dict__.get("_segamd_last_stats") is None:
        return None
    host[1].synchronize()
    return int(host[0].item())


def check_targets(model, bad=None):
    """Raise like nn.CrossEntropyLoss ("Target out of bounds") if the last fused loss of
    `model` saw a label outside [0, C) other than ignore_index.  The kernels flag it
    stream-ordered (the loss and every gradient become NaN); this reads the flag (one
    host sync).  bad: an already-gathered count (e.g. summed over ranks)."""
    if bad is None:
        bad = bad_label_count(model)
    n = 0 if bad is None else int(bad.item())
    if n:
        raise IndexError(f"Target out of bounds: {n} label(s) outside [0, num_classes) that are not "
                         "ignore_index (nn.CrossEntropyLoss raises on these)")


def _params_for(model, x):
    N, _, H, W = x.shape
    return get_program(model, N, H, W).params()


def run_logits(model, x: torch.Tensor) -> torch.Tensor:
    _check_input(x)
    sync = model.__dict__.get("_segamd_sync")
    return _SegFunction.apply(model, "logits", x, None, IGNORE_INDEX, sync, (None, 0.0, "mean", None),
                              *_params_for(model, x))


def run_loss(model, x: torch.Tensor, target: torch.Tensor, ignore_index: int = IGNORE_INDEX, weight=None,
             label_smoothing: float = 0.0, reduction: str = "mean", ce: float = 1.0, dice: float = 0.0,
             focal_gamma: float = 0.0, dice_smooth: float = 1.0, ohem_thresh=None,
             ohem_min_kept=None, kd: float = 0.0, kd_temperature: float = 1.0, kd_ignored: bool = True,
             teacher_logits=None, binary: bool = False, pos_weight: float = 1.0) -> torch.Tensor:
    """nn.CrossEntropyLoss(weight, ignore_index=..., reduction=..., label_smoothing=...)(model(x), target),
    seg_amd.SegLoss(ce, dice, focal_gamma, weight, ...)(model(x), target) or seg_amd.OhemCELoss(ohem_thresh,
    ohem_min_kept, weight, ...)(model(x), target), with the loss fused into the final upsample
    (csrc/loss.hip); the options are checked by loss_options (ValueError).  With kd > 0 and teacher_logits (a teacher's
    forward_low_logits(x): float32 [N, Ht, Wt, round4(C)]) the loss is seg_amd.DistillLoss(teacher, ce, kd,
    kd_temperature, weight, ignore_index, kd_ignored)'s, the teacher's logits upsampled inside the same kernels
    (seg_kd_*); the tensor is read by the forward and by the backward and may be a new one every step.  With
    binary=True the loss is seg_amd.BinarySegLoss(bce=ce, dice, focal_gamma, pos_weight, ignore_index, dice_smooth)'s
    over the model's one logit (seg_bce_*); the target may then be [N, 1, Ho, Wo] and of any integer or bool dtype."""
    _check_input(x)
    sync = model.__dict__.get("_segamd_sync")
    opts = (weight, label_smoothing, reduction, (ce, dice, focal_gamma, dice_smooth, ohem_thresh, ohem_min_kept))
    if binary:
        from .losses import binary_target
        if teacher_logits is not None:
            raise ValueError("binary=True does not combine with distillation")
        target = binary_target(None, target)
        opts = (*opts[:3], (*opts[3], kd, kd_temperature, kd_ignored, True, pos_weight))
    elif kd != 0.0 or teacher_logits is not None:  # the defaults keep the tuple (and the code path) they always had
        opts = (*opts[:3], (*opts[3], kd, kd_temperature, kd_ignored), teacher_logits)
    return _SegFunction.apply(model, "loss", x, target, ignore_index, sync, opts, *_params_for(model, x))


@torch.no_grad()
def run_low_logits(model, x: torch.Tensor) -> torch.Tensor:
    """The NHWC logits in front of the final upsample as a caller-owned float32 tensor [N, Hl, Wl, round4(C)] (the
    pad channels 0): a forward-only plan (mode "low") that ends in seg_low_logits_f32 -- no full-resolution tensor is
    formed, in any conv math.  What a seg_amd.DistillLoss's teacher hands to run_loss as teacher_logits."""
    _check_input(x)
    x = x.contiguous()
    N, _, H, W = x.shape
    prog = get_program(model, N, H, W)
    plan = _plan(model, prog, "low", IGNORE_INDEX, None, False, x.device)
    return plan.forward(x, None)


@torch.no_grad()
def run_metrics(model, x: torch.Tensor, target: torch.Tensor, confusion: torch.Tensor,
                ignore_index: int = IGNORE_INDEX, weight=None, label_smoothing: float = 0.0,
                reduction: str = "mean", ce: float = 1.0, dice: float = 0.0, focal_gamma: float = 0.0,
                dice_smooth: float = 1.0, ohem_thresh=None, ohem_min_kept=None, binary: bool = False,
                pos_weight: float = 1.0, threshold: float = 0.5) -> torch.Tensor:
    """Validation forward: the fused loss of run_loss, and in the same kernel
    confusion[label, argmax of the full-resolution logits] += 1 for every valid pixel
    (csrc/loss.hip: seg_ce_upsample_eval, seg_cew_upsample_eval with loss options, seg_sl_upsample_eval for a
    SegLoss's Dice / focal terms or seg_ohem_upsample_eval for an OhemCELoss -- they change the returned loss only,
    never the matrix, which counts every valid pixel).  With binary=True (a seg_amd.BinarySegLoss over a one-logit
    model: seg_bce_upsample_eval) the matrix is int64 [2, 2], confusion[label, z > log(threshold / (1 - threshold))].
    A forward tape only: no gradient is ever built, so
    DataParallel's buckets are not involved (sync is None).  Plans are keyed by model.training
    like the others: eval() uses the running statistics, train() the batch's."""
    _check_input(x)
    x = x.contiguous()
    N, _, H, W = x.shape
    prog = get_program(model, N, H, W)
    Ho, Wo = prog.out_hw
    C = prog.logits.C
    if binary:
        from .losses import binary_target
        target = binary_target(None, target)
    t = target.contiguous()
    if t.dtype != torch.int64 or tuple(t.shape) != (N, Ho, Wo) or t.device != x.device:
        raise ValueError(f"target must be int64 [{N},{Ho},{Wo}] on {x.device}, got {tuple(t.shape)} {t.dtype} "
                         f"on {t.device}")
    K = 2 if binary else C  # a one-logit model's matrix is [label, z > zthr]
    if (confusion.dtype != torch.int64 or tuple(confusion.shape) != (K, K) or confusion.device != x.device
            or not confusion.is_contiguous()):
        raise ValueError(f"confusion must be a contiguous int64 [{K},{K}] tensor on {x.device}, got "
                         f"{tuple(confusion.shape)} {confusion.dtype} on {confusion.device}")
    if binary:
        opts = loss_options(weight, label_smoothing, reduction, C, x.device, ce, dice, focal_gamma, dice_smooth,
                            ohem_thresh, ohem_min_kept, binary=True, pos_weight=pos_weight, threshold=threshold)
    else:
        opts = loss_options(weight, label_smoothing, reduction, C, x.device, ce, dice, focal_gamma, dice_smooth,
                            ohem_thresh, ohem_min_kept)
    plan = _plan(model, prog, "metrics", ignore_index, None, False, x.device, opts)
    plan.forward(x, t, confusion, opts[0])
    return _publish_stats(model, plan.run.stats)
