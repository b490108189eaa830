"""Static execution plans for the YOLOv8 / YOLO-MS detector graph on MI355X.

A plan is built once per (module, input shape, compute dtype, train/eval) by walking
the module tree (each yolov8 module implements ``emit``).  It records

* NHWC activation buffers (channel stride ``ld`` = round8(C)) laid out in one arena;
  every channel concatenation of the reference (C2f ``torch.cat`` at
  components.py:119, SPPF :146, neck yolov8_neck.py:79-91, head yolov8_head.py:122)
  is a *placement*: producers write at a channel offset of the consumer's buffer,
  so no copy kernel exists;
* a list of ops (ConvOp, BiasConvOp, UpsampleOp, SppfPoolOp, InputOp) whose
  forward/backward are launches of the hand-written HIP kernels in libyms.so.

Training: forward stores the pre-BN conv output z, BN batch statistics are fused in
the conv epilogue (per-tile partial sums) and finalised by one tiny kernel which also
updates running_mean/var exactly like nn.BatchNorm2d(eps=1e-3, momentum=0.03).
Backward walks the ops in reverse: BN+SiLU backward (two-pass reduction), dgrad and
wgrad implicit GEMMs, fp32 parameter gradients written into one flat arena (ordered
in backward-completion order so that data-parallel all-reduce buckets complete
contiguously -- see yms.dist).
"""
from __future__ import annotations

import ctypes
import dataclasses
import os

import torch

from . import _lib as L

ALIGN = 256
# (the BN backward finalize inside the reduce launch -- last-arriving block -- was measured slower,
# 19.5-19.7 ms separate vs 20.4-21.3 ms fused, profiles/r02_ab_bn_fused_priority_graph.txt: it puts one
# block's serial sum of the partial table on the critical path; the fused launch serves the head's
# bias gradients only, yms_bias_bwd)
BN_MOMENTUM = 0.03   # components.py:73
BN_EPS = 1e-3
# Options.head_group when YMS_HEAD_GROUP is unset: the forward only.  Grouping the backward as well
# shortens the head's main-stream span (1.76 -> 1.37 ms) but not the step, whose backward waits for the
# side stream's weight gradients (16.82 vs 16.93 ms/step, profiles/r07_head_group_ab.txt)
HEAD_GROUP_DEFAULT = 1


def r8(c):
    return (c + 7) // 8 * 8


def _al(x):
    return (x + ALIGN - 1) // ALIGN * ALIGN


@dataclasses.dataclass(frozen=True)
class Options:
    """Everything outside (module, input shapes, dtype, train/eval) that shapes a plan or the way it
    runs.  Read once per runner.get_plan call (read_options) and part of the plan-cache key: a plan
    keeps the record it was built under as plan.opts, and a changed switch builds a fresh plan."""
    stem: bool              # YMS_STEM=0: generic input pack + implicit-GEMM stem (Plan._find_stems)
    head_fuse: bool         # YMS_HEAD_FUSE=0: two ConvOps per head pair (Builder.sibling_convs)
    bnred: bool             # YMS_BNRED=0: every BN-backward reduce as its own pass (Plan._find_bnred)
    wgrad_tail_first: bool  # YMS_WGRAD_FIRST=0: no layer enqueues its weight gradient first (Plan)
    grad_inplace: bool      # YMS_GRAD_INPLACE=0: always copy the incoming output gradients (runner)
    wgrad_stream: bool      # YMS_WGRAD_STREAM=0: weight gradients and packs on the main stream (runner)
    # YMS_HEAD_GROUP: the head's independent levels run stage by stage as grouped launches (HeadGroup):
    # 0 off, 1 the forward only, 2 forward and backward
    head_group: int
    # YMS_BWD_SKIP=0: every op runs its backward, whatever its parameters and inputs need (Plan._find_backward)
    bwd_skip: bool
    # YMS_BN_FROZEN=0: the backward of an eval-mode BatchNorm as the three batch-statistics passes (running
    # statistics as mean_invstd, a zeroed coefficient table) instead of yms_bn_frozen_act_bwd
    bn_frozen: bool
    # the library's process-wide direct-conv route (yms_conv_direct_set): it changes
    # yms_conv_stats_rows and yms_conv_dgrad_bnred_rows, which size the plan's scratch
    direct: int


def read_options():
    """The only place the plan / runner switches are read from the environment and the library."""
    def on(name):
        return os.environ.get(name, "1") != "0"

    hg = os.environ.get("YMS_HEAD_GROUP", str(HEAD_GROUP_DEFAULT))
    if hg not in ("0", "1", "2"):
        raise RuntimeError(f"yms: YMS_HEAD_GROUP={hg!r}: expected 0 (off), 1 (forward) or 2 (forward + backward)")
    return Options(stem=on("YMS_STEM"), head_fuse=on("YMS_HEAD_FUSE"), bnred=on("YMS_BNRED"),
                   wgrad_tail_first=on("YMS_WGRAD_FIRST"), grad_inplace=on("YMS_GRAD_INPLACE"),
                   wgrad_stream=on("YMS_WGRAD_STREAM"), head_group=int(hg), bwd_skip=on("YMS_BWD_SKIP"),
                   bn_frozen=on("YMS_BN_FROZEN"), direct=L.lib().yms_conv_direct_set(-1))


class Buf:
    __slots__ = ("idx", "n", "h", "w", "ld", "name", "off", "zero", "needs_grad")

    def __init__(self, idx, n, h, w, ld, name, zero):
        self.idx, self.n, self.h, self.w, self.ld, self.name, self.zero = idx, n, h, w, ld, name, zero
        self.off = None
        self.needs_grad = True

    @property
    def npix(self):
        return self.n * self.h * self.w


class View:
    __slots__ = ("buf", "off", "c")

    def __init__(self, buf, off, c):
        self.buf, self.off, self.c = buf, off, c

    def slot(self, k, c):
        """Channel sub-view [off + k, off + k + c) (8-aligned: the kernels move 16-B chunks)."""
        if (self.off + k) % 8:
            raise RuntimeError(f"yms: channel slice at offset {self.off + k} is not a multiple of 8")
        return View(self.buf, self.off + k, c)

    @property
    def h(self):
        return self.buf.h

    @property
    def w(self):
        return self.buf.w


class Layout:
    """Arena allocator used while finalising a plan (byte offsets)."""

    def __init__(self):
        self.size = 0

    def alloc(self, nbytes):
        off = self.size
        self.size += _al(max(int(nbytes), 1))
        return off


def _overlap(a, b):
    return a.buf is b.buf and a.off < b.off + b.c and b.off < a.off + a.c


def _opt(ptr, v):
    """(address, channel stride, channel offset) launch arguments of an optional view (ptr: rt.a / rt.g)."""
    return (ptr(v), v.buf.ld, v.off) if v is not None else (None, 0, 0)


def _check_not_in_place(op, y):
    """GradTracker.release(y) clears y's gradient interval once its producer has taken it, so an
    earlier writer of that memory stores instead of accumulating.  That is only sound when no
    input of the same op lives in y's channels (an in-place op would lose its input's gradient):
    every op's inputs are checked here."""
    for name, v in vars(op).items() if hasattr(op, "__dict__") else ():
        vs = v if isinstance(v, (list, tuple)) else (v,)
        for u in vs:
            if isinstance(u, View) and u is not y and name != "y" and _overlap(u, y):
                raise RuntimeError(f"yms: {type(op).__name__}.{name} overlaps its output (in-place op)")


class GradTracker:
    """Backward-order simulation deciding, for every write into an activation-gradient slice,
    whether it is the first one (plain store) or must accumulate; buffers that are read
    before any write (or carry zero-padded channels) are zeroed once per backward."""

    def __init__(self):
        self.written = {}
        self.zero = set()
        self.writes = None       # buffers any op writes a gradient into (recorded after the seeds)

    def _iv(self, v):
        return v.off, v.off + v.c

    def _covered(self, v):
        lo, hi = self._iv(v)
        ivs = sorted(self.written.get(v.buf.idx, []))
        cur = lo
        for a, b in ivs:
            if a <= cur < b:
                cur = b
            if cur >= hi:
                return True
        return cur >= hi

    def _touch(self, v):
        lo, hi = self._iv(v)
        return any(a < hi and lo < b for a, b in self.written.get(v.buf.idx, []))

    def _zero_buf(self, v):
        self.zero.add(v.buf.idx)
        self.written[v.buf.idx] = [(0, v.buf.ld)]

    def read(self, v):
        if not self._covered(v):
            self._zero_buf(v)

    def release(self, v):
        """The producer of v has taken its gradient (backward order): the slice's gradient is dead,
        so a later (earlier-in-forward) writer of the same memory stores instead of accumulating.
        Only matters where one buffer slice holds two tensors in turn (MSBlock: Y_{i+1} written over
        X_{i+1}); buffers with zeroed padding always accumulate and are never reused that way."""
        if v.buf.zero:
            return
        lo, hi = self._iv(v)
        out = []
        for a, b in self.written.get(v.buf.idx, []):
            if b <= lo or a >= hi:
                out.append((a, b))
                continue
            if a < lo:
                out.append((a, lo))
            if b > hi:
                out.append((hi, b))
        self.written[v.buf.idx] = out

    def write(self, v):
        """-> accumulate flag (0 = first writer, plain store)."""
        if self.writes is not None:
            self.writes.add(v.buf.idx)
        if v.buf.zero:                       # padded channels must stay zero: zero whole buffer
            if v.buf.idx not in self.zero:
                self._zero_buf(v)
            return 1
        if not self._touch(v):
            self.written.setdefault(v.buf.idx, []).append(self._iv(v))
            return 0
        if not self._covered(v):
            self._zero_buf(v)
        return 1


class Rt:
    """Per-call runtime state."""

    def __init__(self, plan, base, stream, training):
        self.plan = plan
        self.base = base
        self.gbase = None
        self.st = stream
        self.training = training
        self.pg_base = None      # flat fp32 param-grad arena pointer
        self.eval_base = None    # eval cache base pointer (packed weights + folded BN)
        self.prepacked = False   # training: all weight packs already issued (Plan.prepack)
        self.stem_x = {}         # plan input index -> NCHW fp32 tensor read by a stem ConvOp
        self._ev = None          # wst(): main -> side ordering event
        self.main = None         # backward: torch stream objects (main, weight-gradient side stream)
        self.side = None
        self.gover = None        # backward: buffer idx -> incoming output-gradient tensor used in place
        self.pgrad = None        # backward: parameter index -> address of its fp32 gradient (None: frozen)

    def a(self, v):
        return self.base + v.buf.off

    def g(self, v):
        o = self.gover.get(v.buf.idx) if self.gover else None
        return o if o is not None else self.gbase + v.buf.off

    def cnt(self, i):
        """Arrival counter i of the in-launch BN-backward finalize (zeroed at backward start)."""
        return self.gbase + self.plan.gscratch["cnt"] + 16 * i

    def wst(self):
        """Stream for a weight-gradient GEMM (+ its split reduce): a side stream ordered after
        everything enqueued on the main stream so far.  wgrad is off the backward's critical
        path (only the optimizer consumes dw), so it overlaps the next layers' HBM-bound BN
        backward kernels and dgrads.  Only wgrads use the side stream, so the shared
        "wgrad" scratch stays in stream order."""
        if self.side is None:
            return self.st
        # one reusable event (a wait binds the record made before it), not a new one per layer
        if self._ev is None:
            self._ev = torch.cuda.Event()
        self._ev.record(self.main)
        self.side.wait_event(self._ev)
        return self.side.cuda_stream


class Op:
    """What a plan asks of every op besides fwd / bwd / plan_grads; the default answer is nothing."""
    flops = 0
    # set per plan by Plan._find_backward
    runs_bwd = True     # the backward walk runs this op (a parameter of its own or an input needs a gradient)
    bn_eval = False     # its BatchNorm modules are in eval mode inside a training plan: running statistics
    infer = False       # bn_eval and no backward: the conv's epilogue writes y, there is no z

    def layout(self, plan, La, Le):
        pass

    def bn_modules(self):
        """The Conv blocks (.conv, .bn) whose BatchNorm this op runs."""
        return ()

    def eval_inputs(self):
        """The tensors prepare_eval reads: the eval cache is rebuilt when one of them changes."""
        return [t for m in self.bn_modules()
                for t in (m.conv.weight, m.bn.weight, m.bn.bias, m.bn.running_mean, m.bn.running_var)]

    def pack_specs(self):
        """(shape, fp32 weight, arena byte offset of the packed copy, for_dgrad[, (second weight,
        split)]) per training weight pack."""
        return ()

    def prepare_eval(self, rt):
        pass

    def z_padding(self, es):
        """(arena byte offset, bytes) of each training buffer that must start zeroed."""
        return ()

    def grad_params(self):
        return []


class ConvBase(Op):
    """The backward that ConvOp, SiblingConvOp, BiasConvOp and DWConvOp share: an input gradient on
    the main stream and a weight gradient on the side stream, from the same output gradient."""
    res = None
    stem_input = None           # plan input index when this conv reads the NCHW input directly
    tail_wgrad_first = False    # enqueue the weight gradient before the input gradient (Plan)
    WGRAD = "yms_conv_wgrad"

    def layout_eval(self, plan, Le):
        self.wp_elems = L.lib().yms_conv_packed_elems(self.sp, 0)
        self.wpt_elems = L.lib().yms_conv_packed_elems(self.sp, 1)
        self.e_wp = Le.alloc(self.wp_elems * plan.es)

    def layout_packs(self, plan, La):
        self.t_wp = La.alloc(self.wp_elems * plan.es)
        self.t_wpt = La.alloc(self.wpt_elems * plan.es) if self.runs_bwd else None

    def pack_specs(self):
        # (the transposed pack serves the input gradient: an op without a backward has none)
        w = self.conv.weight.data_ptr()
        return [(self.sp, w, self.t_wp, 0)] + ([(self.sp, w, self.t_wpt, 1)] if self.runs_bwd else [])

    def prepare_eval(self, rt):
        L.call("yms_conv_pack_weight", self.sp, self.conv.weight.data_ptr(), rt.eval_base + self.e_wp, 0, rt.st)

    def pack_unless_prepacked(self, rt):
        if not rt.prepacked:
            for sp, w, off, for_dgrad in self.pack_specs():
                L.call("yms_conv_pack_weight", sp, w, rt.base + off, for_dgrad, rt.st)

    def plan_grads(self, T):
        T.read(self.y)
        self.acc_res = T.write(self.res) if self.res is not None else 0
        self.acc_x = T.write(self.x) if self.x.buf.needs_grad else 0

    def conv_job(self, rt, out, ld, off, sc, sh, act, res, stats):
        """The conv into channels [off, off + c) of out, with scale / shift, act and residual in the
        epilogue (eval) or the batch-statistics table into stats (training: the pre-BN output)."""
        x = self.x
        wp = rt.base + self.t_wp if rt.training else rt.eval_base + self.e_wp
        return L.ConvFwdJob(self.shape, rt.a(x), x.buf.ld, x.off, wp, out, ld, off, sc, sh, act, *_opt(rt.a, res), stats)

    def dgrad_job(self, rt, dz, ld, off):
        x = self.x
        return L.ConvDgradJob(self.shape, dz, ld, off, rt.base + self.t_wpt, rt.g(x), x.buf.ld, x.off, self.acc_x)

    def dgrad(self, rt, dz, ld, off):
        L.call_job("yms_conv_dgrad", self.dgrad_job(rt, dz, ld, off), rt.st)

    def launch_wgrad(self, rt, dz, ld, off, dw):
        x = self.x
        L.call(self.WGRAD, self.sp, rt.a(x), x.buf.ld, x.off, dz, ld, off,
               rt.gbase + rt.plan.gscratch["wgrad"], self.wg_ws, dw, 0, rt.wst())

    def wgrad(self, rt, dz, ld, off):
        dw = rt.pgrad(self.pw)
        if dw is not None:
            self.launch_wgrad(rt, dz, ld, off, dw)

    def bwd_grads(self, rt, dz, ld, off, wgrad_first=False):
        """Input gradient, then weight gradient, of the output gradient in channels [off, ..) of dz.
        wgrad_first enqueues the weight gradient (side stream) BEFORE the input gradient, so the
        side stream's wait on the main stream ends at the BN apply, not after the dgrad: only for
        the layers whose input is the stem's output (Plan), the step's tail, where the main stream
        has nothing left but the stem's input-side chain and the side stream's last weight gradient
        otherwise starts after it."""
        if wgrad_first:
            self.wgrad(rt, dz, ld, off)
        if self.x.buf.needs_grad:
            self.dgrad(rt, dz, ld, off)
        if not wgrad_first:
            self.wgrad(rt, dz, ld, off)


class BNConvBase(ConvBase):
    """Training path of Conv2d -> BatchNorm2d -> act shared by ConvOp, SiblingConvOp and DWConvOp:
    the BN state's layout, the forward after the conv launch, and the BN + act backward."""
    bnred_by = None     # consumer whose input gradient computes this op's BN-backward reduce (ConvOp)

    def parts(self):
        """(conv block, channel offset of its output in this op's z) per convolution of the forward;
        each has conv_z, stats_rows and stats_ld."""
        return ((self, 0),)

    def init_block(self, b, mod, x, y, res, act):
        self.mod, self.conv, self.x, self.y, self.res, self.act = mod, mod.conv, x, y, res, act
        self.c = mod.conv.out_channels
        self.npix = b.n * y.h * y.w
        self.pw = b.param(mod.conv, "weight")
        self.pg = b.param(mod.bn, "weight")
        self.pb = b.param(mod.bn, "bias")

    def layout_bn(self, plan, La):
        """Training state over this op's c channels -- the pre-BN output z (the backward writes dz over
        it), the weight packs, scale / shift / (mean, invstd) -- and the scratch the forward's
        statistics tables (one per part), the BN backward and the weight gradient (wg_ws) need."""
        c = self.c
        self.zld = r8(c)
        self.z = None if self.infer else La.alloc(self.npix * self.zld * plan.es)
        self.layout_packs(plan, La)
        self.sc = La.alloc(4 * c)
        self.sh = La.alloc(4 * c)
        self.mi = La.alloc(8 * c)
        self.bwd_rows = L.lib().yms_bn_bwd_rows(self.npix, c)
        if not self.bn_eval:
            for m, _ in self.parts():
                plan.need_scratch("stats", 4 * m.stats_rows * (2 * m.stats_ld + 1))
        if not self.runs_bwd:
            return
        plan.need_scratch("bwd", 4 * 2 * c * self.bwd_rows)
        plan.need_scratch("coef", 8 * c)
        plan.need_scratch("wgrad", self.wg_ws)
        if self.bn_eval:
            plan.need_scratch("zcoef", 8 * c)      # the three-pass route's all-zero coefficients
            self.fz_cnt = plan.counter()           # the one-pass route's arrival counter

    def z_padding(self, es):
        # z buffers with padding channels (c % 8 != 0, e.g. a head with nc = 3): the convs and the BN
        # apply (dz written over z) touch only the c real channels, while the input gradient reads
        # the whole 16-B groups -- padding left as arena garbage (NaN / Inf bit patterns) times the
        # zero weight rows is NaN, so those z buffers start zeroed and their padding stays zero
        return [(self.z, self.npix * self.zld * es)] if self.zld != self.c and self.z is not None else []

    # ---- job records (include/yms.h) of this op's passes: its own fwd / bwd call the solo entry points
    # with them, a HeadGroup collects its members' into grouped calls.  grp: as a member of a group, in the
    # op's own slices (g_stats, g_bwd, g_coef: HeadGroup.layout) of the shared scratch regions.
    def conv_args(self, rt, grp=False):
        """(part, its conv_fwd / conv_job arguments) per conv: training into its channels of z with the
        statistics table, eval into its output with the folded BN + act (+ residual) epilogue."""
        if not rt.training:
            eb = rt.eval_base
            return [(m, (rt.a(m.y), m.y.buf.ld, m.y.off, eb + m.e_sc, eb + m.e_sh, m.act, m.res, None))
                    for m, _ in self.parts()]
        if self.infer:      # eval-mode BN, no backward: as the eval plan, with this step's folded scale / shift
            sc, sh = rt.base + self.sc, rt.base + self.sh
            return [(m, (rt.a(m.y), m.y.buf.ld, m.y.off, sc + 4 * off, sh + 4 * off, m.act, m.res, None))
                    for m, off in self.parts()]
        z, st = rt.base + self.z, rt.base + rt.plan.scratch["stats"]
        return [(m, (z, self.zld, off, None, None, L.ACT_NONE, None,
                     None if self.bn_eval else st + (m.g_stats if grp else 0)))
                for m, off in self.parts()]

    def fold_jobs(self):
        """Eval-mode BN: per part, the fold of its running statistics into this op's scale / shift /
        (running_mean, invstd) slots -- Plan.prepack runs them all in one launch per step."""
        return [L.BnFoldJob(bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                            bn.running_var.data_ptr(), bn.eps, m.c, self.c, self.sc + 4 * off, self.sh + 4 * off,
                            self.mi + 4 * off)
                for m, off in (self.parts() if self.bn_eval else ()) for bn in (m.mod.bn,)]

    def fold_own(self, rt):
        """The solo folds, on rt.st: without the batched prepack, and always for a stem -- the runner issues
        the prepack on the side stream and runs the stem's forward on the main stream before joining the
        two, so the stem's coefficients must not come from the side stream (Plan.fold_table leaves it out)."""
        if not rt.prepacked or self.stem_input is not None:
            for j in self.fold_jobs():
                L.call("yms_bn_fold_mi", j.c, j.gamma, j.beta, j.rmean, j.rvar, ctypes.c_float(j.eps),
                       rt.base + j.scale, rt.base + j.shift, rt.base + j.mean_invstd, j.mi_ld, rt.st)

    def finalize_jobs(self, rt, grp=False):
        """Per part, into its channel slot of this op's state (mean / invstd rows are self.c apart)."""
        if self.bn_eval:
            return []
        st, sc, sh, mi = (rt.base + o for o in (rt.plan.scratch["stats"], self.sc, self.sh, self.mi))
        return [L.BnFinalizeJob(m.c, st + (m.g_stats if grp else 0), m.stats_rows, m.stats_ld, self.npix,
                                bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                                bn.running_var.data_ptr(), bn.momentum if bn.momentum is not None else BN_MOMENTUM,
                                bn.eps, mi + 4 * off, self.c, sc + 4 * off, sh + 4 * off)
                for m, off in self.parts() for bn in (m.mod.bn,)]

    def pass_job(self, rt, **more):
        """z, scale / shift and act, which the affine, reduce and apply passes share."""
        base = rt.base
        return L.BnPassJob(npix=self.npix, c=self.c, z=base + self.z, z_ld=self.zld, z_off=0, scale=base + self.sc,
                           shift=base + self.sh, act=self.act, **more)

    def affine_job(self, rt):
        y = self.y
        res, res_ld, res_off = _opt(rt.a, self.res)
        return self.pass_job(rt, out=rt.a(y), out_ld=y.buf.ld, out_off=y.off, res=res, res_ld=res_ld, res_off=res_off)

    def bwd_jobs(self, rt, dg, db, grp=False):
        """-> the reduce, finalize (dgamma -> dg, dbeta -> db) and apply (dz over z, + the residual's
        gradient) records.  The partial rows are the reduce pass's -- or already written by the consumer's
        input gradient (bnred_by), its last writer, and the reduce record is not launched."""
        y, gb, gs = self.y, rt.gbase, rt.plan.gscratch
        coef = gb + gs["coef"] + (self.g_coef if grp else 0)
        ws, rows = gb + gs["bwd"] + (self.g_bwd if grp else 0), self.bwd_rows
        if self.bnred_by is not None:
            ws, rows = gb + gs[self.bnred_key], self.bnred_rows
        fcoef = coef
        if self.bn_eval:
            # running statistics: dz = scale * (da - 0 - xhat * 0), so the finalize writes no coefficients
            # and the apply reads a table of zeros
            fcoef, coef = None, gb + gs["zcoef"]
        gy = dict(gy=rt.g(y), gy_ld=y.buf.ld, gy_off=y.off, mean_invstd=rt.base + self.mi)
        res, res_ld, res_off = _opt(rt.g, self.res)
        return (self.pass_job(rt, ws=ws, **gy), L.BnBwdFinalizeJob(self.c, ws, rows, self.npix, dg, db, fcoef),
                self.pass_job(rt, coef=coef, out=rt.base + self.z, out_ld=self.zld, out_off=0, res=res, res_ld=res_ld,
                              res_off=res_off, res_acc=self.acc_res, **gy))

    def dz(self, rt):       # (address, channel stride, channel offset) of the output gradient after the apply pass
        return rt.base + self.z, self.zld, 0

    def bn_grads(self, rt):
        return rt.pgrad(self.pg), rt.pgrad(self.pb)

    def fwd(self, rt):
        """Training: each part's conv with its batch statistics finalised before the next part reuses the
        statistics scratch, then one affine + act (+ residual) pass z -> y."""
        fins = self.finalize_jobs(rt) if rt.training else ()
        for i, (m, args) in enumerate(self.conv_args(rt)):
            m.conv_fwd(rt, *args)
            if fins:
                L.call_job("yms_bn_finalize" if m is self else "yms_bn_finalize_ld", fins[i], rt.st)
        if rt.training and not self.infer:
            L.call_job("yms_affine_act", self.affine_job(rt), rt.st, rt.plan.dt)

    def one_pass(self, sums):
        """Eval-mode BN: does yms_bn_frozen_act_bwd serve this layer's backward?  Always as a plain streaming
        pass (1.8-2.1x the three passes); with dgamma / dbeta wanted, its last block sums the rows * 2c partial
        table alone, which pays where that table is small (the fused reduce's bound) or the tensor large:
        (25600, 256) measured 47 us against the three passes' 41, the four other layer shapes 1.2-1.45x
        faster (profiles/bn_frozen_bwd_micro.txt)."""
        return not sums or self.bwd_rows * self.c <= 32768 or self.npix * self.c >= 1 << 23

    def frozen_bwd(self, rt, dg, db):
        """Eval-mode BN: the whole BN + act backward as one launch -> dz."""
        y, gb, gs = self.y, rt.gbase, rt.plan.gscratch
        res, res_ld, res_off = _opt(rt.g, self.res)
        job = self.pass_job(rt, gy=rt.g(y), gy_ld=y.buf.ld, gy_off=y.off, mean_invstd=rt.base + self.mi,
                            out=rt.base + self.z, out_ld=self.zld, out_off=0, res=res, res_ld=res_ld, res_off=res_off,
                            res_acc=self.acc_res, ws=gb + gs["bwd"], counter=rt.cnt(self.fz_cnt))
        L.call("yms_bn_frozen_act_bwd", *L.job_args("yms_bn_frozen_act_bwd", job, rt.plan.dt), dg, db, rt.st)
        return self.dz(rt)

    def bn_bwd(self, rt, dg, db):
        """The reduce (unless bnred_by) and finalize passes -> the apply record, for bn_bwd_apply."""
        red, fin, app = self.bwd_jobs(rt, dg, db)
        if self.bn_eval and dg is None and db is None:
            return app          # running statistics, gamma and beta frozen: nothing to sum, the apply alone gives dz
        if self.bnred_by is None:
            L.call_job("yms_bn_act_bwd_reduce", red, rt.st, rt.plan.dt)
        L.call_job("yms_bn_act_bwd_finalize", fin, rt.st)
        return app

    def bn_bwd_apply(self, rt, app):
        L.call_job("yms_bn_act_bwd_apply", app, rt.st, rt.plan.dt)
        return self.dz(rt)


class ConvOp(BNConvBase):
    """Conv block = Conv2d(bias=False) -> BatchNorm2d -> SiLU/Identity (+ residual),
    components.py:69-77 (residual: Bottleneck :87-93)."""

    def __init__(self, b, mod, x, y, res, act):
        conv = mod.conv
        if conv.groups != 1 or conv.dilation != (1, 1) or conv.kernel_size[0] != conv.kernel_size[1]:
            raise RuntimeError("yms: only square, ungrouped, undilated convolutions are supported")
        if conv.stride[0] != conv.stride[1] or conv.padding[0] != conv.padding[1]:
            raise RuntimeError("yms: anisotropic stride/padding unsupported")
        k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        self.init_block(b, mod, x, y, res, act)
        self.shape = L.ConvShape(b.n, x.h, x.w, conv.in_channels, conv.out_channels, k, s, p,
                                 y.h, y.w, b.dt)
        self.sp = ctypes.pointer(self.shape)
        self.flops = 2 * self.npix * self.c * conv.in_channels * k * k
        self.bnred_for = None    # producer whose BN-backward reduce this conv's input gradient computes
        self.bnred_by = None     # consumer whose input gradient computes this conv's BN-backward reduce
        self.bnred_key = None    # grad-scratch region of the partial rows of THIS conv's reduce
        self.bnred_wkey = None   # grad-scratch region this conv's input gradient writes (its producer's)

    def layout(self, plan, La, Le):
        # eval cache: packed fwd weights + folded scale/shift
        self.layout_eval(plan, Le)
        self.e_sc = Le.alloc(4 * self.c)
        self.e_sh = Le.alloc(4 * self.c)
        if plan.training:
            stem = self.stem_input is not None
            self.stats_rows = (L.lib().yms_conv_stem_stats_rows if stem else L.lib().yms_conv_stats_rows)(self.sp)
            self.stats_ld = L.lib().yms_conv_stats_ld(self.sp)
            self.wg_ws = L.lib().yms_conv_wgrad_ws_bytes(self.sp)
            self.layout_bn(plan, La)
            if stem:
                # its own scratch: the stem's wgrad runs on the MAIN stream while the side stream
                # may still be in the previous layers' wgrads, which share the "wgrad" scratch
                self.wg_ws = L.lib().yms_conv_stem_wgrad_ws_bytes(self.sp)
                plan.need_scratch("stemwg", self.wg_ws)

    def bn_modules(self):
        return (self.mod,)

    def prepare_eval(self, rt):
        super().prepare_eval(rt)
        self.fold_bn(rt)

    def fold_bn(self, rt):
        bn = self.mod.bn
        L.call("yms_bn_fold", self.c, bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
               bn.running_var.data_ptr(), ctypes.c_float(bn.eps), rt.eval_base + self.e_sc,
               rt.eval_base + self.e_sh, rt.st)

    def fwd(self, rt):
        if rt.training:
            self.pack_unless_prepacked(rt)
            self.fold_own(rt)
        super().fwd(rt)

    def conv_fwd(self, rt, out, ld, off, sc, sh, act, res, stats):
        if self.stem_input is None:
            return L.call_job("yms_conv_fwd", self.conv_job(rt, out, ld, off, sc, sh, act, res, stats), rt.st)
        L.call("yms_conv_stem_fwd", self.sp, rt.stem_x[self.stem_input].data_ptr(), self.conv.weight.data_ptr(),
               out, ld, off, sc, sh, act, stats, self.stats_ld if stats else 0, rt.st)

    def dgrad(self, rt, dz, ld, off):
        q = self.bnred_for
        if q is None:
            return super().dgrad(rt, dz, ld, off)
        # + the producer's BN-backward reduce in the epilogue (dx = the producer's final gy)
        base = rt.base
        L.call("yms_conv_dgrad_bnred", *L.job_args("yms_conv_dgrad", self.dgrad_job(rt, dz, ld, off)), base + q.z,
               q.zld, 0, base + q.sc, base + q.sh, base + q.mi, q.act, rt.gbase + rt.plan.gscratch[self.bnred_wkey], rt.st)

    def bwd(self, rt):
        dg, db = self.bn_grads(rt)
        if (self.bn_eval and self.stem_input is None and rt.plan.opts.bn_frozen
                and self.one_pass(dg is not None or db is not None)):
            return self.bwd_grads(rt, *self.frozen_bwd(rt, dg, db), self.tail_wgrad_first)
        app = self.bn_bwd(rt, dg, db)
        if self.stem_input is not None:
            # the stem's input needs no gradient: the apply pass is fused into the weight
            # gradient, which reads gy, z and the NCHW input.
            # It runs on the MAIN stream: the stem is the backward's last layer, so the main stream
            # is idle from here on while the side stream still drains the previous layers'
            # weight gradients -- the two then overlap instead of queueing (step tail 0.53 ms).
            dw = rt.pgrad(self.pw)
            if dw is not None:
                base, y = rt.base, self.y
                L.call("yms_conv_stem_wgrad", self.sp, rt.stem_x[self.stem_input].data_ptr(), rt.g(y), y.buf.ld,
                       y.off, base + self.z, self.zld, 0, base + self.sc, base + self.sh, base + self.mi, app.coef,
                       self.act, rt.gbase + rt.plan.gscratch["stemwg"], self.wg_ws, dw, 0, rt.st)
            return
        self.bwd_grads(rt, *self.bn_bwd_apply(rt, app), self.tail_wgrad_first)

    def grad_params(self):
        return [self.pb, self.pg, self.pw]


class SiblingConvOp(BNConvBase):
    """Two Conv blocks (Conv2d -> BN -> act, components.py:69-77) that read the SAME input view --
    the head's box[i][0] and cls[i][0] (yolov8_head.py:84-85, 99-100: Conv(c_i, 4*ch) and
    Conv(c_i, nc), both 3x3 of x_i) -- with their outputs as the two channel slots of one buffer
    [.., c_a | c_b].  The forward runs each member's conv (its own tile shape) into its slot of one
    z buffer and its own BN finalize; everything after is one pass over the c_a + c_b channels:
    ONE affine pass; in the backward ONE BN reduce / finalize / apply, ONE input gradient (a single
    GEMM with K = k^2 (c_a + c_b): dx is stored once instead of stored, re-read and accumulated by a
    second dgrad) and ONE weight gradient (M = c_a + c_b).  The members' parameter gradients are
    adjacent in the flat gradient arena (grad_params order), so the fused backward writes them in
    place; the transposed dgrad weight is packed from both fp32 weights by one pack job (w2 / split)."""

    def __init__(self, b, mods, x, y, act):
        self.x, self.y, self.res, self.act = x, y, None, act
        self.members, self.offs = [], []
        off = 0
        for m in mods:
            self.offs.append(off)
            self.members.append(ConvOp(b, m, x, y.slot(off, m.conv.out_channels), None, act))
            off += m.conv.out_channels
        self.c = off
        m0 = self.members[0]
        sh0 = m0.shape
        self.shape = L.ConvShape(sh0.n, sh0.h, sh0.w, sh0.cin, self.c, sh0.k, sh0.stride, sh0.pad, sh0.ho, sh0.wo, sh0.dtype)
        self.sp = ctypes.pointer(self.shape)
        self.npix = m0.npix
        self.flops = sum(m.flops for m in self.members)

    def parts(self):
        return zip(self.members, self.offs)

    def layout(self, plan, La, Le):
        es = plan.es
        for m in self.members:
            m.wp_elems = L.lib().yms_conv_packed_elems(m.sp, 0)
            m.e_wp = Le.alloc(m.wp_elems * es)
            m.e_sc = Le.alloc(4 * m.c)
            m.e_sh = Le.alloc(4 * m.c)
        if not plan.training:
            return
        for m in self.members:
            m.stats_rows = L.lib().yms_conv_stats_rows(m.sp)
            m.stats_ld = L.lib().yms_conv_stats_ld(m.sp)
            # the fallback when the members' weight gradients are not adjacent (some frozen): per member
            m.wg_ws = L.lib().yms_conv_wgrad_ws_bytes(m.sp)
            plan.need_scratch("wgrad", m.wg_ws)
        self.wpt_elems = L.lib().yms_conv_packed_elems(self.sp, 1)
        self.wg_ws = L.lib().yms_conv_wgrad_ws_bytes(self.sp)
        self.layout_bn(plan, La)
        # the same fallback for dgamma / dbeta: into scratch, then copied per member
        plan.need_scratch("sib", 8 * self.c)

    def layout_packs(self, plan, La):
        for m in self.members:
            m.t_wp = La.alloc(m.wp_elems * plan.es)
        self.t_wpt = La.alloc(self.wpt_elems * plan.es) if self.runs_bwd else None

    def pack_specs(self):
        specs = [(m.sp, m.mod.conv.weight.data_ptr(), m.t_wp, 0) for m in self.members]
        if not self.runs_bwd:
            return specs
        a, bb = self.members
        specs.append((self.sp, a.mod.conv.weight.data_ptr(), self.t_wpt, 1,
                      (bb.mod.conv.weight.data_ptr(), a.c)))
        return specs

    def prepare_eval(self, rt):
        for m in self.members:
            m.prepare_eval(rt)

    def bn_modules(self):
        return [m.mod for m in self.members]

    def fwd(self, rt):
        if rt.training and not rt.prepacked:
            raise RuntimeError("yms: sibling convs need the batched pack (Plan.prepack)")
        super().fwd(rt)             # (eval: BN + act fused in each member's epilogue, into its slot)

    def _adjacent(self, rt, attr):
        ps = [rt.pgrad(getattr(m, attr)) for m in self.members]
        if any(p is None for p in ps):
            return None
        for m, p, q in zip(self.members, ps, ps[1:]):
            per = m.mod.conv.weight[0].numel() if attr == "pw" else 1
            if q != p + 4 * per * m.c:
                return None
        return ps[0]

    def bn_grads(self, rt):
        return self._adjacent(rt, "pg"), self._adjacent(rt, "pb")

    def bwd(self, rt):
        c = self.c
        dg, db = self.bn_grads(rt)
        if dg is not None and db is not None:
            app = self.bn_bwd(rt, dg, db)
        elif self.bn_eval and all(rt.pgrad(pi) is None for m in self.members for pi in (m.pg, m.pb)):
            app = self.bn_bwd(rt, None, None)
        else:
            tmp = rt.gbase + rt.plan.gscratch["sib"]
            app = self.bn_bwd(rt, tmp, tmp + 4 * c)
            for m, off in self.parts():
                for src, pi in ((tmp, m.pg), (tmp + 4 * c, m.pb)):
                    d = rt.pgrad(pi)
                    if d is not None:
                        L.call("yms_copy", d, src + 4 * off, 4 * m.c, rt.st)
        self.bwd_grads(rt, *self.bn_bwd_apply(rt, app))

    def wgrad(self, rt, dz, ld, off):
        dw = self._adjacent(rt, "pw")
        if dw is not None:
            self.launch_wgrad(rt, dz, ld, off, dw)
        else:
            for m, moff in self.parts():
                m.wgrad(rt, dz, ld, off + moff)

    def grad_params(self):
        # member-major within each kind: the flat arena then holds [dbeta_a | dbeta_b],
        # [dgamma_a | dgamma_b] and [dw_a | dw_b] contiguously (_adjacent)
        return [m.pb for m in self.members] + [m.pg for m in self.members] + [m.pw for m in self.members]


class BiasConvOp(ConvBase):
    """Plain nn.Conv2d with bias (the head's final 1x1 layers, yolov8_head.py:86-109)."""

    def __init__(self, b, conv, x, y):
        if conv.groups != 1 or conv.bias is None:
            raise RuntimeError("yms: biased ungrouped conv expected")
        k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        self.conv, self.x, self.y = conv, x, y
        self.shape = L.ConvShape(b.n, x.h, x.w, conv.in_channels, conv.out_channels, k, s, p, y.h, y.w, b.dt)
        self.sp = ctypes.pointer(self.shape)
        self.c = conv.out_channels
        self.npix = b.n * y.h * y.w
        self.pw = b.param(conv, "weight")
        self.pbias = b.param(conv, "bias")
        self.flops = 2 * self.npix * self.c * conv.in_channels * k * k

    def layout(self, plan, La, Le):
        self.layout_eval(plan, Le)
        if plan.training:
            self.layout_packs(plan, La)
            plan.need_scratch("bwd", 4 * 2 * self.c * L.lib().yms_bn_bwd_rows(self.npix, self.c))
            self.wg_ws = L.lib().yms_conv_wgrad_ws_bytes(self.sp)
            plan.need_scratch("wgrad", self.wg_ws)
            self.cnt = plan.counter()

    def eval_inputs(self):
        return [self.conv.weight]

    def conv_args(self, rt, grp=False):
        y = self.y
        return [(self, (rt.a(y), y.buf.ld, y.off, None, self.conv.bias.data_ptr(), L.ACT_NONE, None, None))]

    def fwd(self, rt):
        if rt.training:
            self.pack_unless_prepacked(rt)
        L.call_job("yms_conv_fwd", self.conv_job(rt, *self.conv_args(rt)[0][1]), rt.st)

    def dz(self, rt):
        y = self.y
        return rt.g(y), y.buf.ld, y.off

    def bias_job(self, rt, grp=False):
        """dbias = the column sums of the output gradient (grp: as BNConvBase's job records)."""
        gy, gy_ld, gy_off = self.dz(rt)
        return L.BnPassJob(npix=self.npix, c=self.c, gy=gy, gy_ld=gy_ld, gy_off=gy_off,
                           ws=rt.gbase + rt.plan.gscratch["bwd"] + (self.g_bwd if grp else 0),
                           counter=rt.cnt(self.cnt), dbias=rt.pgrad(self.pbias))

    def bwd(self, rt):
        if rt.pgrad(self.pbias) is not None:
            L.call_job("yms_bias_bwd", self.bias_job(rt), rt.st, rt.plan.dt)
        self.bwd_grads(rt, *self.dz(rt))

    def grad_params(self):
        return [self.pbias, self.pw]


class DWConvOp(ConvOp):
    """Depthwise Conv block (YOLO-MS IB_k mid conv, yolov8/model/yolo_ms.py): Conv2d(groups=C,
    bias=False, k x k, stride 1, pad k//2) -> BatchNorm2d -> SiLU, on the dwconv kernels.  BN
    forward/backward are the ConvOp path (inherited: only the conv launches and the layout differ);
    weights are read unpacked (fp32 [C][k][k])."""
    WGRAD = "yms_dwconv_wgrad"

    def __init__(self, b, mod, x, y, act):
        conv = mod.conv
        k = conv.kernel_size[0]
        c = conv.out_channels
        if not (conv.groups == c == conv.in_channels and conv.kernel_size[0] == conv.kernel_size[1]
                and k in (3, 5, 7, 9) and conv.stride == (1, 1) and conv.padding == (k // 2, k // 2)
                and conv.dilation == (1, 1)):
            raise RuntimeError("yms: grouped convolutions are supported as depthwise k x k (k = 3/5/7/9), "
                               "stride 1, pad k//2")
        self.init_block(b, mod, x, y, None, act)
        self.dshape = L.DwShape(b.n, x.h, x.w, c, k, b.dt)
        self.sp = ctypes.pointer(self.dshape)
        self.flops = 0         # not an MFMA contraction: excluded from the conv roofline
        self.dw_flops = 2 * self.npix * c * k * k
        self.bnred_for = self.bnred_by = self.bnred_key = self.bnred_wkey = None   # (ConvOp's fused-reduce links: unused)

    def layout(self, plan, La, Le):
        self.e_sc = Le.alloc(4 * self.c)
        self.e_sh = Le.alloc(4 * self.c)
        if plan.training:
            self.stats_rows = L.lib().yms_dwconv_stats_rows(self.sp)
            self.stats_ld = r8(self.c)
            # sized once here and passed as-is at backward time: the C side reads its tiling knobs
            # on every call, so a recomputed size could outgrow the region reserved here
            self.wg_ws = L.lib().yms_dwconv_wgrad_ws_bytes(self.sp)
            self.layout_bn(plan, La)

    def layout_packs(self, plan, La):
        pass

    def pack_specs(self):
        return ()

    def prepare_eval(self, rt):
        self.fold_bn(rt)

    def conv_fwd(self, rt, out, ld, off, sc, sh, act, res, stats):
        x = self.x
        L.call("yms_dwconv_fwd", self.sp, rt.a(x), x.buf.ld, x.off, self.conv.weight.data_ptr(), out, ld, off,
               sc, sh, act, stats, self.stats_ld if stats else 0, rt.st)

    def dgrad(self, rt, dz, ld, off):
        x = self.x
        L.call("yms_dwconv_dgrad", self.sp, dz, ld, off, self.conv.weight.data_ptr(), rt.g(x), x.buf.ld, x.off,
               self.acc_x, rt.st)


class AddOp(Op):
    """y = a + b (b None: y = a) over channel views: the MS-Block branch sums X_i + Y_{i-1} and
    the Y_1 = X_1 placement.  Backward routes dy into both addends (store or accumulate)."""

    def __init__(self, b, a, bb, y):
        self.a, self.b, self.y = a, bb, y
        self.npix = b.n * y.h * y.w
        self.c = y.c

    def fwd(self, rt):
        a, y = self.a, self.y
        L.call("yms_add_views", rt.plan.dt, self.npix, self.c, rt.a(a), a.buf.ld, a.off, *_opt(rt.a, self.b),
               rt.a(y), y.buf.ld, y.off, 0, rt.st)

    def plan_grads(self, T):
        T.read(self.y)
        self.acc = [T.write(v) if (v is not None and v.buf.needs_grad) else None for v in (self.a, self.b)]

    def bwd(self, rt):
        y = self.y
        if all(v is not None and acc is not None for v, acc in zip((self.a, self.b), self.acc)):
            a, b = self.a, self.b
            L.call("yms_add_grad2", rt.plan.dt, self.npix, self.c, rt.g(y), y.buf.ld, y.off, rt.g(a), a.buf.ld,
                   a.off, self.acc[0], rt.g(b), b.buf.ld, b.off, self.acc[1], rt.st)
            return
        for v, acc in zip((self.a, self.b), self.acc):
            if v is None or acc is None:
                continue
            L.call("yms_add_views", rt.plan.dt, self.npix, self.c, rt.g(y), y.buf.ld, y.off, None, 0, 0, rt.g(v),
                   v.buf.ld, v.off, acc, rt.st)


class UpsampleOp(Op):
    """nearest x2, components.py:153-160."""

    def __init__(self, b, x, y):
        self.x, self.y, self.n = x, y, b.n

    def fwd(self, rt):
        x, y = self.x, self.y
        L.call("yms_upsample2x_fwd", rt.plan.dt, self.n, x.h, x.w, x.c, rt.a(x), x.buf.ld, x.off,
               rt.a(y), y.buf.ld, y.off, rt.st)

    def plan_grads(self, T):
        T.read(self.y)
        self.acc_x = T.write(self.x) if self.x.buf.needs_grad else 0

    def bwd(self, rt):
        x, y = self.x, self.y
        if not x.buf.needs_grad:
            return
        L.call("yms_upsample2x_bwd", rt.plan.dt, self.n, x.h, x.w, x.c, rt.g(y), y.buf.ld, y.off,
               rt.g(x), x.buf.ld, x.off, self.acc_x, rt.st)


class SppfPoolOp(Op):
    """The three chained MaxPool2d(5,1,2) of SPPF (components.py:136-146) over a 4-slot buffer."""

    def __init__(self, b, v4, c):
        self.v, self.c, self.n = v4, c, b.n

    def layout(self, plan, La, Le):
        if plan.training:
            plan.need_scratch("sppf", L.lib().yms_sppf_ws_bytes(self.n, self.v.h, self.v.w, self.c))

    def fwd(self, rt):
        v = self.v
        L.call("yms_sppf_pool_fwd", rt.plan.dt, self.n, v.h, v.w, self.c, rt.a(v), v.buf.ld, v.off, rt.st)

    def plan_grads(self, T):
        T.read(self.v)        # slot grads come from conv2's dgrad; the pool chain accumulates in place

    def bwd(self, rt):
        v = self.v
        L.call("yms_sppf_pool_bwd", rt.plan.dt, self.n, v.h, v.w, self.c, rt.a(v), v.buf.ld, v.off,
               rt.g(v), v.buf.ld, v.off, rt.gbase + rt.plan.gscratch["sppf"], rt.st)


def _op_views(op):
    """Every View an op holds, a SiblingConvOp's members' included."""
    for k, v in vars(op).items():
        for u in (v if isinstance(v, (list, tuple)) else (v,)):
            if isinstance(u, View):
                yield u
            elif k == "members":
                yield from _op_views(u)


def _in_views(op):
    """The Views an op reads: all it holds but its output (SppfPoolOp.v is both)."""
    for k, v in vars(op).items():
        if k not in ("y", "members"):
            for u in (v if isinstance(v, (list, tuple)) else (v,)):
                if isinstance(u, View):
                    yield u


def _array(jobs):
    return (type(jobs[0]) * len(jobs))(*jobs)


class HeadGroup:
    """Independent chains of conv ops -- the detection head's three levels (Builder.independent_chains)
    -- run stage by stage: stage d holds, from every chain, the ops d steps behind their chain's input,
    and each pass of a stage over its members is ONE grouped call (yms_*_group), in which every
    member is decomposed exactly as by its solo call, so results are bit-identical to running the ops
    one after the other.  Forward: the convs, then the BN finalizes, then the affine passes.  Backward:
    the bias / BN reduce, finalize and apply passes, the input gradients, then each member's weight
    gradient on the side stream, in the members' backward order, after the launch that wrote its dz.
    The members' slices of the shared "stats", "bwd" and "coef" scratch are disjoint (layout).
    The plan keeps the member ops in plan.ops; plan.sched runs the group in their place."""

    KINDS = None    # the op types a group can run (set below the class)

    def __init__(self, chains):
        self.ops = [op for ch in chains for op in ch]
        self.bwd_ops = tuple(reversed(self.ops))
        depth = {}
        for ch in chains:
            for i, op in enumerate(ch):
                depth[id(op)] = 1 + max((depth[id(q)] for q in ch[:i] if _overlap(q.y, op.x)), default=-1)
        self.stages = [[op for op in self.ops if depth[id(op)] == d] for d in range(1 + max(depth.values()))]

    @classmethod
    def build(cls, chains):
        """-> a HeadGroup, or None (every op then runs on its own, as without grouping) unless the
        chains have the same sequence of op kinds, every op is a plain conv kind without a fused
        neighbour (stem, producer's BN reduce, weight gradient first), ops of different chains touch
        no common memory and no two outputs of one stage overlap."""
        if len(chains) < 2 or len({tuple(type(op) for op in ch) for ch in chains}) != 1:
            return None
        for ch in chains:
            for op in ch:
                if type(op) not in cls.KINDS or op.stem_input is not None or op.tail_wgrad_first:
                    return None
                if getattr(op, "bnred_for", None) is not None or getattr(op, "bnred_by", None) is not None:
                    return None
        views = [[v for op in ch for v in _op_views(op)] for ch in chains]
        for i, va in enumerate(views):
            for vb in views[i + 1:]:
                if any(_overlap(a, b) for a in va for b in vb):
                    return None
        g = cls(chains)
        for st in g.stages:
            if any(_overlap(a.y, b.y) for i, a in enumerate(st) for b in st[i + 1:]):
                return None
        return g

    def layout(self, plan):
        """Training: per stage, the members' slices of the shared scratch regions, which are sized by
        the largest stage's sum."""
        if not plan.training:
            return
        for st in self.stages:
            stats = bwd = coef = 0
            for op in st:
                if isinstance(op, BiasConvOp):
                    op.g_bwd = bwd
                    bwd += _al(4 * 2 * op.c * L.lib().yms_bn_bwd_rows(op.npix, op.c))
                    continue
                for m, _ in op.parts():
                    m.g_stats = stats
                    if not op.bn_eval:           # (running statistics: no table)
                        stats += _al(4 * m.stats_rows * (2 * m.stats_ld + 1))
                op.g_bwd, op.g_coef = bwd, coef
                bwd += _al(4 * 2 * op.c * op.bwd_rows)
                coef += _al(8 * op.c)
            plan.need_scratch("stats", stats)
            plan.need_scratch("bwd", bwd)
            plan.need_scratch("coef", coef)

    # ---- forward -------------------------------------------------------------------------
    def fwd(self, rt):
        if rt.training and not rt.prepacked:
            for op in self.ops:
                op.fwd(rt)
            return
        for st in self.stages:
            self.fwd_stage(rt, st)

    def fwd_stage(self, rt, st):
        convs = [m.conv_job(rt, *args) for op in st for m, args in op.conv_args(rt, True)]
        L.call("yms_conv_fwd_group", len(convs), _array(convs), rt.st)
        bn = [op for op in st if rt.training and isinstance(op, BNConvBase) and not op.infer]
        fins = [j for op in bn for j in op.finalize_jobs(rt, True)]
        if fins:
            L.call("yms_bn_finalize_group", len(fins), _array(fins), rt.st)
        if bn:
            L.call("yms_affine_act_group", rt.plan.dt, len(bn), _array([op.affine_job(rt) for op in bn]), rt.st)

    # ---- backward ------------------------------------------------------------------------
    def bwd_grouped(self, rt):
        """The grouped backward serves the case every training step meets: all the members' parameters
        take a gradient and each sibling pair's gradients are adjacent in the flat arena.  Otherwise
        (a frozen member), and with Options.head_group < 2, the members run their own backward."""
        if rt.plan.opts.head_group < 2 or not all(op.runs_bwd for op in self.ops):
            return False
        for op in self.ops:
            if any(rt.pgrad(pi) is None for pi in op.grad_params()):
                return False
            if isinstance(op, SiblingConvOp) and any(op._adjacent(rt, a) is None for a in ("pg", "pb", "pw")):
                return False
        return True

    def bwd(self, rt):
        if not self.bwd_grouped(rt):
            for op in self.bwd_ops:
                if op.runs_bwd:
                    op.bwd(rt)
            return
        for st in reversed(self.stages):
            self.bwd_stage(rt, st[::-1])

    def bwd_stage(self, rt, ops):
        dt = rt.plan.dt
        bias = [op.bias_job(rt, True) for op in ops if isinstance(op, BiasConvOp)]
        if bias:
            L.call("yms_bias_bwd_group", dt, len(bias), _array(bias), rt.st)
        bn = [op.bwd_jobs(rt, *op.bn_grads(rt), True) for op in ops if isinstance(op, BNConvBase)]
        if bn:
            red, fin, app = zip(*bn)
            L.call("yms_bn_act_bwd_reduce_group", dt, len(red), _array(red), rt.st)
            L.call("yms_bn_act_bwd_finalize_group", len(fin), _array(fin), rt.st)
            L.call("yms_bn_act_bwd_apply_group", dt, len(app), _array(app), rt.st)
        dgs = [op.dgrad_job(rt, *op.dz(rt)) for op in ops if op.x.buf.needs_grad]
        if dgs:
            L.call("yms_conv_dgrad_group", len(dgs), _array(dgs), rt.st)
        for op in ops:
            op.wgrad(rt, *op.dz(rt))


HeadGroup.KINDS = (ConvOp, SiblingConvOp, BiasConvOp)


class Builder:
    """Collects buffers, ops and parameter references while modules ``emit``."""

    def __init__(self, n, dt, training, opts=None):
        self.n, self.dt, self.training = n, dt, training
        self.opts = opts if opts is not None else read_options()
        self.es = 4 if dt == L.F32 else 2
        self.bufs = []
        self.ops = []
        self.param_refs = []      # (module, attr)
        self.chain_sets = []      # independent_chains: [(first op index, end), ...] per set
        self._pidx = {}

    def new(self, h, w, c, name="act", ld=None):
        b = Buf(len(self.bufs), self.n, h, w, ld if ld is not None else r8(c), name, zero=(c % 8 != 0))
        self.bufs.append(b)
        return View(b, 0, c)

    def param(self, mod, attr):
        key = (id(mod), attr)
        if key not in self._pidx:
            self._pidx[key] = len(self.param_refs)
            self.param_refs.append((mod, attr))
        return self._pidx[key]

    # --- emitters used by the yolov8 modules -------------------------------------------
    def conv(self, mod, x, out=None, res=None, act=None):
        conv = mod.conv
        k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        ho, wo = (x.h + 2 * p - k) // s + 1, (x.w + 2 * p - k) // s + 1
        if out is None:
            out = self.new(ho, wo, conv.out_channels)
        assert out.c == conv.out_channels and out.h == ho and out.w == wo, "yms: output view mismatch"
        if act is None:
            act = L.ACT_SILU if isinstance(mod.activation, torch.nn.SiLU) else L.ACT_NONE
        if conv.groups != 1:
            if res is not None:
                raise RuntimeError("yms: residual epilogue is not supported on depthwise convolutions")
            self.ops.append(DWConvOp(self, mod, x, out, act))
        else:
            self.ops.append(ConvOp(self, mod, x, out, res, act))
        return out

    def sibling_convs(self, mods, x):
        """Two Conv blocks reading the same input x -> their output views, the channel slots of one
        buffer (SiblingConvOp), or two separate ConvOps when they cannot share one (different
        geometry or activation, a first member whose width is not a multiple of 8, BatchNorm modules
        in different modes -- one in eval mode inside a training plan, the other not: the fused BN
        passes take one kind of statistics -- or YMS_HEAD_FUSE=0)."""
        ks = {(m.conv.kernel_size, m.conv.stride, m.conv.padding, m.conv.groups, m.conv.dilation,
               isinstance(m.activation, torch.nn.SiLU)) for m in mods}
        fuse = (len(mods) == 2 and len(ks) == 1 and mods[0].conv.groups == 1 and mods[0].conv.out_channels % 8 == 0
                and self.opts.head_fuse and (not self.training or len({m.bn.training for m in mods}) == 1))
        if not fuse:
            return [m.emit(self, x) for m in mods]
        conv = mods[0].conv
        k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        ho, wo = (x.h + 2 * p - k) // s + 1, (x.w + 2 * p - k) // s + 1
        y = self.new(ho, wo, sum(m.conv.out_channels for m in mods))
        act = L.ACT_SILU if isinstance(mods[0].activation, torch.nn.SiLU) else L.ACT_NONE
        op = SiblingConvOp(self, mods, x, y, act)
        self.ops.append(op)
        return [m.y for m in op.members]

    def independent_chains(self, ranges):
        """The ops emitted in each (first, end) index range of self.ops form a chain that shares no
        memory with the other ranges' (the head's levels): the plan may run them side by side, stage
        by stage (HeadGroup)."""
        self.chain_sets.append([tuple(r) for r in ranges])

    def add(self, a, b, out=None):
        """y = a + b (b may be None: a placement copy) -> view."""
        if b is not None and (a.h, a.w, a.c) != (b.h, b.w, b.c):
            raise RuntimeError("yms: add of mismatched views")
        if out is None:
            out = self.new(a.h, a.w, a.c)
        self.ops.append(AddOp(self, a, b, out))
        return out

    def conv2d_bias(self, conv, x, out=None):
        k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        ho, wo = (x.h + 2 * p - k) // s + 1, (x.w + 2 * p - k) // s + 1
        if out is None:
            out = self.new(ho, wo, conv.out_channels)
        self.ops.append(BiasConvOp(self, conv, x, out))
        return out

    def upsample(self, x, out=None):
        if out is None:
            out = self.new(2 * x.h, 2 * x.w, x.c)
        self.ops.append(UpsampleOp(self, x, out))
        return out

    def sppf_pool(self, v4, c):
        self.ops.append(SppfPoolOp(self, v4, c))


class Plan:
    def __init__(self, b: Builder, inputs, outputs, kind):
        self.n, self.dt, self.training, self.es = b.n, b.dt, b.training, b.es
        self.bufs, self.ops, self.param_refs = b.bufs, b.ops, b.param_refs
        self.inputs, self.outputs, self.kind = inputs, outputs, kind
        self.opts = b.opts
        self.scratch_req = {}
        self.n_counters = 0
        # per-plan caches of the runner
        self._pack_tables = {}      # parameter set -> the batched pack's device job table (pack_table)
        self._pg_layouts = {}       # requires_grad pattern -> flat parameter-gradient arena layout
        self._infer_arenas = {}     # (stream, host thread) -> a decode plan's internal arena
        self._nbt = None            # the BatchNorm num_batches_tracked tensors a training step bumps
        self._fold_tables = {}      # parameter set -> the eval-mode BN folds' device job table (fold_table)
        self._fold_bns = self._fold_now = None
        self.root = getattr(b, "root", None)    # the module the plan was built from (names in messages)
        self.stem_inputs = self._find_stems()
        self._find_backward()
        if self.training and self.opts.wgrad_tail_first:
            stem_out = {op.y.buf.idx for op in self.stem_inputs.values()}
            for op in self.ops:
                if type(op) is ConvOp and op.x.buf.idx in stem_out:
                    op.tail_wgrad_first = True
        self._find_bnred()
        self.groups = self._find_groups(b.chain_sets)
        # the backward walk: the steps that have anything to run, in reverse
        self.bwd_sched = [s for s in reversed(self.sched) if any(op.runs_bwd for op in getattr(s, "ops", (s,)))]
        La, Le = Layout(), Layout()
        # an input the stem conv reads as NCHW fp32 has no NHWC buffer: no arena bytes, and no
        # per-step zeroing of its padding channels (3 -> 8: 419 MB, 51 us per configs[2] step)
        stem_bufs = {self.inputs[i].buf.idx for i in self.stem_inputs}
        for buf in self.bufs:
            if buf.idx in stem_bufs:
                buf.off, buf.zero = 0, False
                continue
            buf.off = La.alloc(buf.npix * buf.ld * self.es)
        self.act_bytes = La.size
        for op in self.ops:
            op.layout(self, La, Le)
        for g in self.groups:
            g.layout(self)
        self.scratch = {}
        if self.training:
            self.scratch["stats"] = La.alloc(self.scratch_req.get("stats", 0))
        self.arena_bytes = La.size
        # grad arena: activation grads share the activation layout, then backward scratch
        Lg = Layout()
        Lg.size = self.act_bytes
        self.gscratch = {k: Lg.alloc(self.scratch_req.get(k, 0)) for k in ("bwd", "coef", "wgrad", "sppf", "stemwg", "sib")}
        for k in sorted(k for k in self.scratch_req if k.startswith("bnr")):
            self.gscratch[k] = Lg.alloc(self.scratch_req[k])
        if "zcoef" in self.scratch_req:
            self.gscratch["zcoef"] = Lg.alloc(self.scratch_req["zcoef"])
        self.gscratch["cnt"] = Lg.alloc(16 * max(self.n_counters, 1))
        self.garena_bytes = Lg.size
        self.eval_bytes = Le.size
        self.zero_ranges = [(bf.off, bf.npix * bf.ld * self.es) for bf in self.bufs if bf.zero]
        if self.training:
            for op in self.ops:
                self.zero_ranges.extend(op.z_padding(self.es))
            T = GradTracker()
            self.seed_acc = [T.write(v) for v in self.outputs]
            T.writes = set()
            for op in reversed(self.ops):
                # only the ops that run write or read a gradient: a skipped producer never reads its slot of
                # a buffer whose other slots' consumers wrote the whole of it (the neck's concat buffers)
                if op.runs_bwd:
                    op.plan_grads(T)
                y = getattr(op, "y", None)
                if isinstance(y, View) and not any(y is o for o in self.outputs):
                    _check_not_in_place(op, y)
                    T.release(y)
            # output buffers whose gradient no op writes (only reads): the incoming gradient tensor
            # can serve as that buffer's gradient in place (runner._seed_grad), no copy
            self.grad_read_only = {v.buf.idx for v in self.outputs if v.buf.idx not in T.writes}
            self.gzero_ranges = [(bf.off, bf.npix * bf.ld * self.es) for bf in self.bufs if bf.idx in T.zero]
            self.gzero_ranges.append((self.gscratch["cnt"], 16 * max(self.n_counters, 1)))
            if "zcoef" in self.gscratch:
                self.gzero_ranges.append((self.gscratch["zcoef"], self.scratch_req["zcoef"]))
        self.flops = sum(op.flops for op in self.ops)
        # parameter-gradient arena in backward-completion order (reverse op order)
        order = []
        seen = set()
        for op in reversed(self.ops):
            for pi in op.grad_params():
                if pi not in seen:
                    seen.add(pi)
                    order.append(pi)
        self.pgrad_order = order
        self._eval_sig = None
        self._eval_arena = None

    def _find_stems(self):
        """Inputs whose only reader is a stem-shaped Conv (3x3 stride 2 over <= 3 channels, no
        residual, 16-bit compute, input without gradient): that conv reads the NCHW fp32 input
        itself (yms_conv_stem_fwd, and yms_conv_stem_wgrad with the BN backward apply fused in),
        so the NHWC input pack goes.  YMS_STEM=0 keeps the generic pack + implicit-GEMM path."""
        out = {}
        if self.dt == L.F32 or not self.opts.stem:
            return out
        for i, v in enumerate(self.inputs):
            readers = [op for op in self.ops
                       if any(isinstance(a, View) and a.buf is v.buf for a in vars(op).values())]
            if len(readers) != 1 or type(readers[0]) is not ConvOp:
                continue
            op = readers[0]
            if (op.x.buf is v.buf and op.x.off == 0 and op.x.c == v.c and op.res is None and v.buf.ld == r8(v.c)
                    and not v.buf.needs_grad
                    and L.lib().yms_conv_stem_supported(op.sp)):
                op.stem_input = i
                out[i] = op
        return out

    def _name(self, mod):
        names = [n for n, m in self.root.named_modules() if m is mod] if self.root is not None else []
        return names[0] if names else type(mod).__name__

    def _find_backward(self):
        """Which ops run a backward, which buffers need a gradient, which BN layers use running statistics.
        Static per plan: runner.get_plan keys the cache by the parameters' requires_grad pattern and the
        BatchNorm modules' train / eval pattern.

        An op runs its backward iff a parameter of its own requires a gradient or one of its inputs needs
        one; a buffer needs a gradient iff the producer of any of its slots runs its backward, or it is a
        plan input that requires one (set by get_plan).  An op that does not run launches nothing in the
        backward; one that runs with an input that needs no gradient skips its input gradient
        (x.buf.needs_grad, as the plan inputs always did).  YMS_BWD_SKIP=0: everything runs.

        A BatchNorm module in eval mode inside a training plan normalises with its running statistics
        and leaves them alone (bn_eval); where nothing downstream of it needs a backward either, the op
        takes the inference route (infer: the conv's epilogue writes y, no z)."""
        for op in self.ops:
            op.runs_bwd, op.bn_eval, op.infer = True, False, False
        if not self.training:
            return
        req = [getattr(m, a).requires_grad for m, a in self.param_refs]
        skip = self.opts.bwd_skip
        if skip:
            ins = {v.buf.idx for v in self.inputs}
            for bf in self.bufs:
                if bf.idx not in ins:
                    bf.needs_grad = False
        for op in self.ops:
            if skip:
                op.runs_bwd = (any(req[pi] for pi in op.grad_params())
                               or any(v.buf.needs_grad for v in _in_views(op)))
                if op.runs_bwd and isinstance(getattr(op, "y", None), View):
                    op.y.buf.needs_grad = True
            ev = [not m.bn.training for m in op.bn_modules()]
            if any(ev) and not all(ev):
                raise RuntimeError("yms: " + " and ".join(self._name(m) for m in op.bn_modules()) + " run as one fused "
                                   "pass over both outputs, so their BatchNorm modules must be in the same mode "
                                   "(both train or both eval), or set YMS_HEAD_FUSE=0")
            op.bn_eval = any(ev)
            for m in op.bn_modules() if op.bn_eval else ():
                if m.bn.running_mean is None or m.bn.running_var is None:
                    raise RuntimeError(f"yms: {self._name(m)}.bn is in eval mode without running statistics "
                                       "(track_running_stats=False): torch would normalise with batch statistics "
                                       "there, which the running-statistics routes do not do")
            op.infer = op.bn_eval and skip and not op.runs_bwd
            for m in getattr(op, "members", ()):
                m.runs_bwd, m.bn_eval, m.infer = op.runs_bwd, op.bn_eval, op.infer

    def _find_bnred(self):
        """Training, 16-bit: a Conv whose input gradient runs on the direct 3x3 kernel
        (yms_conv_dgrad_bnred_rows > 0) and whose input view is exactly the output of an earlier
        Conv op P, with no op in between touching that view (so this dgrad is the LAST writer of
        P's output gradient, backward order), computes P's BN + act backward reduce in its epilogue
        (yms_conv_dgrad_bnred): P's separate reduce pass (z and gy read once more) goes, and P's
        finalize reads the partial rows from a grad-scratch region of their own.  YMS_BNRED=0 keeps
        the separate reduce (A/B)."""
        if not self.training or self.dt == L.F32 or not self.opts.bnred:
            return

        def views(op):
            for v in vars(op).values():
                for u in (v if isinstance(v, (list, tuple)) else (v,)):
                    if isinstance(u, View):
                        yield u

        n = 0
        for i, c in enumerate(self.ops):
            if type(c) is not ConvOp or c.stem_input is not None or not c.x.buf.needs_grad or not c.runs_bwd:
                continue
            rows = L.lib().yms_conv_dgrad_bnred_rows(c.sp)
            if rows <= 0:
                continue
            x = c.x
            j = next((j for j in range(i - 1, -1, -1)
                      if isinstance(getattr(self.ops[j], "y", None), View) and _overlap(self.ops[j].y, x)), None)
            if j is None:
                continue
            q = self.ops[j]
            if (type(q) is not ConvOp or q.y.off != x.off or q.y.c != x.c or q.c != x.c or q.bnred_by is not None
                    or q.act not in (L.ACT_NONE, L.ACT_SILU) or not q.runs_bwd or q.bn_eval):
                continue
            if any(_overlap(v, x) for op in self.ops[j + 1:i] for v in views(op)):
                continue
            if any(_overlap(v, x) for k, v in vars(c).items() if isinstance(v, View) and k != "x"):
                continue
            key = f"bnr{n}"
            n += 1
            # a conv can be both: the consumer of one pair (wkey) and the producer of the next (key)
            c.bnred_for, c.bnred_wkey = q, key
            q.bnred_by, q.bnred_key, q.bnred_rows = c, key, rows
            self.need_scratch(key, 4 * rows * 2 * r8(x.c))

    def _find_groups(self, chain_sets):
        """The HeadGroups of the builder's chain sets (Options.head_group; a set whose ranges are not
        one contiguous run of ops, or that HeadGroup.build declines, stays ungrouped), and self.sched:
        what the runner walks -- the ops, with each group in the place of its members."""
        groups = []
        if self.opts.head_group:
            for ranges in chain_sets:
                if any(a >= b for a, b in ranges) or any(r[1] != q[0] for r, q in zip(ranges, ranges[1:])):
                    continue
                g = HeadGroup.build([self.ops[a:b] for a, b in ranges])
                if g is not None:
                    groups.append(g)
        first = {id(g.ops[0]): g for g in groups}
        member = {id(op) for g in groups for op in g.ops}
        self.sched = [first.get(id(op), op) for op in self.ops if id(op) in first or id(op) not in member]
        return groups

    def counter(self):
        """Reserve one 16-B arrival counter in the grad scratch (-> its index)."""
        self.n_counters += 1
        return self.n_counters - 1

    def need_scratch(self, key, nbytes):
        self.scratch_req[key] = max(self.scratch_req.get(key, 0), int(nbytes))

    def params(self):
        return [getattr(m, a) for (m, a) in self.param_refs]

    # ------------------------------------------------------------------------------------
    def ensure_eval_cache(self, device, stream):
        """(Re)pack weights and fold BN when any parameter / buffer changed."""
        sig = tuple((t.data_ptr(), t._version) for op in self.ops for t in op.eval_inputs())
        if self._eval_arena is None or self._eval_arena.device != device:
            self._eval_arena = torch.empty(max(self.eval_bytes, 1), dtype=torch.uint8, device=device)
            self._eval_sig = None
        if sig != self._eval_sig:
            rt = Rt(self, None, stream, False)
            rt.eval_base = self._eval_arena.data_ptr()
            for op in self.ops:
                op.prepare_eval(rt)
            self._eval_sig = sig
        return self._eval_arena.data_ptr()

    def pack_table(self):
        """The batched pack's device job table (built and uploaded on the CURRENT stream on a
        cache miss: call it before handing prepack to another stream)."""
        specs = [sp for op in self.ops for sp in op.pack_specs()]
        key = tuple((sp[1], sp[2], sp[4] if len(sp) > 4 else None) for sp in specs)
        cache = self._pack_tables
        ent = cache.get(key)
        if ent is None:
            jobs, singles = [], []
            for spec in specs:
                sp, w, dst, fd = spec[:4]
                j = L.PackJob()
                st = L.lib().yms_pack_job_init(sp, w, dst, fd, ctypes.byref(j))
                if len(spec) > 4:                 # two sources (SiblingConvOp): batched only
                    if st != 0:
                        raise RuntimeError("yms: a two-source weight pack must be batchable")
                    j.w2, j.split = spec[4]
                if st == 0:
                    jobs.append(j)
                else:
                    singles.append((sp, w, dst, fd))
            arr = (L.PackJob * max(len(jobs), 1))(*jobs)
            host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
            table = host.to(torch.device("cuda", torch.cuda.current_device()))
            if len(cache) >= 4:
                cache.clear()
            ent = cache[key] = (table, len(jobs), singles)
        self._fold_now = self.fold_table()      # (uploaded on the current stream too; prepack uses this one)
        return ent

    def fold_table(self):
        """(device table, jobs, widest c) of the eval-mode BN layers' folds, cached like pack_table (the
        table holds parameter addresses and arena offsets); None without such layers."""
        if self._fold_bns is None:      # once per plan: the layers (a stem folds itself, BNConvBase.fold_own)
            ops = [op for op in self.ops if op.bn_eval and op.stem_input is None]
            self._fold_ops, self._fold_bns = ops, [m.mod.bn for op in ops for m, _ in op.parts()]
        if not self._fold_bns:
            return None
        key = tuple([t.data_ptr() for bn in self._fold_bns for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)])
        ent = self._fold_tables.get(key)
        if ent is None:
            jobs = [j for op in self._fold_ops for j in op.fold_jobs()]
            host = torch.frombuffer(bytearray(bytes(_array(jobs))), dtype=torch.uint8)
            table = host.to(torch.device("cuda", torch.cuda.current_device()))
            if len(self._fold_tables) >= 4:
                self._fold_tables.clear()
            ent = self._fold_tables[key] = (table, len(jobs), max(j.c for j in jobs))
        return ent

    def prepack(self, rt, ent=None):
        """Training: issue every conv weight pack of the step on rt.st -- one batched launch for
        the plain packs (device job table of arena OFFSETS, cached per parameter set, so it is
        valid for any arena and is built before any graph capture) plus the stride-2 dgrad
        parity packs individually."""
        table, nj, singles = ent if ent is not None else self.pack_table()
        L.call("yms_conv_pack_weights_batched", nj, table.data_ptr(), rt.base, rt.st)
        for sp, w, dst, fd in singles:
            L.call("yms_conv_pack_weight", sp, w, rt.base + dst, fd, rt.st)
        fold = self._fold_now           # (pack_table's, of this step)
        if fold is not None:
            L.call("yms_bn_fold_mi_batched", fold[1], fold[0].data_ptr(), fold[2], rt.base, rt.st)
        rt.prepacked = True

    def new_arena(self, device, stream):
        arena = torch.empty(max(self.arena_bytes, 1), dtype=torch.uint8, device=device)
        base = arena.data_ptr()
        for off, nb in self.zero_ranges:
            L.call("yms_zero", base + off, nb, stream)
        return arena

    def act_tensor(self, arena, view, dtype):
        """torch view (NCHW-shaped, channels-last strided) of an activation buffer slice."""
        b = view.buf
        nb = b.npix * b.ld * self.es
        t = arena[b.off:b.off + nb].view(dtype).view(b.n, b.h, b.w, b.ld)
        return t[..., view.off:view.off + view.c].permute(0, 3, 1, 2)
