"""Test infra (no GPU): trace a plan's calls on meta tensors and turn each into the memory it reads and writes.

trace_fwd / trace_bwd run op.fwd(rt) over plan.sched / step.bwd(rt) over reversed(plan.sched) with
yms._lib.call recording every call (entry point, arguments by name, stream; a grouped call as its member
jobs), on an Rt with fake base addresses and fake stream / event objects.  The ACCESS table turns every
call into the byte ranges it reads and writes -- written from the contracts of include/yms.h, not from
the plan code.  An entry point the table does not know fails the trace: a new pass has to be classified.
A view's range knows its channel slice, so two slots of one buffer (same address, same channel stride)
do not overlap.

Two audits use it: tests/test_stream_hazards_cpu.py (no main-stream pass disturbs a side-stream weight
gradient) and tests/test_plan_init_cpu.py (uninitialised below: every 16-byte channel group a call reads
was written before, by a call or by a zero range)."""
import ctypes

import torch

from yms import _lib as L
from yms import runner
from yms.plan import Rt

BASE, GBASE, PBASE, EBASE, XBASE = 1 << 40, 1 << 41, 1 << 43, 1 << 44, 1 << 45
MAIN, SIDE = 0x1000, 0x2000


# ---- tracing ---------------------------------------------------------------------------------------
# The arguments before the stream, by name (include/yms.h; the per-pixel passes under the field names
# of yms_bn_pass_job, which their grouped forms carry: out = dz, res = gres of yms_bn_act_bwd_apply,
# out = y of yms_affine_act).
SIG = {k: v.split() for k, v in {
    # the backward
    "yms_conv_dgrad": "shape dz dz_ld dz_off wpacked_t dx dx_ld dx_off accumulate",
    "yms_conv_dgrad_bnred": "shape dz dz_ld dz_off wpacked_t dx dx_ld dx_off accumulate z z_ld z_off scale shift "
                            "mean_invstd act ws",
    "yms_conv_wgrad": "shape x x_ld x_off dz dz_ld dz_off ws ws_bytes dw accumulate",
    "yms_conv_stem_wgrad": "shape x gy gy_ld gy_off z z_ld z_off scale shift mean_invstd coef act ws ws_bytes dw "
                           "accumulate",
    "yms_dwconv_dgrad": "shape dz dz_ld dz_off w dx dx_ld dx_off accumulate",
    "yms_dwconv_wgrad": "shape x x_ld x_off dz dz_ld dz_off ws ws_bytes dw accumulate",
    "yms_bn_act_bwd_reduce": "dtype npix c z z_ld z_off gy gy_ld gy_off scale shift mean_invstd act ws",
    "yms_bn_act_bwd_finalize": "c ws rows count dgamma dbeta coef",
    "yms_bn_act_bwd_apply": "dtype npix c z z_ld z_off gy gy_ld gy_off scale shift mean_invstd coef act "
                            "out out_ld out_off res res_ld res_off res_acc",
    "yms_bias_bwd": "dtype npix c gy gy_ld gy_off ws counter dbias",
    "yms_copy": "dst src bytes",
    "yms_add_views": "dtype npix c a a_ld a_off b b_ld b_off y y_ld y_off accumulate",
    "yms_add_grad2": "dtype npix c g g_ld g_off ga ga_ld ga_off acc1 gb gb_ld gb_off acc2",
    "yms_upsample2x_bwd": "dtype n h w c gy gy_ld gy_off gx gx_ld gx_off accumulate",
    "yms_sppf_pool_bwd": "dtype n h w c buf ld off gbuf gld goff ws",
    # the forward
    "yms_conv_fwd": "shape x x_ld x_off wpacked y y_ld y_off scale shift act res res_ld res_off stats",
    "yms_conv_stem_fwd": "shape x w y y_ld y_off scale shift act stats stats_ld",
    "yms_dwconv_fwd": "shape x x_ld x_off w y y_ld y_off scale shift act stats stats_ld",
    "yms_bn_finalize": "c stats rows stats_ld count gamma beta rmean rvar momentum eps mean_invstd scale shift",
    "yms_bn_finalize_ld": "c stats rows stats_ld count gamma beta rmean rvar momentum eps mean_invstd mi_ld scale shift",
    "yms_affine_act": "dtype npix c z z_ld z_off scale shift act res res_ld res_off out out_ld out_off",
    "yms_sppf_pool_fwd": "dtype n h w c buf ld off",
    "yms_upsample2x_fwd": "dtype n h w c x x_ld x_off y y_ld y_off",
    "yms_pack_input": "dtype n c h w x y ld",
    "yms_nchw_to_nhwc": "dtype_nchw dtype n h w c x y ld off accumulate",
    "yms_conv_pack_weights_batched": "njobs jobs dst_base",
    "yms_conv_pack_weight": "shape w packed for_dgrad",
}.items()}
# grouped entry point -> its members' solo one; (dtype,) njobs, jobs, stream
GROUPS = {"yms_conv_dgrad_group": "yms_conv_dgrad", "yms_bn_act_bwd_reduce_group": "yms_bn_act_bwd_reduce",
          "yms_bn_act_bwd_finalize_group": "yms_bn_act_bwd_finalize", "yms_bn_act_bwd_apply_group": "yms_bn_act_bwd_apply",
          "yms_bias_bwd_group": "yms_bias_bwd", "yms_conv_fwd_group": "yms_conv_fwd",
          "yms_bn_finalize_group": "yms_bn_finalize_ld", "yms_affine_act_group": "yms_affine_act"}


class Call:
    def __init__(self, pos, name, stream, a):
        self.pos, self.name, self.stream, self.a = pos, name, stream, a

    def __repr__(self):
        return f"#{self.pos} {self.name} on {'side' if self.stream == SIDE else 'main'}"


def _plain(v):
    if hasattr(v, "contents"):
        return v.contents
    return getattr(v, "value", v)


class _Stream:
    def __init__(self, ptr, log):
        self.cuda_stream, self.log = ptr, log

    def wait_event(self, ev):
        # wst(): the side stream waits for everything the main stream holds so far -- the event was
        # recorded on the main stream with no call in between
        assert self.cuda_stream == SIDE and ev.on is not None and ev.on.cuda_stream == MAIN
        assert ev.at == len(self.log), "the side stream waits on a stale record of the main stream"

    def wait_stream(self, other):
        raise AssertionError("no op's backward joins the streams: only _PlanFn.backward does, at its end")


class _Event:
    def __init__(self, log):
        self.log, self.on, self.at = log, None, None

    def record(self, stream):
        self.on, self.at = stream, len(self.log)


def recorder(log):
    """-> the stand-in of yms._lib.call that appends a Call per (member of a) call to log."""
    def rec(name, *args):
        *args, stream = args
        solo = GROUPS.get(name)
        if solo is not None:
            names = [f for f in SIG[solo] if f != "dtype"]
            dt = {"dtype": args[0]} if "dtype" in SIG[solo] else {}
            assert len(args) == 2 + len(dt), name
            for j in args[-1][:args[-2]]:
                log.append(Call(len(log), solo, stream, dict({f: _plain(getattr(j, f)) for f in names}, **dt)))
            return
        assert name in SIG, f"{name}: an entry point of the plan the access table does not classify"
        assert len(args) == len(SIG[name]), name
        log.append(Call(len(log), name, stream, {f: _plain(v) for f, v in zip(SIG[name], args)}))
    return rec


class _Fake:
    """Stands for a device tensor the trace only takes the address of."""

    def __init__(self, ptr):
        self._ptr = ptr

    def data_ptr(self):
        return self._ptr


def _rt(plan, log):
    rt = Rt(plan, BASE, MAIN, plan.training)
    rt.eval_base = EBASE
    for i in plan.stem_inputs:
        rt.stem_x[i] = _Fake(XBASE)
    return rt


def trace_fwd(plan, monkeypatch):
    """-> [Call] of the plan's forward as _PlanFn.forward / runner.run issue it on one stream: the input
    loads, the step's weight packs (training; as one batched job list), then op.fwd over plan.sched."""
    log = []
    with monkeypatch.context() as mp:
        mp.setattr(L, "call", recorder(log))
        rt = _rt(plan, log)
        n, sizes = plan.n, [(v.c, v.h, v.w) for v in plan.inputs]
        runner._load_inputs(plan, rt, [torch.empty(n, c, h, w, device="meta") for c, h, w in sizes])
        if plan.training:
            specs = [sp for op in plan.ops for sp in op.pack_specs()]
            plan.prepack(rt, (_Fake(XBASE), len(specs), []))
        for op in plan.sched:
            op.fwd(rt)
    assert all(c.stream == MAIN for c in log)
    return log


def trace_bwd(plan, params, monkeypatch):
    """-> [Call] of the plan's backward as _PlanFn.backward runs it (the op loop; what comes before it
    is main-stream work ahead of every weight gradient, what comes after follows the streams' join)."""
    log = []
    with monkeypatch.context() as mp:
        mp.setattr(L, "call", recorder(log))
        rt = _rt(plan, log)
        ptrs, off = [None] * len(params), 0
        for i in plan.pgrad_order:                      # the runner's flat gradient arena
            if params[i].requires_grad:
                ptrs[i] = PBASE + 4 * off
                off += params[i].numel()
        rt.gbase, rt.pgrad = GBASE, lambda i: ptrs[i]
        rt.main = _Stream(MAIN, log)
        rt.side = _Stream(SIDE, log) if plan.opts.wgrad_stream else None
        rt._ev = _Event(log)
        for step in reversed(plan.sched):
            step.bwd(rt)
    assert all(c.stream in (MAIN, SIDE) for c in log)
    return log


# ---- access table ------------------------------------------------------------------------------------
class Range:
    """Bytes [lo, hi); a view's also (address, channel stride, channel slice rounded up to whole 16-byte
    groups, end of the exact slice) in bytes, which decides against another view of the same address and
    stride."""

    def __init__(self, what, lo, hi, view=None):
        self.what, self.lo, self.hi, self.view = what, lo, hi, view

    def hits(self, o):
        if self.hi <= o.lo or o.hi <= self.lo:
            return False
        if self.view and o.view and self.view[:2] == o.view[:2]:
            return self.view[2] < o.view[3] and o.view[2] < self.view[3]
        return True

    def __repr__(self):
        return f"{self.what}[{self.lo:#x}, {self.hi:#x})"


def _es(dtype):
    return 4 if dtype == L.F32 else 2


def flat(what, ptr, nbytes):
    return [Range(what, ptr, ptr + int(nbytes))] if ptr is not None and nbytes > 0 else []


def view(what, ptr, ld, off, pixels, c, es):
    """Element (p, ch) of a view lives at ptr[p * ld + off + ch]; the kernels move whole 16-byte groups
    and producers keep the channels up to the next multiple of 8 zero, so the slice is rounded up to 8."""
    if ptr is None:
        return []
    c8 = (c + 7) // 8 * 8
    assert ld % 8 == 0 and off % 8 == 0 and off + c8 <= ld and pixels > 0, (what, ld, off, c)
    return [Range(what, ptr + off * es, ptr + ((pixels - 1) * ld + off + c8) * es,
                  (ptr, ld * es, off * es, (off + c8) * es, (off + c) * es))]


def _conv(a):
    s = a["shape"]
    return s, _es(s.dtype), s.n * s.h * s.w, s.n * s.ho * s.wo


def acc_conv_dgrad(a):
    s, es, pin, pout = _conv(a)
    dx = view("dx", a["dx"], a["dx_ld"], a["dx_off"], pin, s.cin, es)
    r = view("dz", a["dz"], a["dz_ld"], a["dz_off"], pout, s.cout, es)
    r += flat("wpacked_t", a["wpacked_t"], L.lib().yms_conv_packed_elems(ctypes.byref(s), 1) * es)
    return r + (dx if a["accumulate"] else []), dx


def acc_conv_dgrad_bnred(a):
    s, es, pin, _ = _conv(a)
    r, w = acc_conv_dgrad(a)
    r = r + view("z", a["z"], a["z_ld"], a["z_off"], pin, s.cin, es)
    r += flat("scale", a["scale"], 4 * s.cin) + flat("shift", a["shift"], 4 * s.cin)
    r += flat("mean_invstd", a["mean_invstd"], 8 * s.cin)
    rows = L.lib().yms_conv_dgrad_bnred_rows(ctypes.byref(s))
    assert rows > 0
    return r, w + flat("bnred ws", a["ws"], 4 * rows * 2 * s.cin)


def acc_conv_wgrad(a):
    s, es, pin, pout = _conv(a)
    r = view("x", a["x"], a["x_ld"], a["x_off"], pin, s.cin, es)
    r += view("dz", a["dz"], a["dz_ld"], a["dz_off"], pout, s.cout, es)
    w = flat("ws", a["ws"], a["ws_bytes"]) + flat("dw", a["dw"], 4 * s.cout * s.cin * s.k * s.k)
    return r + w, w


def acc_dw(a, x, dx):
    s = a["shape"]
    es, pix = _es(s.dtype), s.n * s.h * s.w
    return s, [view(k, a[k], a[k + "_ld"], a[k + "_off"], pix, s.c, es) for k in (x, dx)]


def acc_dwconv_wgrad(a):
    s, (x, dz) = acc_dw(a, "x", "dz")
    w = flat("ws", a["ws"], a["ws_bytes"]) + flat("dw", a["dw"], 4 * s.c * s.k * s.k)
    return x + dz + w, w


def acc_dwconv_dgrad(a):
    s, (dz, dx) = acc_dw(a, "dz", "dx")
    return dz + flat("w", a["w"], 4 * s.c * s.k * s.k) + (dx if a["accumulate"] else []), dx


def acc_stem_wgrad(a):
    s, es, pin, pout = _conv(a)
    r = flat("x", a["x"], 4 * pin * s.cin)              # the NCHW fp32 input
    r += view("gy", a["gy"], a["gy_ld"], a["gy_off"], pout, s.cout, es)
    r += view("z", a["z"], a["z_ld"], a["z_off"], pout, s.cout, es)
    r += flat("scale", a["scale"], 4 * s.cout) + flat("shift", a["shift"], 4 * s.cout)
    r += flat("mean_invstd", a["mean_invstd"], 8 * s.cout) + flat("coef", a["coef"], 8 * s.cout)
    w = flat("ws", a["ws"], a["ws_bytes"]) + flat("dw", a["dw"], 4 * s.cout * s.cin * s.k * s.k)
    return r + w, w


def _pass_reads(a):
    c, es = a["c"], _es(a["dtype"])
    r = view("z", a["z"], a["z_ld"], a["z_off"], a["npix"], c, es)
    r += view("gy", a["gy"], a["gy_ld"], a["gy_off"], a["npix"], c, es)
    return r + flat("scale", a["scale"], 4 * c) + flat("shift", a["shift"], 4 * c) + flat("mean_invstd", a["mean_invstd"], 8 * c)


def _rows_bytes(a):
    return 4 * L.lib().yms_bn_bwd_rows(a["npix"], a["c"]) * 2 * a["c"]


def acc_reduce(a):
    return _pass_reads(a), flat("reduce ws", a["ws"], _rows_bytes(a))


def acc_finalize(a):
    c = a["c"]
    w = flat("dgamma", a["dgamma"], 4 * c) + flat("dbeta", a["dbeta"], 4 * c) + flat("coef", a["coef"], 8 * c)
    return flat("partial rows", a["ws"], 4 * a["rows"] * 2 * c) + w, w          # dgamma / dbeta (+=)


def acc_apply(a):
    c, es = a["c"], _es(a["dtype"])
    out = view("out", a["out"], a["out_ld"], a["out_off"], a["npix"], c, es)
    res = view("gres", a["res"], a["res_ld"], a["res_off"], a["npix"], c, es)
    return _pass_reads(a) + flat("coef", a["coef"], 8 * c) + (res if a["res_acc"] else []), out + res


def acc_bias(a):
    w = flat("bias ws", a["ws"], _rows_bytes(a)) + flat("counter", a["counter"], 16) + flat("dbias", a["dbias"], 4 * a["c"])
    return view("gy", a["gy"], a["gy_ld"], a["gy_off"], a["npix"], a["c"], _es(a["dtype"])) + w, w


def acc_copy(a):
    return flat("src", a["src"], a["bytes"]), flat("dst", a["dst"], a["bytes"])


def acc_add_views(a):
    es = _es(a["dtype"])
    y = view("y", a["y"], a["y_ld"], a["y_off"], a["npix"], a["c"], es)
    r = [r for k in "ab" for r in view(k, a[k], a[k + "_ld"], a[k + "_off"], a["npix"], a["c"], es)]
    return r + (y if a["accumulate"] else []), y


def acc_add_grad2(a):
    es = _es(a["dtype"])
    ga, gb = (view(k, a[k], a[k + "_ld"], a[k + "_off"], a["npix"], a["c"], es) for k in ("ga", "gb"))
    r = view("g", a["g"], a["g_ld"], a["g_off"], a["npix"], a["c"], es)
    return r + (ga if a["acc1"] else []) + (gb if a["acc2"] else []), ga + gb


def acc_upsample_bwd(a):
    es, pix = _es(a["dtype"]), a["n"] * a["h"] * a["w"]
    gx = view("gx", a["gx"], a["gx_ld"], a["gx_off"], pix, a["c"], es)
    return view("gy", a["gy"], a["gy_ld"], a["gy_off"], 4 * pix, a["c"], es) + (gx if a["accumulate"] else []), gx


def acc_sppf_bwd(a):
    es, pix = _es(a["dtype"]), a["n"] * a["h"] * a["w"]
    g = view("gbuf", a["gbuf"], a["gld"], a["goff"], pix, 4 * a["c"], es)
    w = g + flat("sppf ws", a["ws"], L.lib().yms_sppf_ws_bytes(a["n"], a["h"], a["w"], a["c"]))
    return view("buf", a["buf"], a["ld"], a["off"], pix, 4 * a["c"], es) + w, w


# ---- the forward (yms.h: yms_conv_fwd .. yms_add_views) ------------------------------------------------
def _stats(a, rows, ld):
    return flat("stats", a["stats"], 4 * rows * (2 * ld + 1))


def _epilogue(a, c):
    return flat("scale", a["scale"], 4 * c) + flat("shift", a["shift"], 4 * c)


def acc_conv_fwd(a):
    s, es, pin, pout = _conv(a)
    sp = ctypes.byref(s)
    r = view("x", a["x"], a["x_ld"], a["x_off"], pin, s.cin, es)
    r += flat("wpacked", a["wpacked"], L.lib().yms_conv_packed_elems(sp, 0) * es) + _epilogue(a, s.cout)
    r += view("res", a["res"], a["res_ld"], a["res_off"], pout, s.cout, es)
    w = view("y", a["y"], a["y_ld"], a["y_off"], pout, s.cout, es)
    return r, w + _stats(a, L.lib().yms_conv_stats_rows(sp), L.lib().yms_conv_stats_ld(sp))


def acc_stem_fwd(a):
    s, es, pin, pout = _conv(a)
    r = flat("x", a["x"], 4 * pin * s.cin) + flat("w", a["w"], 4 * s.cout * s.cin * s.k * s.k) + _epilogue(a, s.cout)
    w = view("y", a["y"], a["y_ld"], a["y_off"], pout, s.cout, es)
    return r, w + _stats(a, L.lib().yms_conv_stem_stats_rows(ctypes.byref(s)), a["stats_ld"])


def acc_dwconv_fwd(a):
    s, (x, y) = acc_dw(a, "x", "y")
    r = x + flat("w", a["w"], 4 * s.c * s.k * s.k) + _epilogue(a, s.c)
    return r, y + _stats(a, L.lib().yms_dwconv_stats_rows(ctypes.byref(s)), a["stats_ld"])


def acc_bn_finalize(a):
    c, mi_ld = a["c"], a.get("mi_ld", a["c"])
    st = _stats(a, a["rows"], a["stats_ld"])             # consumed: long tables are pre-reduced in place
    state = flat("rmean", a["rmean"], 4 * c) + flat("rvar", a["rvar"], 4 * c)
    w = flat("mean", a["mean_invstd"], 4 * c) + flat("invstd", a["mean_invstd"] + 4 * mi_ld, 4 * c)
    w += flat("scale", a["scale"], 4 * c) + flat("shift", a["shift"], 4 * c)
    return st + state + flat("gamma", a["gamma"], 4 * c) + flat("beta", a["beta"], 4 * c), st + state + w


def acc_affine(a):
    c, es = a["c"], _es(a["dtype"])
    r = view("z", a["z"], a["z_ld"], a["z_off"], a["npix"], c, es) + _epilogue(a, c)
    r += view("res", a["res"], a["res_ld"], a["res_off"], a["npix"], c, es)
    return r, view("y", a["out"], a["out_ld"], a["out_off"], a["npix"], c, es)


def acc_sppf_fwd(a):
    es, pix, c = _es(a["dtype"]), a["n"] * a["h"] * a["w"], a["c"]
    return view("slot 0", a["buf"], a["ld"], a["off"], pix, c, es), view("slots 1..3", a["buf"], a["ld"], a["off"] + c, pix, 3 * c, es)


def acc_upsample_fwd(a):
    es, pix = _es(a["dtype"]), a["n"] * a["h"] * a["w"]
    return (view("x", a["x"], a["x_ld"], a["x_off"], pix, a["c"], es),
            view("y", a["y"], a["y_ld"], a["y_off"], 4 * pix, a["c"], es))


def acc_pack_input(a):
    pix = a["n"] * a["h"] * a["w"]
    # "channels padded with zeros up to ld": the whole pixel row is written
    return flat("x", a["x"], 4 * pix * a["c"]), view("y", a["y"], a["ld"], 0, pix, a["ld"], _es(a["dtype"]))


def acc_nchw_to_nhwc(a):
    pix = a["n"] * a["h"] * a["w"]
    y = view("y", a["y"], a["ld"], a["off"], pix, a["c"], _es(a["dtype"]))
    return flat("x", a["x"], _es(a["dtype_nchw"]) * pix * a["c"]) + (y if a["accumulate"] else []), y


def acc_pack_batched(a):
    # the destinations (byte offsets from dst_base) are in the device job table, which a trace does not hold
    return flat("jobs", a["jobs"], a["njobs"] * ctypes.sizeof(L.PackJob)), []


def acc_pack_weight(a):
    s = a["shape"]
    es = _es(s.dtype)
    return (flat("w", a["w"], 4 * s.cout * s.cin * s.k * s.k),
            flat("packed", a["packed"], L.lib().yms_conv_packed_elems(ctypes.byref(s), a["for_dgrad"]) * es))


ACCESS = {"yms_conv_dgrad": acc_conv_dgrad, "yms_conv_dgrad_bnred": acc_conv_dgrad_bnred, "yms_conv_wgrad": acc_conv_wgrad,
          "yms_conv_stem_wgrad": acc_stem_wgrad, "yms_dwconv_dgrad": acc_dwconv_dgrad, "yms_dwconv_wgrad": acc_dwconv_wgrad,
          "yms_bn_act_bwd_reduce": acc_reduce, "yms_bn_act_bwd_finalize": acc_finalize, "yms_bn_act_bwd_apply": acc_apply,
          "yms_bias_bwd": acc_bias, "yms_copy": acc_copy, "yms_add_views": acc_add_views, "yms_add_grad2": acc_add_grad2,
          "yms_upsample2x_bwd": acc_upsample_bwd, "yms_sppf_pool_bwd": acc_sppf_bwd,
          "yms_conv_fwd": acc_conv_fwd, "yms_conv_stem_fwd": acc_stem_fwd, "yms_dwconv_fwd": acc_dwconv_fwd,
          "yms_bn_finalize": acc_bn_finalize, "yms_bn_finalize_ld": acc_bn_finalize, "yms_affine_act": acc_affine,
          "yms_sppf_pool_fwd": acc_sppf_fwd, "yms_upsample2x_fwd": acc_upsample_fwd, "yms_pack_input": acc_pack_input,
          "yms_nchw_to_nhwc": acc_nchw_to_nhwc, "yms_conv_pack_weights_batched": acc_pack_batched,
          "yms_conv_pack_weight": acc_pack_weight}
assert ACCESS.keys() == SIG.keys()


# ---- define before use ---------------------------------------------------------------------------------
class Uninit:
    """A call (None: a seeded output gradient) reads channel bytes [lo, hi) of the buffer at ptr that
    nothing wrote before."""

    def __init__(self, call, what, ptr, lo, hi):
        self.call, self.what, self.ptr, self.lo, self.hi = call, what, ptr, lo, hi

    def __repr__(self):
        return f"{self.call}: {self.what} reads unwritten channel bytes [{self.lo}, {self.hi}) of the buffer at {self.ptr:#x}"


class Coverage:
    """Per buffer (its base address) the channel byte intervals written so far, at the granularity the
    kernels move data in: a read of a view takes its whole 16-byte groups of every pixel, a write covers
    its exact channels only; a zero range covers every channel of the buffer it starts at."""
    ALL = 1 << 40

    def __init__(self):
        self.ivs, self.found = {}, []

    def write(self, ptr, lo, hi):
        self.ivs.setdefault(ptr, []).append((lo, hi))

    def zero(self, base, ranges):
        for off, _ in ranges:
            self.write(base + off, 0, self.ALL)

    def gap(self, ptr, lo, hi):
        """-> the first unwritten (lo, hi) inside [lo, hi) or None."""
        cur = lo
        for a, b in sorted(self.ivs.get(ptr, [])):
            if a > cur:
                break
            cur = max(cur, b)
            if cur >= hi:
                return None
        nxt = min([a for a, _ in self.ivs.get(ptr, []) if a > cur] + [hi])
        return cur, nxt

    def read(self, call, what, ptr, lo, hi):
        g = self.gap(ptr, lo, hi)
        if g is not None:
            self.found.append(Uninit(call, what, ptr, *g))

    def run(self, log):
        for c in log:
            reads, writes = ACCESS[c.name](c.a)
            for r in reads:
                if r.view:
                    self.read(c, r.what, r.view[0], r.view[2], r.view[3])
            for w in writes:
                if w.view:
                    self.write(w.view[0], w.view[2], w.view[4])


def uninitialised(plan, fwd, bwd=None):
    """-> [Uninit] of a plan's traced forward (and backward), in the order the runner issues things:
    zero_ranges, the forward, gzero_ranges, the seeded output gradients (an accumulating seed reads its
    slice first; rt.gover's tensor is the same write), the backward."""
    cov = Coverage()
    cov.zero(BASE, plan.zero_ranges)
    cov.run(fwd)
    if bwd is not None:
        cov.zero(GBASE, plan.gzero_ranges)
        for v, acc in zip(plan.outputs, plan.seed_acc):
            ptr, lo, hi = GBASE + v.buf.off, v.off * plan.es, (v.off + v.c) * plan.es
            if acc:
                cov.read(None, "seed", ptr, lo, hi)
            cov.write(ptr, lo, hi)
        cov.run(bwd)
    return cov.found
