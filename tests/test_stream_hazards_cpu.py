"""CPU tier: a trace-based audit of the two-stream backward (plans built on meta tensors, no GPU).

The backward's weight gradients (ConvBase.launch_wgrad, the only user of Rt.wst()) go to a side stream
that waits on the main stream; the main stream never waits on the side stream before _PlanFn.backward
ends.  So the step is correct only if no main-stream pass enqueued AFTER a weight gradient writes what
that weight gradient reads or writes (its x view, its dz, the shared "wgrad" scratch, its dw) or reads
what it writes, and if no main-stream pass at all touches the "wgrad" scratch.

The audit runs step.bwd(rt) over reversed(plan.sched) with yms._lib.call recording every call (entry
point, arguments by name, stream; a grouped call as its member jobs), on an Rt with fake base addresses
and fake stream / event objects, and turns every call into the byte ranges it reads and writes by the
ACCESS table below -- written from the contracts of include/yms.h, not from the plan code.  An entry
point the table does not know fails the audit: a new pass has to be classified.  A view's range knows
its channel slice, so two slots of one buffer (same address, same channel stride) do not overlap.

Negative controls: with the stem's scratch pointed at the side stream's the audit reports the stem's
main-stream weight gradient (what tests/test_stem_plan_cpu.py guards by hand); a weight gradient moved
in front of the apply pass that writes its dz is reported with that pass; and with YMS_WGRAD_STREAM=0
there is no side-stream call at all.

The real plans pass: the audit found no hazard in the library."""
import ctypes

import pytest
import torch

from yms import _lib as L
from yms import runner
from yms.plan import Rt
from yolov8.yolov8 import YOLOv8

BASE, GBASE, PBASE = 1 << 40, 1 << 41, 1 << 43
MAIN, SIDE = 0x1000, 0x2000


# ---- tracing ---------------------------------------------------------------------------------------
# The arguments before the stream, by name (include/yms.h; the per-pixel passes under the field names
# of yms_bn_pass_job, which their grouped forms carry: out = dz, res = gres of yms_bn_act_bwd_apply).
SIG = {k: v.split() for k, v in {
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
}.items()}
# grouped entry point -> its members' solo one; (dtype,) njobs, jobs, stream
GROUPS = {"yms_conv_dgrad_group": "yms_conv_dgrad", "yms_bn_act_bwd_reduce_group": "yms_bn_act_bwd_reduce",
          "yms_bn_act_bwd_finalize_group": "yms_bn_act_bwd_finalize", "yms_bn_act_bwd_apply_group": "yms_bn_act_bwd_apply",
          "yms_bias_bwd_group": "yms_bias_bwd"}


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


def _trace(plan, params, monkeypatch):
    """-> [Call] of the plan's backward as _PlanFn.backward runs it (the op loop; what comes before it
    is main-stream work ahead of every weight gradient, what comes after follows the streams' join)."""
    log = []

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
        assert name in SIG, f"{name}: an entry point of the backward the access table does not classify"
        assert len(args) == len(SIG[name]), name
        log.append(Call(len(log), name, stream, {f: _plain(v) for f, v in zip(SIG[name], args)}))

    with monkeypatch.context() as mp:
        mp.setattr(L, "call", rec)
        rt = Rt(plan, BASE, MAIN, True)
        for i in plan.stem_inputs:
            rt.stem_x[i] = torch.zeros(plan.n, 3, 2 * plan.stem_inputs[i].y.h, 2 * plan.stem_inputs[i].y.w)
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
    """Bytes [lo, hi); a view's also (address, channel stride, channel slice) in bytes, which decides
    against another view of the same address and stride."""

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
    return [Range(what, ptr + off * es, ptr + ((pixels - 1) * ld + off + c8) * es, (ptr, ld * es, off * es, (off + c8) * es))]


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


ACCESS = {"yms_conv_dgrad": acc_conv_dgrad, "yms_conv_dgrad_bnred": acc_conv_dgrad_bnred, "yms_conv_wgrad": acc_conv_wgrad,
          "yms_conv_stem_wgrad": acc_stem_wgrad, "yms_dwconv_dgrad": acc_dwconv_dgrad, "yms_dwconv_wgrad": acc_dwconv_wgrad,
          "yms_bn_act_bwd_reduce": acc_reduce, "yms_bn_act_bwd_finalize": acc_finalize, "yms_bn_act_bwd_apply": acc_apply,
          "yms_bias_bwd": acc_bias, "yms_copy": acc_copy, "yms_add_views": acc_add_views, "yms_add_grad2": acc_add_grad2,
          "yms_upsample2x_bwd": acc_upsample_bwd, "yms_sppf_pool_bwd": acc_sppf_bwd}
assert ACCESS.keys() == SIG.keys()


# ---- the audit ---------------------------------------------------------------------------------------
def audit(plan, log):
    """-> [(rule, side or None, main call, range of the main call, range it meets)] over the three rules."""
    acc = [ACCESS[c.name](c.a) for c in log]
    g = plan.gscratch
    scratch = Range('"wgrad" scratch', GBASE + g["wgrad"], GBASE + g["wgrad"] + max(plan.scratch_req.get("wgrad", 0), 1))
    found = []
    mains = [c for c in log if c.stream == MAIN]
    for m in mains:
        reads, writes = acc[m.pos]
        found += [("main stream in the side stream's scratch", None, m, r, scratch) for r in reads + writes if r.hits(scratch)]
    for s in (c for c in log if c.stream == SIDE):
        s_reads, s_writes = acc[s.pos]
        for m in mains:
            if m.pos < s.pos:
                continue
            m_reads, m_writes = acc[m.pos]
            found += [("written under a weight gradient", s, m, w, r) for w in m_writes for r in s_reads + s_writes if w.hits(r)]
            found += [("weight gradient's output read early", s, m, r, w) for r in m_reads for w in s_writes if r.hits(w)]
    return found


def _model(v, nc):
    return YOLOv8(v, nc).train()


def _plan(m, dtype, size, monkeypatch, **env):
    for k, val in env.items():
        monkeypatch.setenv(k, str(val))
    return runner.get_plan(m, [torch.empty(2, 3, *size, device="meta")], dtype, True)


SIZES = {"n": (64, 64), "ms-xs": (96, 128)}


@pytest.mark.parametrize("group", [0, 2])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("v,nc", [("n", 80), ("n", 3), ("ms-xs", 80)])
def test_no_main_stream_pass_disturbs_a_weight_gradient(v, nc, dtype, group, monkeypatch):
    m = _model(v, nc)
    plan = _plan(m, dtype, SIZES[v], monkeypatch, YMS_HEAD_GROUP=group)
    assert plan.opts.wgrad_stream and bool(plan.groups) == (group > 0)
    log = _trace(plan, plan.params(), monkeypatch)
    side = [c for c in log if c.stream == SIDE]
    # every weight gradient but the stem's is on the side stream, and nothing else is
    assert {c.name for c in side} == {"yms_conv_wgrad"} | ({"yms_dwconv_wgrad"} if v.startswith("ms-") else set())
    assert [c.name for c in log if c.stream == MAIN and "wgrad" in c.name] == ["yms_conv_stem_wgrad"] * len(plan.stem_inputs)
    assert len(plan.stem_inputs) == (dtype != torch.float32)
    n_w = sum(p.dim() == 4 and p.requires_grad for p in plan.params()) - len(plan.stem_inputs)
    n_sib = sum(hasattr(op, "members") for op in plan.ops)
    assert len(side) == n_w - n_sib                     # a sibling pair's two weights: one launch
    assert audit(plan, log) == []


def test_frozen_head_parameters_take_the_members_own_passes(monkeypatch):
    """A frozen weight of a sibling pair: the pair's weight gradient falls back to the other member's own
    launch; a frozen BN bias: dgamma / dbeta go through the "sib" scratch and are copied per member."""
    m = _model("n", 80)
    pd = dict(m.named_parameters())
    pd["head.cls.0.0.conv.weight"].requires_grad_(False)
    pd["head.box.1.0.bn.bias"].requires_grad_(False)
    plan = _plan(m, torch.bfloat16, SIZES["n"], monkeypatch, YMS_HEAD_GROUP=2)
    log = _trace(plan, plan.params(), monkeypatch)
    full = _trace(plan, [torch.nn.Parameter(torch.empty(p.shape, device="meta")) for p in plan.params()], monkeypatch)
    wg = lambda t: [c for c in t if c.name == "yms_conv_wgrad"]        # noqa: E731
    assert len(wg(log)) == len(wg(full)) and sorted(c.a["shape"].cout for c in wg(log)) != sorted(c.a["shape"].cout for c in wg(full))
    assert sum(c.name == "yms_copy" for c in log) == 3 and not any(c.name == "yms_copy" for c in full)
    assert all(c.stream == SIDE for c in wg(log))
    assert audit(plan, log) == []


def test_audit_reports_the_stem_in_the_side_streams_scratch(monkeypatch):
    """Negative control: the stem's weight gradient is the one weight gradient on the main stream, so in
    the region the side stream's weight gradients share it is a real hazard -- and the audit's finding."""
    plan = _plan(_model("n", 80), torch.bfloat16, SIZES["n"], monkeypatch)
    assert plan.scratch_req["stemwg"] > 0 and plan.gscratch["stemwg"] != plan.gscratch["wgrad"]
    assert audit(plan, _trace(plan, plan.params(), monkeypatch)) == []
    plan.gscratch["stemwg"] = plan.gscratch["wgrad"]
    log = _trace(plan, plan.params(), monkeypatch)
    found = audit(plan, log)
    assert found and {f[2].name for f in found} == {"yms_conv_stem_wgrad"}
    assert {f[0] for f in found} == {"main stream in the side stream's scratch", "written under a weight gradient",
                                     "weight gradient's output read early"}
    stem = found[0][2]
    assert stem.stream == MAIN and stem is log[-1]
    # every earlier weight gradient may still be running in that scratch
    assert {f[1].pos for f in found if f[1] is not None} == {c.pos for c in log if c.stream == SIDE}


def test_audit_reports_a_weight_gradient_issued_before_its_dz_is_written(monkeypatch):
    """Negative control on the views: every BN layer's weight gradient reads the dz its apply pass wrote
    over z.  Moved in front of that apply pass, the weight gradient may run under it: the audit names the
    pair, by the channel slice of the one buffer they share."""
    plan = _plan(_model("n", 3), torch.bfloat16, SIZES["n"], monkeypatch, YMS_HEAD_GROUP=2)
    log = _trace(plan, plan.params(), monkeypatch)
    moved = 0
    for s in [c for c in log if c.stream == SIDE]:
        writers = [c for c in log[:s.pos] if c.name == "yms_bn_act_bwd_apply" and c.a["out"] == s.a["dz"]]
        if not writers:
            continue            # the head's biased convs: dz is the head map's gradient
        a = writers[-1]
        assert a.stream == MAIN and (a.a["out_ld"], a.a["out_off"]) == (s.a["dz_ld"], s.a["dz_off"])
        order = log[:a.pos] + [s] + log[a.pos:s.pos] + log[s.pos + 1:]
        bad = [Call(i, c.name, c.stream, c.a) for i, c in enumerate(order)]
        found = audit(plan, bad)
        assert ("written under a weight gradient", a.pos, a.pos + 1, "out", "dz") in {
            (f[0], f[1].pos, f[2].pos, f[3].what, f[4].what) for f in found}
        # and nothing else of that weight gradient is in anybody's way
        assert all(f[1].pos != a.pos or f[2].pos == a.pos + 1 for f in found)
        moved += 1
    assert moved == sum(c.name == "yms_bn_act_bwd_apply" for c in log) > 50       # (the stem has no apply pass: fused)


def test_ranges_know_their_channel_slice():
    es = 2
    box = view("box", BASE, 72, 0, 128, 64, es)[0]
    cls = view("cls", BASE, 72, 64, 128, 3, es)[0]              # channels [64, 67) -> the group [64, 72)
    assert not box.hits(cls) and not cls.hits(box) and box.hits(box) and cls.hits(view("c", BASE, 72, 64, 128, 8, es)[0])
    assert box.hits(view("half", BASE, 72, 32, 128, 8, es)[0])
    # another address or stride: decided by the bytes they span
    assert box.hits(view("other", BASE + 16, 64, 0, 128, 8, es)[0])
    assert not box.hits(view("next", BASE + 128 * 72 * es, 72, 0, 128, 64, es)[0])
    assert box.hits(flat("bytes", BASE + 100, 4)[0]) and not box.hits(flat("bytes", BASE - 4, 4)[0])
    assert view("none", None, 72, 0, 128, 64, es) == [] and flat("none", None, 4) == []
    with pytest.raises(AssertionError):
        view("ragged", BASE, 72, 68, 128, 8, es)


def test_without_the_side_stream_every_call_is_on_the_main_stream(monkeypatch):
    plan = _plan(_model("ms-xs", 80), torch.bfloat16, SIZES["ms-xs"], monkeypatch, YMS_WGRAD_STREAM=0)
    assert not plan.opts.wgrad_stream
    log = _trace(plan, plan.params(), monkeypatch)
    assert log and not [c for c in log if c.stream == SIDE]
    assert {"yms_conv_wgrad", "yms_dwconv_wgrad"} <= {c.name for c in log}
    # ... so all the audit has to say is that the weight gradients, now main-stream calls, use their scratch
    found = audit(plan, log)
    assert {(f[0], f[1], f[2].name) for f in found} == {
        ("main stream in the side stream's scratch", None, n) for n in ("yms_conv_wgrad", "yms_dwconv_wgrad")}
