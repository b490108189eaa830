"""CPU tier for the job records (include/yms.h) being the one description of a BN / conv pass.

* The plan: a HeadGroup only collects its members' job records, so with YMS_HEAD_GROUP=2 the head runs
  exactly the passes, with exactly the fields, it runs op by op with YMS_HEAD_GROUP=0 -- up to where in
  the shared scratch regions a member's slice starts -- and every member's passes keep their order.
* The C side: the solo entry point, the grouped one with that job alone and the grouped one with the bad
  job second validate a job identically, before any launch (so no GPU is needed).
"""
import collections
import ctypes

import pytest
import torch

from yms import _lib as L
from yms import runner
from yms.plan import BiasConvOp, HeadGroup, Rt
from yolov8.yolov8 import YOLOv8

BASE, GBASE, EBASE, PBASE = 1 << 40, 1 << 41, 1 << 42, 1 << 43
SCRATCH = ("stats", "ws", "coef", "counter")      # the fields that point into the shared scratch regions


def _regions(plan):
    """[(start, name)] of the scratch regions, and per region the offsets at which a slice may start:
    0, and a HeadGroup member's own slice (HeadGroup.layout)."""
    regs = [(GBASE + off, k) for k, off in plan.gscratch.items()]
    if plan.training:
        regs.append((BASE + plan.scratch["stats"], "stats"))
    starts = {"stats": {0}, "bwd": {0}, "coef": {0}}
    for g in plan.groups if plan.training else ():
        for op in g.ops:
            starts["bwd"].add(op.g_bwd)
            if not isinstance(op, BiasConvOp):
                starts["coef"].add(op.g_coef)
                starts["stats"].update(m.g_stats for m, _ in op.parts())
    return sorted(regs), starts


def _reduce(ptr, regs, starts):
    """A scratch pointer -> (region, 'slice') for the regions members have slices of, (region, offset)
    for the others (the arrival counters, the fused reduce's rows): the regions themselves move when the
    grouped plan sizes "bwd" and "coef" by a stage's sum."""
    if ptr is None:
        return None
    start, name = max((r for r in regs if r[0] <= ptr), default=(None, None))
    assert name is not None, hex(ptr)
    off = ptr - start
    if name in starts:
        assert off in starts[name], (name, off)
        return name, "slice"
    return name, off


def _value(v):
    if isinstance(v, ctypes.Structure):
        return tuple(getattr(v, f[0]) for f in v._fields_)
    if hasattr(v, "contents"):
        return _value(v.contents)
    if isinstance(v, float) or hasattr(v, "value"):
        return ctypes.c_float(getattr(v, "value", v)).value
    return v


def _record(name, fields, dtype, regs, starts):
    """(pass, ((field, value), ...)) of one job; yms_bn_finalize is yms_bn_finalize_ld with mi_ld = c."""
    if name == "yms_bn_finalize":
        fields = dict(fields, mi_ld=fields["c"])
    if "dtype" in L._ARGS[name]:
        fields = dict(fields, dtype=dtype)
    name = {"yms_bn_finalize_ld": "yms_bn_finalize"}.get(name, name)
    return name, tuple(sorted((k, _reduce(v, regs, starts) if k in SCRATCH else _value(v)) for k, v in fields.items()))


def _trace(m, training, mode, monkeypatch):
    """-> [(record, member op index or None)] of one forward (+ backward) of the plan under YMS_HEAD_GROUP=mode,
    the passes that have a job record only; every job of a grouped call is one record."""
    monkeypatch.setenv("YMS_HEAD_GROUP", str(mode))
    plan = runner.get_plan(m, [torch.empty(2, 3, 64, 64, device="meta")], torch.bfloat16, training)
    assert bool(plan.groups) == (mode > 0)
    regs, starts = _regions(plan)
    out, current = [], [None]

    def rec(name, *args):
        solo = L._GROUP_AS.get(name)
        if solo is not None:
            solo = {"yms_bn_finalize": "yms_bn_finalize_ld"}.get(solo, solo)       # the job has an mi_ld
            names = [f for f in L._ARGS[solo] if f != "dtype"]
            dtype = args[0] if "dtype" in L._ARGS[solo] else None
            for j in args[-2][:args[-3]]:
                out.append((_record(solo, {f: getattr(j, f) for f in names}, dtype, regs, starts), current[0]))
        elif name in L._ARGS:
            out.append((_record(name, dict(zip(L._ARGS[name], args)), args[0], regs, starts), current[0]))

    monkeypatch.setattr(L, "call", rec)
    rt = Rt(plan, BASE, None, training)
    rt.eval_base, rt.prepacked = EBASE, True
    for i in plan.stem_inputs:
        rt.stem_x[i] = torch.zeros(2, 3, 64, 64)

    def walk(steps, run):
        for step in steps:
            if isinstance(step, HeadGroup):
                run(step)
                continue
            current[0] = plan.ops.index(step)
            run(step)
            current[0] = None

    walk(plan.sched, lambda s: s.fwd(rt))
    if training:
        params = plan.params()
        ptrs, off = [None] * len(params), 0
        for i in plan.pgrad_order:               # the runner's flat gradient arena
            ptrs[i] = PBASE + 4 * off
            off += params[i].numel()
        rt.gbase, rt.pgrad = GBASE, lambda i: ptrs[i]
        walk(reversed(plan.sched), lambda s: s.bwd(rt))
    monkeypatch.undo()
    return out, plan


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("v,nc", [("n", 3), ("n", 80), ("s", 80)])
def test_grouped_head_runs_the_members_own_jobs(v, nc, training, monkeypatch):
    m = YOLOv8(v, nc).train(training)            # one module: the same parameter addresses in both modes
    solo, _ = _trace(m, training, 0, monkeypatch)
    grouped, plan = _trace(m, training, 2, monkeypatch)
    assert all(who is not None for _, who in solo)
    recs = [r for r, _ in solo]
    assert len(set(recs)) == len(recs)                              # a record names one pass of one op
    assert collections.Counter(recs) == collections.Counter(r for r, _ in grouped)
    # the jobs of the group's calls (who is None) are exactly the jobs of the group's member ops
    member = dict(solo)
    head = {member[r] for r, who in grouped if who is None}
    assert head == {plan.ops.index(op) for g in plan.groups for op in g.ops}
    assert all(who == member[r] for r, who in grouped if who is not None)
    # per member: each pass's jobs in the same order (a sibling pair's parts), and the passes in the
    # same order of first and of last appearance (conv, finalize, affine; reduce, finalize, apply, dgrad).
    # (Not the member's whole sequence: solo, a sibling pair runs conv a, finalize a, conv b, finalize b
    # on the one statistics scratch; grouped, both convs and then both finalizes on the parts' own slices.)
    for op in head:
        seqs = [[r for r, _ in t if member[r] == op] for t in (solo, grouped)]
        kinds = [[r[0] for r in s] for s in seqs]
        for k in set(kinds[0]):
            assert [r for r in seqs[0] if r[0] == k] == [r for r in seqs[1] if r[0] == k], (op, k)
        first = [sorted(set(ks), key=ks.index) for ks in kinds]
        last = [sorted(set(ks), key=ks[::-1].index) for ks in kinds]
        assert first[0] == first[1] and last[0] == last[1], (op, first, last)


# ---- validation: solo == group of one == group with the bad job second ----------------------------
P = 4096          # a non-null address: validation never reads through it
SHAPE = L.ConvShape(2, 8, 8, 16, 16, 3, 1, 1, 8, 8, L.BF16)
GOOD = {
    "yms_conv_fwd": L.ConvFwdJob(SHAPE, P, 16, 0, P, P, 16, 0, P, P, L.ACT_SILU, P, 16, 0, None),
    "yms_conv_dgrad": L.ConvDgradJob(SHAPE, P, 16, 0, P, P, 16, 0, 0),
    "yms_bn_finalize": L.BnFinalizeJob(16, P, 4, 128, 128, P, P, P, P, 0.03, 1e-3, P, 16, P, P),
    "yms_affine_act": L.BnPassJob(npix=128, c=16, z=P, z_ld=16, scale=P, shift=P, out=P, out_ld=16, res=P, res_ld=16),
    "yms_bn_act_bwd_reduce": L.BnPassJob(npix=128, c=16, z=P, z_ld=16, gy=P, gy_ld=16, scale=P, shift=P,
                                         mean_invstd=P, ws=P),
    "yms_bn_act_bwd_finalize": L.BnBwdFinalizeJob(16, P, 2, 128, P, P, P),
    "yms_bn_act_bwd_apply": L.BnPassJob(npix=128, c=16, z=P, z_ld=16, gy=P, gy_ld=16, scale=P, shift=P, mean_invstd=P,
                                        coef=P, out=P, out_ld=16, res=P, res_ld=16),
    "yms_bias_bwd": L.BnPassJob(npix=128, c=16, gy=P, gy_ld=16, ws=P, counter=P, dbias=P),
}
INVALID, UNSUPPORTED = 1, 2
_PASS_VIEWS = {"yms_affine_act": ("z", "out", "res"), "yms_bn_act_bwd_reduce": ("z", "gy"),
               "yms_bn_act_bwd_apply": ("z", "gy", "out", "res"), "yms_bias_bwd": ("gy",)}
_REQUIRED = {"yms_conv_fwd": ("x", "wpacked", "y"), "yms_conv_dgrad": ("dz", "wpacked_t", "dx"),
             "yms_bn_finalize": ("stats", "gamma", "beta", "mean_invstd", "scale", "shift"),
             "yms_affine_act": ("z", "out"), "yms_bn_act_bwd_reduce": ("gy", "ws", "scale", "shift", "mean_invstd"),
             "yms_bn_act_bwd_finalize": ("ws",),
             "yms_bn_act_bwd_apply": ("z", "gy", "out", "scale", "shift", "mean_invstd", "coef"),
             "yms_bias_bwd": ("gy", "ws", "counter")}


def _bad_jobs():
    """(pass, what, {field: value} changes to the good job, expected status)."""
    for name, ptrs in _REQUIRED.items():
        for f in ptrs:
            yield name, f"null {f}", {f: None}, INVALID
    for name, views in _PASS_VIEWS.items():
        for v in views:
            yield name, f"{v}_ld % 8", {v + "_ld": 20}, INVALID
            yield name, f"{v}_off % 8", {v + "_ld": 24, v + "_off": 4}, INVALID
            yield name, f"{v}_off + c > ld", {v + "_off": 8}, INVALID
        wide = {v + "_ld": 2056 for v in views}
        yield name, "c > 2048", dict(wide, c=2056), UNSUPPORTED
        yield name, "c <= 0", {"c": 0}, INVALID
        yield name, "npix <= 0", {"npix": 0}, INVALID
    for name, views in (("yms_conv_fwd", ("x", "y", "res")), ("yms_conv_dgrad", ("dz", "dx"))):
        for v in views:
            yield name, f"{v}_ld % 8", {v + "_ld": 20}, INVALID
            yield name, f"{v}_off + c > ld", {v + "_off": 8}, INVALID
        for f, bad in (("n", 0), ("h", -1), ("k", 5), ("stride", 3), ("ho", 7), ("dtype", 3)):
            sh = L.ConvShape.from_buffer_copy(SHAPE)
            setattr(sh, f, bad)
            yield name, f"shape.{f} = {bad}", {"shape": sh}, INVALID
    for f in ("c", "rows", "count"):
        yield "yms_bn_finalize", f"{f} <= 0", {f: 0}, INVALID
        yield "yms_bn_act_bwd_finalize", f"{f} <= 0", {f: 0}, INVALID
    yield "yms_bn_finalize", "stats_ld < c", {"stats_ld": 8}, INVALID
    yield "yms_bn_finalize", "mi_ld < c", {"mi_ld": 8}, INVALID


@pytest.mark.parametrize("name,what,changes,expect", list(_bad_jobs()), ids=lambda v: v if isinstance(v, str) else None)
def test_solo_and_grouped_calls_reject_a_job_alike(name, what, changes, expect):
    good = GOOD[name]
    bad = type(good).from_buffer_copy(good)
    for f, v in changes.items():
        setattr(bad, f, v)
    lib = L.lib()
    dt = (L.BF16,) if "dtype" in L._ARGS[name] else ()
    solo_name = "yms_bn_finalize_ld" if name == "yms_bn_finalize" else name
    solo = getattr(lib, solo_name)(*L.job_args(solo_name, bad, *dt), None)
    group = getattr(lib, name + "_group")
    one = group(*dt, 1, (type(bad) * 1)(bad), None)
    two = group(*dt, 2, (type(bad) * 2)(good, bad), None)
    assert solo == one == two == expect, (solo, one, two)
