"""CPU tier: the project's two static audits on fine-tuning plans (meta tensors, no GPU).

tests/test_stream_hazards_cpu.py and tests/test_plan_init_cpu.py trace default plans only.  Here the same
tracing (tests/plan_access.py) runs on plans with frozen layers and eval-mode BatchNorm, with table entries
of this file's own for the entry points those routes add (from the contracts of include/yms.h):
yms_bn_fold_mi, yms_bn_fold_mi_batched, yms_bn_frozen_act_bwd.  The batched pack and fold take their
destinations from device tables a trace cannot read, so their writes are taken from the plan's own job
lists (pack_specs, fold_jobs).

a. The forward's two streams (runner._run_forward, driven with fake streams): the step's packs and folds go
   to the side stream while the stem's forward runs on the main stream, before the two join.  Nothing the
   main stream touches in that window may be written or read-then-written by the side stream.  The stem of
   an eval-mode BN reads its folded scale / shift there: it must fold them itself, on the main stream.
   Negative control: with the stem's fold moved to the side stream the audit names the stem's forward.
b. The backward's two streams (test_stream_hazards_cpu.audit) over Plan.bwd_sched, as the runner walks it.
c. Define before use (plan_access.uninitialised): with some z buffers, backward writes and whole ops gone,
   every 16-byte channel group a call reads was still written before, by a call or a zero range."""
import pytest
import torch

import plan_access as A
from plan_access import BASE, GBASE, MAIN, PBASE, SIDE, XBASE, Call, flat, view
from test_stream_hazards_cpu import audit
from yms import _lib as L
from yms import finetune, runner
from yolov8.yolov8 import YOLOv8

SIG = {k: v.split() for k, v in {
    "yms_bn_fold_mi": "c gamma beta rmean rvar eps scale shift mean_invstd mi_ld",
    "yms_bn_fold_mi_batched": "njobs jobs max_c base",
    "yms_bn_frozen_act_bwd": "dtype npix c z z_ld z_off gy gy_ld gy_off scale shift mean_invstd act "
                             "out out_ld out_off res res_ld res_off res_acc ws counter dgamma dbeta",
}.items()}


def _fold_ranges(c, scale, shift, mi, mi_ld):
    return (flat("scale", scale, 4 * c) + flat("shift", shift, 4 * c) + flat("mean", mi, 4 * c)
            + flat("invstd", mi + 4 * mi_ld, 4 * c))


def acc_fold_mi(a):
    c = a["c"]
    r = [x for k in ("gamma", "beta", "rmean", "rvar") for x in flat(k, a[k], 4 * c)]
    return r, _fold_ranges(c, a["scale"], a["shift"], a["mean_invstd"], a["mi_ld"])


def acc_frozen(a):
    c, es = a["c"], A._es(a["dtype"])
    out = view("out", a["out"], a["out_ld"], a["out_off"], a["npix"], c, es)
    res = view("gres", a["res"], a["res_ld"], a["res_off"], a["npix"], c, es)
    w = out + res
    if a["dgamma"] is not None or a["dbeta"] is not None:
        w = w + flat("ws", a["ws"], A._rows_bytes(a)) + flat("counter", a["counter"], 16)
        w += flat("dgamma", a["dgamma"], 4 * c) + flat("dbeta", a["dbeta"], 4 * c)
    return A._pass_reads(a) + (res if a["res_acc"] else []), w


def _fold_ops(plan):
    return [op for op in plan.ops if op.bn_eval and op.stem_input is None]


def _tables(plan, mp):
    """Classify the new entry points, and give the two batched calls the writes their device tables hold."""
    es = plan.es
    packs = [r for op in plan.ops for sp in op.pack_specs()
             for r in flat("packed", BASE + sp[2], L.lib().yms_conv_packed_elems(sp[0], sp[3]) * es)]
    folds = [r for op in _fold_ops(plan) for j in op.fold_jobs()
             for r in _fold_ranges(j.c, BASE + j.scale, BASE + j.shift, BASE + j.mean_invstd, j.mi_ld)]
    for k, v in SIG.items():
        mp.setitem(A.SIG, k, v)
    mp.setitem(A.ACCESS, "yms_bn_fold_mi", acc_fold_mi)
    mp.setitem(A.ACCESS, "yms_bn_frozen_act_bwd", acc_frozen)
    mp.setitem(A.ACCESS, "yms_bn_fold_mi_batched", lambda a: ([], folds))
    mp.setitem(A.ACCESS, "yms_conv_pack_weights_batched", lambda a: ([], packs))


class _FwdStream:
    def __init__(self, ptr, log, marks):
        self.cuda_stream, self.log, self.marks = ptr, log, marks

    def wait_stream(self, other):
        self.marks.append((self.cuda_stream, other.cuda_stream, len(self.log)))


def trace_forward(plan, mp, two_streams):
    """-> ([Call], [(waiting stream, awaited stream, position)]) of runner._run_forward."""
    log, marks = [], []
    mp.setattr(L, "call", A.recorder(log))
    rt = A._rt(plan, log)
    nspecs = len([sp for op in plan.ops for sp in op.pack_specs()])
    mp.setattr(plan, "pack_table", lambda: (A._Fake(XBASE), nspecs, []))
    fo = _fold_ops(plan)
    plan._fold_now = (A._Fake(XBASE + (1 << 20)), sum(len(op.fold_jobs()) for op in fo), max(op.c for op in fo)) if fo else None
    runner._load_inputs(plan, rt, [torch.empty(plan.n, v.c, v.h, v.w, device="meta") for v in plan.inputs])
    main, side = _FwdStream(MAIN, log, marks), _FwdStream(SIDE, log, marks)
    runner._run_forward(plan, rt, main, side if two_streams else None)
    return log, marks


def audit_forward(log, marks):
    """-> [(side call, main call, the main call's range, the side call's range)] inside the window between
    the side stream's wait on the main stream and the main stream's wait on the side stream."""
    (w0, a0, fork), (w1, a1, join) = marks
    assert (w0, a0, w1, a1) == (SIDE, MAIN, MAIN, SIDE) and fork <= join
    acc = [A.ACCESS[c.name](c.a) for c in log]
    sides = [c for c in log if c.stream == SIDE]
    assert all(c.pos >= fork for c in sides) and all(c.stream == MAIN for c in log[join:])
    found = []
    for s in sides:
        s_r, s_w = acc[s.pos]
        for m in (c for c in log[fork:join] if c.stream == MAIN):
            m_r, m_w = acc[m.pos]
            found += [(s, m, x, y) for x in m_r + m_w for y in s_w if x.hits(y)]
            found += [(s, m, x, y) for x in m_w for y in s_r if x.hits(y)]
    return found


def trace_bwd(plan, mp):
    """plan_access.trace_bwd over Plan.bwd_sched, the walk the runner takes."""
    log, params = [], plan.params()
    mp.setattr(L, "call", A.recorder(log))
    rt = A._rt(plan, log)
    ptrs, off = [None] * len(params), 0
    for i in plan.pgrad_order:
        if params[i].requires_grad:
            ptrs[i] = PBASE + 4 * off
            off += params[i].numel()
    rt.gbase, rt.pgrad, rt.prepacked = GBASE, (lambda i: ptrs[i]), True
    rt.main = A._Stream(MAIN, log)
    rt.side = A._Stream(SIDE, log) if plan.opts.wgrad_stream else None
    rt._ev = A._Event(log)
    for step in plan.bwd_sched:
        step.bwd(rt)
    return log


def _model(v, nc, patterns, ne):
    m = YOLOv8(v, nc).train()
    if patterns:
        finetune.freeze(m, patterns, norm_eval=ne)
    elif ne:
        finetune.norm_eval(m)
    return m


def _plan(m, v, dtype=torch.bfloat16):
    size = (96, 128) if v.startswith("ms-") else (64, 64)
    return runner.get_plan(m, [torch.empty(2, 3, *size, device="meta")], dtype, True)


@pytest.mark.parametrize("patterns,ne", [(["backbone"], True), ([], True), (["backbone"], False), ([], False)],
                         ids=["frozen-prefix", "norm_eval-everywhere", "frozen-train-mode", "default"])
def test_the_stems_forward_meets_nothing_of_the_side_stream(patterns, ne, monkeypatch):
    plan = _plan(_model("n", 80, patterns, ne), "n")
    stem = plan.ops[0]
    assert plan.opts.wgrad_stream and stem.stem_input == 0 and stem.bn_eval == ne
    assert stem.infer == (ne and bool(patterns))
    with monkeypatch.context() as mp:
        _tables(plan, mp)
        log, marks = trace_forward(plan, mp, True)
        names = [c.name for c in log]
        side = [c for c in log if c.stream == SIDE]
        assert [c.name for c in side] == ["yms_conv_pack_weights_batched"] + ["yms_bn_fold_mi_batched"] * ne
        fork, join = marks[0][2], marks[1][2]
        window = [c.name for c in log[fork:join] if c.stream == MAIN]
        # the stem folds its own coefficients on the main stream, before its conv reads them
        own = ["yms_bn_fold_mi"] * ne
        assert window[:len(own) + 1] == own + ["yms_conv_stem_fwd"] and names.count("yms_bn_fold_mi") == len(own)
        assert ("yms_affine_act" in window) == (not stem.infer) and ("yms_bn_finalize" in window) == (not ne)
        assert audit_forward(log, marks) == []
        if not ne:
            return
        # negative control: the stem's fold on the side stream is a race with the stem's forward
        i = names.index("yms_bn_fold_mi")
        bad = [Call(c.pos, c.name, SIDE if c.pos == i else c.stream, c.a) for c in log]
        found = audit_forward(bad, marks)
        assert found and {f[0].pos for f in found} == {i}
        assert {f[1].name for f in found} == {"yms_conv_stem_fwd" if stem.infer else "yms_affine_act"}
        assert {f[3].what for f in found} <= {"scale", "shift"}


CASES = [(["backbone"], False), (["backbone"], True), (["backbone", "neck"], True), ([], True), (["head.cls"], True),
         (["neck.conv1"], True)]


@pytest.mark.parametrize("patterns,ne,one_pass", [c + (1,) for c in CASES] + [c + (0,) for c in CASES if c[1]],
                         ids=lambda c: "+".join(c) if isinstance(c, list) else None)
@pytest.mark.parametrize("v,nc,dtype", [("n", 3, torch.bfloat16), ("n", 80, torch.float32), ("ms-xs", 80, torch.bfloat16)])
def test_hazard_and_initialisation_audits_on_finetune_plans(v, nc, dtype, patterns, ne, one_pass, monkeypatch):
    monkeypatch.setenv("YMS_BN_FROZEN", str(one_pass))
    plan = _plan(_model(v, nc, patterns, ne), v, dtype)
    assert plan.opts.bn_frozen == bool(one_pass) and any(op.bn_eval for op in plan.ops) == ne
    with monkeypatch.context() as mp:
        _tables(plan, mp)
        fwd, _ = trace_forward(plan, mp, False)
        assert all(c.stream == MAIN for c in fwd)
        bwd = trace_bwd(plan, mp)
        names = {c.name for c in bwd}
        served = [op for op in plan.ops if op.bn_eval and op.runs_bwd and type(op).__name__ in ("ConvOp", "DWConvOp")
                  and op.stem_input is None]
        assert ("yms_bn_frozen_act_bwd" in names) == bool(served and one_pass)
        assert audit(plan, bwd) == []
        assert A.uninitialised(plan, fwd, bwd) == []
    # a skipped op launched nothing: no call of the backward names a frozen-prefix layer's z or its gradient
    skipped = [op for op in plan.ops if not op.runs_bwd and getattr(op, "z", None) is not None]
    zs = {BASE + op.z for op in skipped}
    assert not any(c.a.get("z") in zs or c.a.get("dz") in zs for c in bwd)
