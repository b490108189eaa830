"""CPU tier: a trace-based audit of the two-stream backward (plans built on meta tensors, no GPU).

The backward's weight gradients (ConvBase.launch_wgrad, the only user of Rt.wst()) go to a side stream
that waits on the main stream; the main stream never waits on the side stream before _PlanFn.backward
ends.  So the step is correct only if no main-stream pass enqueued AFTER a weight gradient writes what
that weight gradient reads or writes (its x view, its dz, the shared "wgrad" scratch, its dw) or reads
what it writes, and if no main-stream pass at all touches the "wgrad" scratch.

The audit runs step.bwd(rt) over reversed(plan.sched) with yms._lib.call recording every call (entry
point, arguments by name, stream; a grouped call as its member jobs), on an Rt with fake base addresses
and fake stream / event objects, and turns every call into the byte ranges it reads and writes by the
ACCESS table of tests/plan_access.py (the tracing lives there too, shared with tests/test_plan_init_cpu.py)
-- written from the contracts of include/yms.h, not from the plan code.  An entry
point the table does not know fails the audit: a new pass has to be classified.  A view's range knows
its channel slice, so two slots of one buffer (same address, same channel stride) do not overlap.

Negative controls: with the stem's scratch pointed at the side stream's the audit reports the stem's
main-stream weight gradient (what tests/test_stem_plan_cpu.py guards by hand); a weight gradient moved
in front of the apply pass that writes its dz is reported with that pass; and with YMS_WGRAD_STREAM=0
there is no side-stream call at all.

The real plans pass: the audit found no hazard in the library."""
import pytest
import torch

from plan_access import ACCESS, BASE, GBASE, MAIN, SIDE, Call, Range, flat, view
from plan_access import trace_bwd as _trace
from yms import runner
from yolov8.yolov8 import YOLOv8


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
