"""CPU tier for the head's grouped launches (plans built on meta tensors, no GPU): the HeadGroup's
stages, the members' disjoint slices of the shared scratch regions (sized by the largest stage's sum),
the plan-cache key, and the clean fall-backs -- chains of different shapes build no group, a frozen
member sends the backward through the members' own."""
import dataclasses

import pytest
import torch

from yms import _lib as L
from yms import runner
from yms.plan import (ALIGN, BiasConvOp, Builder, ConvOp, HEAD_GROUP_DEFAULT, HeadGroup, Plan, Rt, SiblingConvOp,
                      read_options)
from yolov8.model.components import Conv, _YmsModule
from yolov8.yolov8 import YOLOv8


def _plan(v="s", nc=80, training=True, size=64, batch=2):
    m = YOLOv8(v, nc).train(training)
    x = torch.empty(batch, 3, size, size, device="meta")
    return runner.get_plan(m, [x], torch.bfloat16, training), m


def _group(p):
    gs = [s for s in p.sched if isinstance(s, HeadGroup)]
    assert gs == p.groups and len(gs) == 1
    return gs[0]


@pytest.mark.parametrize("training", [True, False])
def test_head_runs_as_three_stages(training, monkeypatch):
    monkeypatch.delenv("YMS_HEAD_GROUP", raising=False)
    p, _ = _plan(training=training)
    g = _group(p)
    assert p.opts.head_group == HEAD_GROUP_DEFAULT
    assert g.ops == p.ops[-15:] and p.sched == p.ops[:-15] + [g]        # plan.ops keeps the member ops
    kinds = [[type(op) for op in st] for st in g.stages]
    assert kinds == [[SiblingConvOp] * 3, [ConvOp] * 6, [BiasConvOp] * 6]
    # a stage's members: one op per chain position, in plan order, reading only earlier stages
    for d, st in enumerate(g.stages):
        assert [p.ops.index(op) for op in st] == sorted(p.ops.index(op) for op in st)
        for op in st:
            prod = [q for q in g.ops if q is not op and q.y.buf is op.x.buf]
            assert all(q in g.stages[d - 1] for q in prod) and bool(prod) == (d > 0)


def _slices(st):
    """(region, offset, bytes) of every scratch slice the members of one stage use."""
    out = []
    for op in st:
        rows = L.lib().yms_bn_bwd_rows(op.npix, op.c)
        out.append(("bwd", op.g_bwd, 4 * 2 * op.c * rows))
        if isinstance(op, BiasConvOp):
            continue
        assert rows == op.bwd_rows
        out.append(("coef", op.g_coef, 8 * op.c))
        for m, _ in op.parts():
            out.append(("stats", m.g_stats, 4 * m.stats_rows * (2 * m.stats_ld + 1)))
    return out


@pytest.mark.parametrize("v,nc,size,batch", [("s", 80, 64, 2), ("n", 3, 64, 2), ("s", 80, 640, 64)])
def test_scratch_regions_hold_the_group_sums_without_overlap(v, nc, size, batch, monkeypatch):
    monkeypatch.setenv("YMS_HEAD_GROUP", "2")
    p, _ = _plan(v, nc, size=size, batch=batch)
    for st in _group(p).stages:
        by_region = {}
        for region, off, nb in _slices(st):
            assert off % ALIGN == 0 and nb > 0 and off + nb <= p.scratch_req[region], (region, off, nb)
            by_region.setdefault(region, []).append((off, off + nb))
        for region, ivs in by_region.items():
            ivs.sort()
            assert all(a1 <= b0 for (_, a1), (b0, _) in zip(ivs, ivs[1:])), region
    # ... and still every single op's need, as without grouping
    monkeypatch.setenv("YMS_HEAD_GROUP", "0")
    p0, _ = _plan(v, nc, size=size, batch=batch)
    assert not p0.groups and p0.sched == p0.ops
    for k in ("stats", "bwd", "coef"):
        assert p.scratch_req[k] >= p0.scratch_req[k]
    # YOLOv8-n's widest layer has 256 channels, its head stages hold six BN layers: the region grew
    if v == "n":
        assert p.scratch_req["coef"] > p0.scratch_req["coef"]


def test_switch_is_part_of_the_plan_key(monkeypatch):
    monkeypatch.delenv("YMS_HEAD_GROUP", raising=False)
    m = YOLOv8("n", 3).train()
    x = torch.empty(2, 3, 64, 64, device="meta")
    p = runner.get_plan(m, [x], torch.bfloat16, True)
    base = read_options()
    for mode in (0, 1, 2):
        monkeypatch.setenv("YMS_HEAD_GROUP", str(mode))
        q = runner.get_plan(m, [x], torch.bfloat16, True)
        assert read_options() == dataclasses.replace(base, head_group=mode) == q.opts
        assert (q is p) == (mode == HEAD_GROUP_DEFAULT) and bool(q.groups) == (mode > 0)
    monkeypatch.setenv("YMS_HEAD_GROUP", "fwd")
    with pytest.raises(RuntimeError):
        read_options()


class _TwoChains(_YmsModule):
    """Two independent chains: the same shape (a, b both two convs) or different (b one conv)."""

    def __init__(self, same):
        super().__init__()
        self.a = torch.nn.ModuleList([Conv(16, 16), Conv(16, 16)])
        self.b = torch.nn.ModuleList([Conv(16, 16), Conv(16, 16)] if same else [Conv(16, 16)])

    def emit(self, b, x0, x1):
        outs, ranges = [], []
        for chain, x in ((self.a, x0), (self.b, x1)):
            first = len(b.ops)
            for c in chain:
                x = c.emit(b, x)
            outs.append(x)
            ranges.append((first, len(b.ops)))
        b.independent_chains(ranges)
        return outs


def _two_chain_plan(mod, shared_input=False):
    opts = dataclasses.replace(read_options(), head_group=2)
    b = Builder(2, L.BF16, True, opts)
    if shared_input:
        v = b.new(8, 8, 16)
        ins, outs = [v], mod.emit(b, v, v)
    else:
        ins, outs, _ = mod._yms_plan(b, [torch.empty(2, 16, 8, 8, device="meta")] * 2)
    return Plan(b, ins, outs, "maps")


def test_chains_of_different_shapes_stay_ungrouped():
    p = _two_chain_plan(_TwoChains(True))
    assert len(p.groups) == 1 and [len(st) for st in p.groups[0].stages] == [2, 2] and len(p.sched) == 1
    q = _two_chain_plan(_TwoChains(False))
    assert not q.groups and q.sched == q.ops and len(q.ops) == 3
    # chains that touch common memory (one input feeding both) are not independent: no group
    r = _two_chain_plan(_TwoChains(True), shared_input=True)
    assert not r.groups and r.sched == r.ops


def test_frozen_member_falls_back_to_the_members_backward(monkeypatch):
    monkeypatch.setenv("YMS_HEAD_GROUP", "2")
    p, m = _plan("n", 3)
    g = _group(p)
    params = p.params()

    def rt_for(frozen):
        """Rt with the runner's flat gradient arena layout (plan.pgrad_order) for this freeze pattern."""
        ptrs, off = [None] * len(params), 0
        for i in p.pgrad_order:
            if i not in frozen:
                ptrs[i] = 4096 + 4 * off
                off += params[i].numel()
        rt = Rt(p, 0, None, True)
        rt.pgrad = lambda i: ptrs[i]
        return rt

    assert g.bwd_grouped(rt_for(set()))
    sib, conv, bias = g.stages[0][1], g.stages[1][2], g.stages[2][5]
    for pi in (bias.pbias, bias.pw, conv.pg, conv.pw, sib.members[0].pb, sib.members[1].pw):
        assert not g.bwd_grouped(rt_for({pi})), pi
    # a frozen parameter outside the head does not matter
    assert g.bwd_grouped(rt_for({p.ops[0].pw}))
    # forward-only mode never groups the backward
    monkeypatch.setenv("YMS_HEAD_GROUP", "1")
    p1 = runner.get_plan(m, [torch.empty(2, 3, 64, 64, device="meta")], torch.bfloat16, True)
    rt = rt_for(set())
    rt.plan = p1
    assert p1 is not p and not _group(p1).bwd_grouped(rt)
