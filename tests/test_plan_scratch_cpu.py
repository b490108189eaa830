"""CPU tier for the plan's scratch ownership (plans built on meta tensors, no GPU): every backward
scratch region is its own range of the grad arena -- the side stream's weight gradients use only
"wgrad", the main stream the others -- and a plan is cached under the options and the direct-conv
route that sized it."""
import dataclasses

import pytest
import torch

from yms import _lib as L
from yms import runner
from yms.plan import ConvOp, SiblingConvOp, read_options
from yolov8.yolov8 import YOLOv8


def _plan(v, dt=torch.bfloat16, training=True, size=64):
    m = YOLOv8(v, 80).train(training)
    x = torch.empty(2, 3, size, size, device="meta")
    return runner.get_plan(m, [x], dt, training)


@pytest.mark.parametrize("v", ["s", "l", "ms-s"])
def test_grad_scratch_regions_are_disjoint_and_sized(v):
    p = _plan(v)
    regions = sorted((p.gscratch[k], p.gscratch[k] + p.scratch_req.get(k, 0), k)
                     for k in ("bwd", "coef", "wgrad", "sppf", "stemwg"))
    assert regions[0][0] >= p.act_bytes                  # after the activation-gradient layout
    for (a0, a1, ka), (b0, b1, kb) in zip(regions, regions[1:]):
        assert a1 <= b0, (ka, kb)
    assert regions[-1][1] <= p.gscratch["cnt"] <= p.garena_bytes
    # every op's weight-gradient workspace fits the shared side-stream region
    for op in p.ops:
        if isinstance(op, ConvOp) and type(op) is ConvOp and op.stem_input is None:
            assert op.wg_ws <= p.scratch_req["wgrad"]


def _stats_bytes(op):
    """The statistics table op's training forward writes, as the library sizes it right now."""
    rows = (L.lib().yms_conv_stem_stats_rows if op.stem_input is not None else L.lib().yms_conv_stats_rows)(op.sp)
    return 4 * rows * (2 * L.lib().yms_conv_stats_ld(op.sp) + 1)


def _stat_convs(p):
    return [c for op in p.ops for c in (op.members if isinstance(op, SiblingConvOp) else [op]) if type(c) is ConvOp]


def test_direct_route_flip_builds_a_fresh_plan():
    """The process-wide direct-conv route changes yms_conv_stats_rows and yms_conv_dgrad_bnred_rows, so
    it is part of the plan-cache key: a module that already holds a plan gets a fresh one, sized under
    the new route and without fused-reduce pairs, and the first plan again once the route is back."""
    m = YOLOv8("s", 80).train()
    x = torch.empty(2, 3, 256, 256, device="meta")
    prev = L.lib().yms_conv_direct_set(-1)
    try:
        L.lib().yms_conv_direct_set(1)
        p1 = runner.get_plan(m, [x], torch.bfloat16, True)
        assert p1.opts.direct == 1 and any(op.bnred_for is not None for op in _stat_convs(p1))
        assert all(_stats_bytes(c) <= p1.scratch_req["stats"] for c in _stat_convs(p1))
        L.lib().yms_conv_direct_set(0)
        p0 = runner.get_plan(m, [x], torch.bfloat16, True)
        assert p0 is not p1 and p0.opts.direct == 0
        assert not any(getattr(op, "bnred_for", None) is not None for op in p0.ops)
        assert all(_stats_bytes(c) <= p0.scratch_req["stats"] for c in _stat_convs(p0))
        L.lib().yms_conv_direct_set(1)
        assert runner.get_plan(m, [x], torch.bfloat16, True) is p1
    finally:
        L.lib().yms_conv_direct_set(prev)


def test_switch_change_after_build_yields_a_fresh_plan(monkeypatch):
    """A plan records the options it was built under (plan.opts = read_options() at that moment, the one
    place the switches are read); a switch changed afterwards makes get_plan build another plan."""
    for name in ("YMS_STEM", "YMS_HEAD_FUSE", "YMS_BNRED", "YMS_WGRAD_FIRST", "YMS_GRAD_INPLACE", "YMS_WGRAD_STREAM"):
        monkeypatch.delenv(name, raising=False)
    m = YOLOv8("s", 80).train()
    x = torch.empty(2, 3, 64, 64, device="meta")
    p = runner.get_plan(m, [x], torch.bfloat16, True)
    base = read_options()
    assert p.opts == base and hash(p.opts) == hash(base) and any(isinstance(op, SiblingConvOp) for op in p.ops)
    monkeypatch.setenv("YMS_HEAD_FUSE", "0")
    p2 = runner.get_plan(m, [x], torch.bfloat16, True)
    assert p2 is not p and not any(isinstance(op, SiblingConvOp) for op in p2.ops)
    assert p2.opts == read_options() == dataclasses.replace(base, head_fuse=False)
    monkeypatch.delenv("YMS_HEAD_FUSE")
    assert runner.get_plan(m, [x], torch.bfloat16, True) is p
    # each switch is one field of the record, read at that one place
    for name, field in (("YMS_STEM", "stem"), ("YMS_BNRED", "bnred"), ("YMS_WGRAD_FIRST", "wgrad_tail_first"),
                        ("YMS_GRAD_INPLACE", "grad_inplace"), ("YMS_WGRAD_STREAM", "wgrad_stream")):
        monkeypatch.setenv(name, "0")
        assert read_options() == dataclasses.replace(base, **{field: False}), name
        monkeypatch.delenv(name)
