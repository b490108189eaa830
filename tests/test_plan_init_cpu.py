"""CPU tier: a static define-before-use audit of the plans (built on meta tensors, no GPU).

The plan's arenas come from torch.empty and only plan.zero_ranges / plan.gzero_ranges are cleared, while
the kernels move whole 16-byte channel groups.  So every group a call reads must have been written
earlier in the step or lie in a zeroed range.  tests/test_arena_poison_gpu.py checks that on the GPU by
filling the arenas; this audit names the op when that fails, and reaches plans too large for a GPU test.

tests/plan_access.py traces the forward (input loads, op.fwd over plan.sched) and the backward of a plan
and turns every call into the views it reads and writes by its ACCESS table (written from include/yms.h;
an entry point it does not classify fails the trace).  Activation and activation-gradient views are
followed at 16-byte-group granularity with an interval set per buffer (plan_access.Coverage):

  a read of view (buf, off, c) reads channels [off, off + r8(c)) of every pixel;
  a write covers [off, off + c) only;
  zero_ranges / gzero_ranges are writes of the whole range, at the moment the runner issues them;
  the seeded output gradients (rt.gover's tensors included) are writes.

Scratch regions are left to the GPU test: their row semantics are the kernels' business.

Negative controls: without the z_padding ranges the audit reports the input gradient that reads the
padding of dz (= z) on ("n", 3); with one buffer's entry taken out of gzero_ranges it reports that
buffer's first reader.

The real plans pass: the audit found no read of unwritten memory in the library."""
import functools

import pytest
import torch

import plan_access as A
from yms import runner
from yolov8.yolov8 import YOLOv8

SWITCHES = ("YMS_HEAD_FUSE", "YMS_BNRED", "YMS_STEM", "YMS_GRAD_INPLACE", "YMS_HEAD_GROUP")
OPTIONS = [{}] + [{k: 0} for k in SWITCHES]
SMALL, BENCH = (2, 64, 64), (64, 640, 640)
PLANS = [("n", nc, SMALL) for nc in (1, 3, 17, 80)] + [(v, 80, SMALL) for v in ("s", "ms-xs", "ms-s", "ms-l")]
PLANS += [("s", 80, BENCH), ("ms-s", 80, BENCH)]
DTYPES = [torch.bfloat16, torch.float32]


@functools.lru_cache(maxsize=None)
def _model(v, nc):
    with torch.device("meta"):
        return YOLOv8(v, nc)


def _plan(v, nc, shape, dtype, training, env, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, str(val))
    n, h, w = shape
    return runner.get_plan(_model(v, nc), [torch.empty(n, 3, h, w, device="meta")], dtype, training)


def _audit(plan, monkeypatch):
    fwd = A.trace_fwd(plan, monkeypatch)
    bwd = A.trace_bwd(plan, plan.params(), monkeypatch) if plan.training else None
    return A.uninitialised(plan, fwd, bwd), fwd, bwd


def _ids(v):
    return str(v).replace("torch.", "") if isinstance(v, torch.dtype) else "x".join(map(str, v)) if isinstance(v, tuple) else None


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("v,nc,shape", PLANS, ids=_ids)
def test_every_group_read_was_written(v, nc, shape, dtype, training, monkeypatch):
    for env in OPTIONS:
        plan = _plan(v, nc, shape, dtype, training, env, monkeypatch)
        o = plan.opts
        got = dict(YMS_HEAD_FUSE=o.head_fuse, YMS_BNRED=o.bnred, YMS_STEM=o.stem, YMS_GRAD_INPLACE=o.grad_inplace,
                   YMS_HEAD_GROUP=o.head_group)
        assert all(bool(got[k]) == bool(env.get(k, 1)) for k in SWITCHES) and plan.training == training
        found, fwd, bwd = _audit(plan, monkeypatch)
        assert not found, (env, len(found), found[:4])
        # the trace is the whole step: every op's conv is in it, and in training every BN layer's passes
        names = {c.name for c in fwd}
        assert "yms_conv_fwd" in names and ("yms_affine_act" in names) == training
        assert {"yms_pack_input", "yms_conv_stem_fwd"} & names
        if training:
            assert {"yms_conv_dgrad", "yms_conv_wgrad", "yms_bn_act_bwd_apply"} <= {c.name for c in bwd}


def test_audit_follows_slots_and_padding():
    cov = A.Coverage()
    cov.write(A.BASE, 0, 128)
    cov.write(A.BASE, 128, 134)
    assert cov.gap(A.BASE, 0, 128) is None and cov.gap(A.BASE, 64, 134) is None
    assert cov.gap(A.BASE, 128, 144) == (134, 144)              # the tail group's padding
    assert cov.gap(A.BASE, 160, 176) == (160, 176) and cov.gap(A.BASE + 256, 0, 16) == (0, 16)
    cov.write(A.BASE, 160, 176)
    assert cov.gap(A.BASE, 0, 176) == (134, 160)
    cov.zero(A.BASE, [(0, 4096)])
    assert cov.gap(A.BASE, 0, 1 << 20) is None
    # a view's read is rounded up to whole groups, its write is not
    (r,) = A.view("cls", A.BASE, 72, 64, 128, 3, 2)
    assert r.view[2:] == (128, 144, 134)


def test_audit_reports_the_input_gradient_reading_unzeroed_z_padding(monkeypatch):
    """Negative control (commit 3a9769c): the z buffers of ("n", 3) have padding channels (67 -> 72, 3 -> 8)
    that no pass writes; without their zero ranges the input gradient reads them as dz."""
    plan = _plan("n", 3, SMALL, torch.bfloat16, True, {}, monkeypatch)
    found, fwd, bwd = _audit(plan, monkeypatch)
    assert not found
    pad = [r for op in plan.ops for r in op.z_padding(plan.es)]
    assert pad and all(r in plan.zero_ranges for r in pad)
    full = plan.zero_ranges
    plan.zero_ranges = [r for r in full if r not in pad]
    found = A.uninitialised(plan, fwd, bwd)
    plan.zero_ranges = full                                         # (the model, and its plans, are shared)
    assert found and {f.ptr for f in found} == {A.BASE + off for off, _ in pad}
    dgrads = [f for f in found if f.call.name == "yms_conv_dgrad" and f.what == "dz"]
    assert {f.ptr for f in dgrads} == {f.ptr for f in found}        # every such z has an input gradient reading it
    for f in dgrads:
        s = f.call.a["shape"]
        assert s.cout % 8 and (f.lo, f.hi) == (s.cout * plan.es, (s.cout + 7) // 8 * 8 * plan.es)
    assert {f.call.a["shape"].cout for f in dgrads} == {67, 3}


@pytest.mark.parametrize("v,nc", [("n", 3), ("n", 17)])
def test_audit_reports_the_first_reader_of_an_unzeroed_gradient_buffer(v, nc, monkeypatch):
    """Negative control: a buffer is in gzero_ranges because something reads (or accumulates into) a part
    of its gradient before anything wrote it; taken out, that first reader is the audit's first finding."""
    plan = _plan(v, nc, SMALL, torch.bfloat16, True, {}, monkeypatch)
    found, fwd, bwd = _audit(plan, monkeypatch)
    assert not found
    full = list(plan.gzero_ranges)
    bufs = full[:-1]                                                # the last entry: the arrival counters
    assert bufs and full[-1][0] == plan.gscratch["cnt"]
    for drop in bufs:
        plan.gzero_ranges = [r for r in full if r != drop]
        found = A.uninitialised(plan, fwd, bwd)
        ptr = A.GBASE + drop[0]
        assert found and {f.ptr for f in found} == {ptr}, (drop, found[:3])
        first = found[0]
        if first.call is None:                                      # an accumulating seed of an output gradient
            assert any(o.buf.off == drop[0] for o in plan.outputs)
            continue
        # no earlier call of the backward reads an unwritten group of that buffer: replay up to the finding
        cov = A.Coverage()
        cov.zero(A.BASE, plan.zero_ranges)
        cov.run(fwd)
        cov.zero(A.GBASE, plan.gzero_ranges)
        for o in plan.outputs:
            cov.write(A.GBASE + o.buf.off, o.off * plan.es, (o.off + o.c) * plan.es)
        cov.run(bwd[:first.call.pos])
        assert not cov.found
        reads, _ = A.ACCESS[first.call.name](first.call.a)
        assert any(r.view and r.view[0] == ptr and r.view[2] <= first.lo < r.view[3] for r in reads)
    plan.gzero_ranges = full
