"""The training step's stream and scheduling switches (plan.Options) at plan level: two consecutive steps
(forward, ComputeLoss total, backward, plain SGD in between) of a whole model on the well-conditioned
fixture (oracle.model_ref.ordered_init), with every head map, the loss, every parameter gradient and
every buffer of both steps collected.  The second step shows that the updated weights reach the
side-stream packs and that nothing of step 1 is still in flight when step 2 reuses its memory.

a. YMS_WGRAD_STREAM, YMS_GRAD_INPLACE and YMS_WGRAD_FIRST change only where and in which order passes
   are enqueued, and the weight gradients are deterministic (split-K slabs and a reduce, no atomics),
   so each of them alone and all three together (the default) must give every collected tensor EQUAL,
   bit for bit, to the run with all three off.
b. The routes are really taken (yms._lib.call wrapped in a counting pass-through): with the stream on
   every weight gradient launch carries a stream that is not the main one's, with it off none does;
   with grad-inplace on the backward's yms_copy count drops by the number of head maps; with
   wgrad-first on the layer after the stem issues its weight gradient before its input gradient.
   The in-place path needs the incoming gradient to BE the buffer's gradient (runner._seed_grad:
   c == ld).  ("n", 3) does not take it: its head maps are 67 channels in a channel stride of 72, the
   loss's gradient is a 67-channel slice of a 72-wide tensor and goes through yms_nchw_to_nhwc with
   the switch on or off, so no yms_copy is issued either way.  fp32 plans have no stem kernel, hence no
   layer "after the stem": YMS_WGRAD_FIRST marks nothing there.
c. A lagging side stream: before each forward and each backward ~0.1 s of matmuls is enqueued on the
   side stream, so the forward's weight packs and every weight gradient start only after the host has
   enqueued the main stream's whole pass (asserted: the filler is still running when the call
   returns).  A main-stream overwrite of something a weight gradient still needs (tests/
   test_stream_hazards_cpu.py audits the same property on the traced calls) is then a deterministic
   mismatch instead of a rare race.  All accesses stay inside allocated memory.
d. YMS_BNRED (the BN-backward reduce in the consumer's input gradient) on and off, bf16, one step with
   the sum(o^2).mean() loss: maps and buffers bit-equal (the switch touches the backward only); the
   gradients differ by fp32 summation order, gated against the reference's own bf16 drift.

The switches passed (a)-(d) as they stand: no mismatch was found in the library.
"""
import functools

import pytest
import torch

from oracle import model_ref as M
from oracle import ms_ref as MS
from test_train_conditioned_gpu import _cpu, _rel
from yms import _lib as L
from yms import runner, set_compute_dtype
from yms.plan import ConvOp
from yolov8.tools.loss import ComputeLoss
from yolov8.yolov8 import YOLOv8

pytestmark = pytest.mark.gpu

SWITCHES = ("YMS_WGRAD_STREAM", "YMS_GRAD_INPLACE", "YMS_WGRAD_FIRST")
OFF = (0, 0, 0)
COMBOS = {"stream": (1, 0, 0), "inplace": (0, 1, 0), "first": (0, 0, 1), "all": (1, 1, 1)}
SIZES = {"n": (64, 64), "ms-xs": (96, 128), "ms-s": (96, 128)}
# ("n", 3): ragged head width 67 -> ld 72; ms-xs: depthwise weight gradients, add_grad2, the in-place [X|Y] slices
CASES = [("n", 80, torch.bfloat16), ("n", 3, torch.bfloat16), ("ms-xs", 80, torch.bfloat16),
         ("n", 80, torch.float32), ("n", 80, torch.float16)]
WGRADS = ("yms_conv_wgrad", "yms_dwconv_wgrad")
TARGETS = [[0, 1, 0.5, 0.5, 0.4, 0.3], [1, 2, 0.3, 0.6, 0.2, 0.5], [1, 0, 0.7, 0.2, 0.3, 0.3]]


def _ids(v):
    return str(v).replace("torch.", "") if isinstance(v, torch.dtype) else None


@functools.lru_cache(maxsize=None)
def _fixture(v, nc, size=None):
    sd = M.ordered_init((MS if v.startswith("ms-") else M).init_params(v, nc))
    x = torch.randn(2, 3, *(size or SIZES[v]), generator=torch.Generator().manual_seed(7 + nc))
    return sd, x


_FILL = {}


def _lag(side, ms=120.0):
    """~ms of matmuls on the side stream -> the event that ends them."""
    if not _FILL:
        a = torch.full((4096, 4096), 1.0 / 4096, device="cuda")
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):                  # the second round is the timed one
            t0.record()
            for _ in range(8):
                a @ a
            t1.record()
        torch.cuda.synchronize()
        _FILL["a"], _FILL["per"] = a, max(t0.elapsed_time(t1) / 8, 1e-3)
    a = _FILL["a"]
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(int(ms / _FILL["per"]) + 1):
            a @ a
        done = torch.cuda.Event()
        done.record()
    return done


def _run(v, nc, dtype, env, lag=False, steps=2, det_loss=True, size=None):
    """-> ({name: tensor on the CPU}, [(phase, entry point, args)], the training plan)."""
    sd, x = _fixture(v, nc, size)
    calls, phase = [], ["setup"]
    real = L.call

    def counted(name, *args):
        calls.append((phase[0], name, args))
        return real(name, *args)

    with pytest.MonkeyPatch.context() as mp:
        for k, val in env.items():
            mp.setenv(k, str(val))
        mp.setattr(L, "call", counted)       # call_job and every op resolve `call` through the module
        m = YOLOv8(v, nc).cuda()
        m.load_state_dict(sd)
        set_compute_dtype(m, dtype)
        m.train()
        xg = x.cuda()
        crit = ComputeLoss(m.head, nc, "cuda", tuple(x.shape[2:]))
        tg = torch.tensor(TARGETS, device="cuda")
        opt = torch.optim.SGD(m.parameters(), lr=0.01)
        side = runner._side_stream(xg.device)
        out = {}
        for s in range(steps):
            opt.zero_grad(set_to_none=True)
            phase[0] = f"fwd{s}"
            busy = _lag(side) if lag else None
            outs = m(xg)
            assert busy is None or not busy.query(), "the side stream's filler ended before the forward was enqueued"
            for i, o in enumerate(outs):
                out[f"s{s}:map{i}"] = o.detach().clone()
            phase[0] = f"loss{s}"
            if det_loss:
                total = crit.loss_tensor(outs, tg)[0]        # ComputeLoss's total, without forward()'s host sync
            else:
                total = sum((o.double() ** 2).mean() for o in outs)
            phase[0] = f"bwd{s}"
            busy = _lag(side) if lag else None
            total.backward()
            assert busy is None or not busy.query(), "the side stream's filler ended before the backward was enqueued"
            phase[0] = "host"
            out[f"s{s}:loss"] = total.detach().clone()
            for k, p in m.named_parameters():
                if k != "head.dfl.conv.weight":
                    assert p.grad is not None, k
                    out[f"s{s}:grad:{k}"] = p.grad.clone()
            for k, b in m.named_buffers():
                out[f"s{s}:buf:{k}"] = b.clone()
            if s + 1 < steps:
                opt.step()
        torch.cuda.synchronize()
        plans = list(m.__dict__["_yms_plans"].values())
    assert len(plans) == 1 and plans[0].training
    return {k: t.cpu() for k, t in out.items()}, calls, plans[0]


_RUNS = {}


def _cached(v, nc, dtype, sw):
    """One run per (case, switch setting), shared by the tests and left unchanged."""
    key = (v, nc, dtype, sw)
    if key not in _RUNS:
        _RUNS[key] = _run(v, nc, dtype, dict(zip(SWITCHES, sw)))
    return _RUNS[key]


def _assert_same(got, base, what):
    assert got.keys() == base.keys()
    bad = [k for k in base if not torch.equal(got[k], base[k])]
    assert not bad, f"{what}: {len(bad)} of {len(base)} tensors differ from the baseline, first {bad[:4]}"


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("v,nc,dtype", CASES, ids=_ids)
def test_order_only_switches_are_bit_identical(v, nc, dtype, combo):
    base, _, bplan = _cached(v, nc, dtype, OFF)
    got, _, plan = _cached(v, nc, dtype, COMBOS[combo])
    o = plan.opts
    assert (o.wgrad_stream, o.grad_inplace, o.wgrad_tail_first) == tuple(map(bool, COMBOS[combo]))
    assert (bplan.opts.wgrad_stream, bplan.opts.grad_inplace, bplan.opts.wgrad_tail_first) == (False, False, False)
    assert any(k.startswith("s1:grad:") for k in base) and any(k.startswith("s1:buf:") for k in base)
    assert all(torch.isfinite(t.float()).all() for t in base.values())
    # the two steps differ (the SGD step reached the packs and the loss), so step 2 is a test of its own
    assert not torch.equal(base["s0:loss"], base["s1:loss"]) and not torch.equal(base["s0:map0"], base["s1:map0"])
    _assert_same(got, base, combo)


def _streams(calls, names):
    return [a[-1] or 0 for ph, n, a in calls if n in names and ph.startswith("bwd")]


@pytest.mark.parametrize("v,nc,dtype", CASES, ids=_ids)
def test_weight_gradients_take_the_side_stream(v, nc, dtype):
    main = L.stream_ptr(torch.device("cuda", torch.cuda.current_device())) or 0
    side = runner._side_stream(torch.device("cuda", torch.cuda.current_device())).cuda_stream
    assert side != main
    n_w = {}
    for sw in (OFF, COMBOS["stream"], COMBOS["all"]):
        _, calls, plan = _cached(v, nc, dtype, sw)
        for names in (WGRADS[:1], WGRADS[1:]):
            st = _streams(calls, names)
            n_w.setdefault(names, len(st))
            assert len(st) == n_w[names] and (len(st) > 0) == (names == WGRADS[:1] or v.startswith("ms-"))
            assert all(s == (side if sw[0] else main) for s in st), (sw, names)
        # nothing but the weight gradients (and the forward's packs) goes to the side stream
        other = {n for ph, n, a in calls if n in L._STREAM_LAST and n not in WGRADS and (a[-1] or 0) == side}
        assert other <= ({"yms_conv_pack_weights_batched", "yms_conv_pack_weight"} if sw[0] and plan.stem_inputs else set())


@pytest.mark.parametrize("v,nc,dtype", CASES, ids=_ids)
def test_grad_inplace_drops_the_head_map_copies(v, nc, dtype):
    def copies(sw):
        _, calls, plan = _cached(v, nc, dtype, sw)
        return [sum(n == "yms_copy" for ph, n, a in calls if ph == f"bwd{s}") for s in range(2)], plan

    (off, plan), (on, _), (dflt, _) = copies(OFF), copies(COMBOS["inplace"]), copies(COMBOS["all"])
    assert len(plan.outputs) == 3 and all(v.buf.idx in plan.grad_read_only for v in plan.outputs)
    if nc == 80:            # 144 channels = the channel stride: the loss's gradient is the buffer's gradient
        assert all(v.c == v.buf.ld for v in plan.outputs)
        assert off == [3, 3] and on == dflt == [0, 0]
    else:                   # 67 of 72 (module docstring): no copy to drop
        assert all(v.c == 67 and v.buf.ld == 72 for v in plan.outputs)
        assert off == on == dflt == [0, 0]


def _shape(s):
    s = getattr(s, "contents", s)
    return tuple(getattr(s, f[0]) for f in s._fields_)


@pytest.mark.parametrize("v,nc,dtype", [c for c in CASES if c[2] != torch.float32], ids=_ids)
def test_wgrad_first_reorders_the_layer_after_the_stem(v, nc, dtype):
    for sw, first in ((OFF, False), (COMBOS["first"], True), (COMBOS["all"], True)):
        _, calls, plan = _cached(v, nc, dtype, sw)
        tail = [op for op in plan.ops if getattr(op, "tail_wgrad_first", False)]
        if not first:
            assert not tail
            stem_out = {op.y.buf.idx for op in plan.stem_inputs.values()}
            tail = [op for op in plan.ops if type(op) is ConvOp and op.x.buf.idx in stem_out]
        assert len(tail) == 1 and len(plan.stem_inputs) == 1
        want = _shape(tail[0].shape)
        assert [type(op) is ConvOp and _shape(op.shape) == want for op in plan.ops].count(True) == 1
        for s in range(2):
            seq = [n for ph, n, a in calls if ph == f"bwd{s}" and n in ("yms_conv_wgrad", "yms_conv_dgrad", "yms_conv_dgrad_bnred")
                   and _shape(a[0]) == want]
            assert len(seq) == 2 and seq[0 if first else 1] == "yms_conv_wgrad", (sw, seq)


@pytest.mark.parametrize("v,nc,dtype", CASES, ids=_ids)
def test_lagging_side_stream_changes_nothing(v, nc, dtype):
    base, _, _ = _cached(v, nc, dtype, OFF)
    got, calls, plan = _run(v, nc, dtype, dict(zip(SWITCHES, COMBOS["all"])), lag=True)
    assert plan.opts.wgrad_stream and plan.opts.grad_inplace and plan.opts.wgrad_tail_first
    assert len(_streams(calls, WGRADS)) > 0 and 0 not in _streams(calls, WGRADS)
    _assert_same(got, base, "default switches, side stream held back")


# ---- (d) YMS_BNRED --------------------------------------------------------------------------------
# (v, size, fused pairs): the issue's two cases; "ms-xs" has no conv the fused reduce supports (its
# direct-kernel input gradients need 32 / 64 reduction channels, ms-xs is 24 / 48 / 112 wide), so there
# the switch must change nothing at all; ("n", 96x128) and "ms-s" add the stride-1 pairs and a YOLO-MS
# graph that does take the route.
BNRED_CASES = [("n", None, 1), ("ms-xs", None, 0), ("n", (96, 128), 6), ("ms-s", None, 1)]


@pytest.mark.parametrize("v,size,pairs", BNRED_CASES)
def test_bnred_route_against_the_separate_reduce(v, size, pairs):
    """d(k) = relative L2 between the two routes' gradients of tensor k; y(k) = relative L2 between the
    CPU oracle under bf16 autocast and the fp64 oracle.  Gate: d(k) <= y(k) / 4 for every k.
    Measured largest d / y on an MI355X (the route changes 2 to 14 of the gradient tensors at all):

        n 64x64      6.4e-6   (backbone.conv0.conv.weight)
        ms-xs        0        (no fused pair: bit-equal)
        n 96x128     6.9e-6   (neck.c2f_2.m.0.conv1.bn.bias)
        ms-s         2.7e-6   (backbone.conv0.bn.bias)

    with the smallest y around 2e-3: five orders of magnitude below the gate; a wrong row table or a
    clobbered scratch region would give O(1)."""
    runs = {}
    for sw in (0, 1):
        runs[sw] = _run(v, 80, torch.bfloat16, {"YMS_BNRED": sw}, steps=1, det_loss=False, size=size)
        fused = [op for op in runs[sw][2].ops if getattr(op, "bnred_for", None) is not None]
        assert len(fused) == (pairs if sw else 0)
        n_fused = sum(n == "yms_conv_dgrad_bnred" for ph, n, a in runs[sw][1])
        n_reduce = sum(n == "yms_bn_act_bwd_reduce" for ph, n, a in runs[sw][1])
        assert n_fused == len(fused)
        runs[sw] += (n_reduce,)
    (off, _, _, red_off), (on, _, _, red_on) = runs[0], runs[1]
    assert red_off - red_on == pairs                    # each fused pair saves its producer's reduce pass
    assert off.keys() == on.keys() and all(torch.isfinite(t.float()).all() for t in off.values())
    grads = [k for k in off if ":grad:" in k]
    _assert_same({k: t for k, t in on.items() if k not in grads}, {k: t for k, t in off.items() if k not in grads}, "YMS_BNRED=1")
    if not pairs:
        _assert_same(on, off, "YMS_BNRED=1 without a fused pair")
    sd, x = _fixture(v, 80, size)
    g64, _, _ = _cpu(v, sd, x, torch.float64)
    gbf, _, _ = _cpu(v, sd, x, torch.float32, autocast=True)
    assert {"s0:grad:" + k for k in g64} == set(grads)
    ratio = sorted((_rel(on["s0:grad:" + k], off["s0:grad:" + k]) / _rel(gbf[k], g64[k]), k) for k in g64)
    differ = sum(r > 0 for r, _ in ratio)
    print(f"{v} {tuple(x.shape[2:])} YMS_BNRED on vs off: {differ} of {len(ratio)} gradients differ, "
          f"largest d/y {ratio[-1][0]:.3g} ({ratio[-1][1]}), smallest y {min(_rel(gbf[k], g64[k]) for k in g64):.3g}")
    assert ratio[-1][0] <= 0.25, ratio[-3:]
