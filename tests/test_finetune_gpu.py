"""Fine-tuning steps of the planned model against fp64 CPU runs of the oracle (tests/finetune_ref.py):
frozen layers (requires_grad False) and BatchNorm modules in eval mode inside a training model.

Model ("n", nc in {3, 80}) at 2x3x64x64 on the well-conditioned fixture (oracle.model_ref.ordered_init),
loss sum(o^2).mean() (test_model_gpu._oracle_grads); ("ms-xs", 80) at 96x128 adds the depthwise layers --
oracle.ms_ref.conv_block takes the same wrapper, so the MS family is compared against the oracle too (its
running statistics calibrated to the input, finetune_ref.fixture).

Gates: fp32 maps within the golden tolerance (1e-3 of the map's maximum), every trainable gradient
within 1e-3 (relative L2) of fp64, frozen parameters without a gradient; eval-mode BN buffers bit-unchanged,
train-mode buffers as the oracle updates them (1e-5, as test_model_gpu); skip on / off bit-identical
gradients; one-pass kernel against the three-pass route fp32 <= 2e-5, bf16 drift from fp32 no larger than
the three-pass route's (median 1.2x, maximum 1.5x: tests/test_sibling_gpu.py's bounds)."""
import functools

import pytest
import torch

import finetune_ref as F
import yms.optim
from test_arena_poison_gpu import PATCHED, _TorchProxy
from test_model_gpu import _maxerr, _rel
from yms import finetune, set_compute_dtype
from yolov8.yolov8 import YOLOv8

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
PATTERNS = [(), ("backbone",), ("backbone", "neck"), ("neck.conv1",), ("head.cls",)]
HAND = ["neck.c2f_2.m.0.conv1"]                     # bn.eval() by hand on one mid-graph layer
CASES = ([(p, ne) for p in PATTERNS for ne in (False, True) if p or not ne]
         + [((), "all"), ((), HAND)])


def _id(c):
    p, ne = c
    tail = {False: "", True: "-normeval", "all": "-normeval_all"}.get(ne if isinstance(ne, (bool, str)) else None, "-hand_eval")
    return "+".join(p or ("none",)) + tail


@functools.lru_cache(maxsize=None)
def _fix(v, nc):
    return F.fixture(v, nc, (96, 128) if v.startswith("ms-") else (64, 64))


@functools.lru_cache(maxsize=None)
def _oracle(v, nc, patterns, ne):
    sd, x = _fix(v, nc)
    frozen = F.frozen_names(sd, patterns)
    ev = F.eval_blocks(sd, patterns, ne if isinstance(ne, (bool, str)) else list(ne), set(frozen))
    return frozen, ev, F.oracle_step(v, nc, sd, x, set(frozen), ev)


def _key(ne):
    return tuple(ne) if isinstance(ne, list) else ne


def _check_against_oracle(v, nc, patterns, ne, r):
    frozen, ev, (maps, g64, bufs) = _oracle(v, nc, patterns, _key(ne))
    for got, ref in zip(r["maps"], maps):
        assert _maxerr(got, ref) < 1e-3
    for k, g in r["grads"].items():
        if k in frozen or k == "head.dfl.conv.weight":
            assert g is None, k
        else:
            assert g is not None and _rel(g, g64[k]) < 1e-3, (k, _rel(g, g64[k]))
    assert set(g64) == {k for k, g in r["grads"].items() if g is not None}
    for k, after in r["after"].items():
        if k.rsplit(".", 2)[0] in ev:
            assert torch.equal(after, r["before"][k]), k        # eval mode: bit-unchanged (fails on the parent)
        elif "running" in k:
            assert _maxerr(after, bufs[k]) < 1e-5, k
        elif k.endswith("num_batches_tracked"):
            assert int(after) == int(bufs[k]) == int(r["before"][k]) + 1, k
    return ev


@pytest.mark.parametrize("case", CASES, ids=_id)
@pytest.mark.parametrize("nc", [3, 80])
def test_fp32_step_vs_fp64_oracle(nc, case):
    patterns, ne = case
    sd, x = _fix("n", nc)
    r = F.gpu_step("n", nc, sd, x, F32, patterns, ne)
    ev = _check_against_oracle("n", nc, patterns, ne, r)
    p = r["plan"]
    assert sum(op.bn_eval for op in p.ops for _ in op.bn_modules()) == len(ev)
    if patterns[:1] == ("backbone",):
        assert any(not op.runs_bwd for op in p.ops) and any(op.infer for op in p.ops) == (ne is True)


@pytest.mark.parametrize("case", [(("backbone",), True), ((), "all")], ids=_id)
def test_ms_fp32_step_vs_fp64_oracle(case):
    """The MS family (depthwise layers, MS-Block sums) through the same oracle wrapper."""
    patterns, ne = case
    sd, x = _fix("ms-xs", 80)
    _check_against_oracle("ms-xs", 80, patterns, ne, F.gpu_step("ms-xs", 80, sd, x, F32, patterns, ne))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [c for c in CASES if c[1] is not True] + [(("head.cls",), True)], ids=_id)
def test_skip_on_and_off_give_the_same_bits(case, dtype):
    """The skip removes launches whose results nobody reads: every gradient, map and buffer is bit-equal
    to the run with YMS_BWD_SKIP=0.  (With norm_eval over a frozen prefix the skip also moves that prefix
    to the inference route, whose activations are the eval plan's -- the next test -- not the z route's.)"""
    patterns, ne = case
    sd, x = _fix("n", 3)
    on = F.gpu_step("n", 3, sd, x, dtype, patterns, ne)
    off = F.gpu_step("n", 3, sd, x, dtype, patterns, ne, env={"YMS_BWD_SKIP": 0})
    assert all(op.runs_bwd for op in off["plan"].ops) and not any(op.infer for op in on["plan"].ops)
    assert all(op.runs_bwd for op in on["plan"].ops) == (not patterns or patterns in (("neck.conv1",), ("head.cls",)))
    for a, b in zip(on["maps"], off["maps"]):
        assert torch.equal(a, b)
    for k, g in on["grads"].items():
        assert (g is None) == (off["grads"][k] is None) and (g is None or torch.equal(g, off["grads"][k])), k
    for k, t in on["after"].items():
        assert torch.equal(t, off["after"][k]), k


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_frozen_prefix_on_the_inference_route_gives_the_eval_plans_activations(dtype):
    sd, x = _fix("n", 80)
    m = YOLOv8("n", 80).cuda()
    m.load_state_dict(sd)
    set_compute_dtype(m, dtype)
    m.train()
    finetune.freeze(m, ["backbone"])
    xg = x.cuda()
    got = [t.clone() for t in m.backbone(xg)]               # the backbone's own training plan: all inference route
    plan = [p for p in m.backbone.__dict__["_yms_plans"].values() if p.training][0]
    assert all(op.infer for op in plan.ops if op.bn_modules()) and not plan.bwd_sched
    before = {k: t.clone() for k, t in m.named_buffers()}
    m.backbone.eval()
    ref = m.backbone(xg)
    torch.cuda.synchronize()
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    assert all(torch.equal(t, before[k]) for k, t in m.named_buffers())


def _grads(r):
    return {k: g.double().cpu() for k, g in r["grads"].items() if g is not None}


@pytest.mark.parametrize("v,nc", [("n", 3), ("ms-xs", 80)])
@pytest.mark.parametrize("case", [((), "all"), (("head.cls",), True)], ids=_id)
def test_one_pass_kernel_against_the_three_pass_route(case, v, nc):
    patterns, ne = case
    sd, x = _fix(v, nc)
    off = {"YMS_BN_FROZEN": 0}
    one32, fb32 = F.gpu_step(v, nc, sd, x, F32, patterns, ne), F.gpu_step(v, nc, sd, x, F32, patterns, ne, env=off)
    assert one32["plan"].opts.bn_frozen and not fb32["plan"].opts.bn_frozen
    g1, g0 = _grads(one32), _grads(fb32)
    worst = max((_rel(g1[k], g0[k]), k) for k in g0)
    assert set(g1) == set(g0) and worst[0] <= 2e-5, worst
    for a, b in zip(one32["maps"], fb32["maps"]):
        assert torch.equal(a, b)                              # the forward is the same route
    b1 = _grads(F.gpu_step(v, nc, sd, x, BF16, patterns, ne))
    b0 = _grads(F.gpu_step(v, nc, sd, x, BF16, patterns, ne, env=off))
    d1 = torch.tensor([((b1[k] - g0[k]).norm() / (g0[k].norm() + 1e-30)).item() for k in g0])
    d0 = torch.tensor([((b0[k] - g0[k]).norm() / (g0[k].norm() + 1e-30)).item() for k in g0])
    print(f"bf16 drift from fp32: one-pass median {d1.median():.3g} max {d1.max():.3g}; "
          f"three-pass median {d0.median():.3g} max {d0.max():.3g}")
    assert d1.median() <= 1.2 * d0.median() and d1.max() <= 1.5 * d0.max(), (d1.median(), d0.median(), d1.max(), d0.max())


@pytest.mark.parametrize("case", [(("backbone",), True), ((), "all")], ids=_id)
def test_no_result_depends_on_unwritten_memory(case):
    """["backbone"] + norm_eval (and every BN in eval mode, whose stem keeps its z route) in the manner of tests/test_arena_poison_gpu.py: some z buffers and backward
    writes are gone, and the stem reads coefficients it folds itself beside the side stream's packs, so every byte torch.empty hands the plan is poisoned (0xFF: NaN in every format) and
    every collected tensor must equal the zero-filled run's, bit for bit."""
    sd, x = _fix("n", 3)
    runs = []
    for byte in (0x00, 0xFF):
        proxy = _TorchProxy(byte)
        with pytest.MonkeyPatch.context() as mp:
            for mod in PATCHED:
                mp.setattr(mod, "torch", proxy)
            runs.append(F.gpu_step("n", 3, sd, x, BF16, *case, steps=2))
        assert proxy.fills >= 6
    a, b = runs
    for k in ("maps",):
        assert all(torch.equal(s, t) for s, t in zip(a[k], b[k]))
    for k, g in a["grads"].items():
        assert (g is None) == (b["grads"][k] is None) and (g is None or torch.equal(g, b["grads"][k])), k
        assert g is None or torch.isfinite(g).all(), k
    assert all(torch.equal(t, b["after"][k]) for k, t in a["after"].items())


def test_two_optimizer_steps_leave_the_frozen_part_alone():
    """yms.optim.SGD over the trainable parameters only: frozen parameters and eval-mode buffers are
    bit-unchanged after two steps, and the trainable parameters are those of the run without the skip
    (same routes: norm_eval off, so no layer changes its forward)."""
    sd, x = _fix("n", 3)

    def opt(ps):
        return yms.optim.SGD(ps, lr=0.01, momentum=0.9)

    r = F.gpu_step("n", 3, sd, x, BF16, ("backbone",), True, steps=2, opt=opt)
    frozen = set(F.frozen_names(sd, ("backbone",)))
    for k, t in r["params"].items():
        assert torch.equal(t.cpu(), sd[k]) == (k in frozen or k == "head.dfl.conv.weight"), k
    for k, t in r["after"].items():
        if k.startswith("backbone."):
            assert torch.equal(t, r["before"][k]), k
        elif k.endswith("num_batches_tracked"):
            assert int(t) == 2, k
    on = F.gpu_step("n", 3, sd, x, BF16, ("backbone",), False, steps=2, opt=opt)
    off = F.gpu_step("n", 3, sd, x, BF16, ("backbone",), False, steps=2, opt=opt, env={"YMS_BWD_SKIP": 0})
    assert any(not op.runs_bwd for op in on["plan"].ops) and all(op.runs_bwd for op in off["plan"].ops)
    for k, t in on["params"].items():
        assert torch.equal(t, off["params"][k]), k
    for k, t in on["after"].items():
        assert torch.equal(t, off["after"][k]), k


def test_unservable_layer_raises_at_plan_build_by_name():
    sd, x = _fix("n", 3)
    m = YOLOv8("n", 3).cuda()
    m.load_state_dict(sd)
    m.train()
    bn = m.neck.conv1.bn
    bn.running_mean = bn.running_var = None
    bn.eval()
    with pytest.raises(RuntimeError, match=r"neck\.conv1\.bn is in eval mode without running statistics"):
        m(x.cuda())
