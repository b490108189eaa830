"""CPU tier of the AdamW / exp-momentum EMA / on-device schedule additions to yms.optim: the argument
checks of yms_optim_step_ext (no launch happens: the pointers are host dummies), the host restatement
of the schedule (yms.optim.schedule_factor, the definition the GPU tests compare the kernel with)
against torch's own schedulers, the config reader's new keys and the YOLO-MS recipe's values.

torch's LinearLR and CosineAnnealingLR are recursive (each learning rate is computed from the previous
one), schedule_factor is closed-form; over the <= 64 iterations used here the two agree to fp64
round-off, for which relative 1e-12 (4500 ulp) is a generous ceiling."""
import ctypes
import math

import pytest
import torch

from yms import _lib as L
from yms import optim as O
from yolov8.yolov8 import YOLOv8

Segment = O.Segment


def test_step_ext_argument_validation():
    """One valid yms_optim_step_ext call with one argument broken -> YMS_ERR_INVALID before any launch.
    Every kind the entry point knows passes the kind check: with a table that is still NULL the call is
    rejected for that reason alone, and a kind the entry point does not know is rejected with every other
    argument valid."""
    lib = L.lib()
    assert (L.OPTIM_ADAMW, L.OPTIM_EMA_TAU, L.OPTIM_EMA_EXPMOM, L.OPTIM_MAX_SEGMENTS) == (2, 0, 1, 8)
    assert ctypes.sizeof(L.OptimSegment) == 48 and ctypes.sizeof(L.OptimExt) == 16 + 8 * 48
    assert ctypes.sizeof(L.OptimHyper) == 8 * (4 + 8 * 8)              # the old records keep their layouts
    buf = (ctypes.c_float * 64)()
    P = ctypes.addressof(buf)
    good = dict(kind=L.OPTIM_ADAMW, table=P, nchunks=2, base=P, hyper=P, ext=P, counters=P, sched_out=P, partials=P,
                npartials=2, stream=None)
    broken = dict(kind3=dict(kind=3), kind_neg=dict(kind=-1), table=dict(table=None), nchunks0=dict(nchunks=0),
                  nchunks_neg=dict(nchunks=-1), nchunks_huge=dict(nchunks=1 << 31), hyper=dict(hyper=None),
                  counters=dict(counters=None), partials_without_count=dict(npartials=0),
                  count_without_partials=dict(partials=None), npartials_neg=dict(npartials=-1))
    for kind in (L.OPTIM_SGD, L.OPTIM_ADAM, L.OPTIM_ADAMW):
        for opt in (dict(), dict(ext=None), dict(sched_out=None), dict(ext=None, sched_out=None)):
            for label, change in broken.items():
                if "kind" in change and kind != L.OPTIM_ADAMW:
                    continue
                args = dict(good, kind=kind, **opt)
                args.update(change)
                assert lib.yms_optim_step_ext(*args.values()) == 1, (kind, opt, label)
    # too many partial sums is "unsupported", not "invalid": that check comes after the kind check, so a
    # status of 2 shows that kinds 0, 1 and 2 got past it with ext / sched_out NULL or not; 3 and -1 do not
    many = dict(good, npartials=256 * 128 + 1)
    for kind, want in ((0, 2), (1, 2), (2, 2), (3, 1), (-1, 1)):
        for opt in (dict(), dict(ext=None, sched_out=None)):
            assert lib.yms_optim_step_ext(*dict(many, kind=kind, **opt).values()) == want, (kind, opt)
    # the old entry point keeps its signature and still knows kinds 0 and 1 only
    old = dict(kind=L.OPTIM_ADAMW, table=P, nchunks=2, base=P, hyper=P, counters=P, partials=P, npartials=2, stream=None)
    assert lib.yms_optim_step(*old.values()) == 1
    assert lib.yms_optim_step(*dict(old, npartials=256 * 128 + 1).values()) == 1
    assert lib.yms_optim_step(*dict(old, kind=L.OPTIM_ADAM, npartials=256 * 128 + 1).values()) == 2


def _torch_factors(make, n):
    """lr / base of a torch scheduler for iterations 0 .. n - 1."""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=0.25)
    sch = make(opt)
    out = []
    for _ in range(n):
        out.append(opt.param_groups[0]["lr"] / 0.25)
        opt.step()
        sch.step()
    return out


def _close(a, b):
    return abs(a - b) <= 1e-12 * max(abs(a), abs(b))


@pytest.mark.parametrize("start,end", [(1e-5, 1000 // 32), (0.1, 3), (0.5, 64)])
def test_linear_segment_is_torch_linear_lr(start, end):
    want = _torch_factors(lambda o: torch.optim.lr_scheduler.LinearLR(o, start_factor=start, end_factor=1.0,
                                                                      total_iters=end), end + 6)
    segs = [Segment(0, end, start, 1.0)]
    for n in range(end + 6):
        got = O.schedule_factor(segs, n)
        assert _close(got, want[n]), (n, got, want[n])
    assert O.schedule_factor(segs, 0) == start and O.schedule_factor(segs, end) == 1.0 == O.schedule_factor(segs, end + 5)


@pytest.mark.parametrize("ratio,end", [(0.05, 64), (0.0, 7), (0.5, 1)])
def test_cosine_segment_is_torch_cosine_annealing(ratio, end):
    want = _torch_factors(lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=end, eta_min=0.25 * ratio),
                          end + 1)
    segs = [Segment(0, end, 1.0, ratio, shape="cosine")]
    for n in range(end + 1):
        got = O.schedule_factor(segs, n)
        assert _close(got, want[n]) or abs(got - want[n]) <= 1e-15, (n, got, want[n])    # (ratio 0: the last is 0 vs 1e-17)
    # past its end a segment holds its value (torch's scheduler would start the next half wave)
    assert all(O.schedule_factor(segs, n) == ratio for n in (end, end + 1, end + 5, 10 ** 9))
    assert O.schedule_factor(segs, -3) == 1.0


def test_warmup_flat_cosine_masks_and_targets():
    warm, lo, hi, ratio = 8, 20, 40, 0.05
    segs = [Segment(0, warm, 1e-5, 1.0), Segment(lo, hi, 1.0, ratio, shape="cosine")]
    lin = _torch_factors(lambda o: torch.optim.lr_scheduler.LinearLR(o, start_factor=1e-5, total_iters=warm), warm + 1)
    cos = _torch_factors(lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=hi - lo, eta_min=0.25 * ratio),
                         hi - lo + 1)
    for n in range(hi + 6):
        want = lin[n] if n <= warm else 1.0 if n <= lo else cos[n - lo] if n <= hi else ratio
        assert _close(O.schedule_factor(segs, n), want), n
    assert O.schedule_factor(segs, warm) == 1.0 == O.schedule_factor(segs, lo) and O.schedule_factor(segs, hi + 5) == ratio
    # masks, the momentum target, products, and what is ignored
    segs = [Segment(0, 4, 0.1, 1.0), Segment(4, 8, 1.0, 0.5, shape="cosine", groups=[1]),
            Segment(0, 5, 0.8 / 0.937, 1.0, target="momentum"), Segment(3, 3, 7.0, 9.0), Segment(9, 2, 7.0, 9.0),
            Segment(0, 4, 2.0, 2.0, groups=(0, 1))]
    f = O.schedule_factor
    assert f(segs, 2, 0) == pytest.approx(0.55 * 2.0, rel=1e-15) and f(segs, 2, 1) == f(segs, 2, 0)
    assert f(segs, 6, 0) == 2.0 and f(segs, 6, 1) == pytest.approx(0.75 * 2.0, rel=1e-15)
    assert f(segs, 6, 2) == 1.0                                   # group 2 is in neither masked segment
    assert f(segs, 100, 0) == 2.0 and f(segs, 100, 1) == 1.0
    assert f(segs, 0, 0, target="momentum") == 0.8 / 0.937 and f(segs, 5, 1, target="momentum") == 1.0
    assert f(segs, 2, 0, target="momentum") == pytest.approx(0.8 / 0.937 + (1 - 0.8 / 0.937) * 0.4, rel=1e-15)
    assert f(None, 3) == 1.0 and f([], 3) == 1.0
    assert f([(0, 4, 0.0, 1.0)], 1) == 0.25                       # plain tuples are segments too
    for bad in (Segment(0, 4, 0.1, 1.0, target="beta2"), Segment(0, 4, 0.1, 1.0, shape="step"),
                Segment(0, 4, 0.1, 1.0, groups=[8])):
        with pytest.raises(ValueError, match="segment"):
            f([bad], 1)


def _cfg(**training):
    return {"training": dict({"learning_rate": 0.002, "weight_decay": 5e-4}, **training)}


def test_optimizer_config_reads_adamw_the_ema_rule_and_the_schedule():
    m = YOLOv8("n", 3)
    cls, groups, kw, ema = O.optimizer_config(m, _cfg(optimizer="AdamW"))
    assert cls is O.AdamW and ema is None
    assert kw == dict(lr=0.002, betas=(0.9, 0.999), weight_decay=5e-4, clip_grad_norm=None, skip_nonfinite=False)
    assert [id(p) for p in groups] == [id(p) for p in m.parameters()]
    cls, groups, kw, ema = O.optimizer_config(m, _cfg(
        optimizer="adamw", adam_betas=[0.8, 0.99], no_decay_bn_bias=True, ema={"rule": "exp_momentum", "gamma": 500},
        lr_schedule=dict(warmup_iters=1000, warmup_start_factor=1e-5, cosine_begin_iter=4000, cosine_end_iter=8000,
                         min_lr_ratio=0.05)))
    assert cls is O.AdamW and kw["betas"] == (0.8, 0.99) and len(groups) == 2 and groups[1]["weight_decay"] == 0.0
    assert ema == {"rule": "exp_momentum", "momentum": 0.0002, "gamma": 500}
    assert kw["schedule"] == [Segment(0, 1000, 1e-5, 1.0, "lr", "linear", None),
                              Segment(4000, 8000, 1.0, 0.05, "lr", "cosine", None)]
    _, _, kw, ema = O.optimizer_config(m, _cfg(optimizer="sgd", ema={"rule": "tau", "tau": 500},
                                               lr_schedule=dict(warmup_iters=100)))
    assert ema == {"decay": 0.9999, "tau": 500} and kw["schedule"] == [Segment(0, 100, 1e-3, 1.0)]
    # without the new keys nothing new is returned
    _, _, kw, ema = O.optimizer_config(m, _cfg(optimizer="adam", ema=True))
    assert "schedule" not in kw and ema == {"decay": 0.9999, "tau": 2000}
    with pytest.raises(ValueError, match="Unsupported EMA rule: sma"):
        O.optimizer_config(m, _cfg(optimizer="adam", ema={"rule": "sma"}))
    for fn in (O.optimizer_config, O.build_optimizer):
        with pytest.raises(ValueError, match="Unsupported optimizer: lion"):
            fn(m, _cfg(optimizer="Lion"))


def test_adamw_constructor_refusals():
    p = [torch.nn.Parameter(torch.zeros(4))]
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(foreach=True), dict(fused=True), dict(capturable=True),
               dict(differentiable=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            O.AdamW(p, **kw)
    with pytest.raises(ValueError, match="ROCm"):
        O.AdamW(p)                            # CPU parameters: there is no CPU path
    with pytest.raises(ValueError, match="yms.optim.AdamW: invalid"):
        O.AdamW(p, weight_decay=-1.0)


def test_yolo_ms_recipe_values(monkeypatch):
    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv2d(3, 8, 3, bias=True)
            self.bn = torch.nn.BatchNorm2d(8)
            self.gn = torch.nn.GroupNorm(2, 8)
            self.fc = torch.nn.Linear(8, 4, bias=False)

    with torch.device("meta"):
        net = Net()
    cls, groups, kw, ema = O.yolo_ms_recipe_config(net, iters_per_epoch=100, epochs=300, batch_size=64)
    assert cls is O.AdamW and kw["lr"] == 0.001 and kw["weight_decay"] == 0.05 and kw["betas"] == (0.9, 0.999)
    assert ema == {"rule": "exp_momentum", "momentum": 0.0002, "gamma": 2000}
    assert [id(p) for p in groups[0]["params"]] == [id(net.conv.weight), id(net.fc.weight)] and "weight_decay" not in groups[0]
    assert [id(p) for p in groups[1]["params"]] == [id(p) for p in (net.conv.bias, net.bn.weight, net.bn.bias,
                                                                    net.gn.weight, net.gn.bias)]
    assert groups[1]["weight_decay"] == 0.0
    segs = kw["schedule"]
    assert segs == [Segment(0, 1000, 1e-5, 1.0, "lr", "linear", None), Segment(15000, 30000, 1.0, 0.05, "lr", "cosine", None)]
    lr = lambda n: kw["lr"] * O.schedule_factor(segs, n)
    assert lr(0) == 0.001 * 1e-5 and lr(1000) == 0.001 == lr(15000) and lr(30000) == 0.001 * 0.05 == lr(40000)
    assert lr(500) == pytest.approx(0.001 * (1e-5 + (1 - 1e-5) * 0.5), rel=1e-14)
    assert lr(22500) == pytest.approx(0.001 * (0.05 + 0.95 * 0.5), rel=1e-14)
    assert O.yolo_ms_recipe_config(net, 10, epochs=7)[2]["schedule"][1][:2] == (30, 70)
    assert O.yolo_ms_recipe_config(net, 10)[2]["lr"] == 0.004
    assert "UNPINNED" in O.yolo_ms_recipe.__doc__
    # the builder hands exactly this to the class and attaches the EMA (a stub stands in: no kernel call)
    made = []

    class Stub:
        def __init__(self, groups, **kw):
            made.append((groups, kw))

        def attach_ema(self, model, **kw):
            made.append((model, kw))

    monkeypatch.setattr(O, "AdamW", Stub)
    opt = O.yolo_ms_recipe(net, 100, batch_size=64)
    assert isinstance(opt, Stub) and made[0][1] == kw and made[1] == (net, ema)
    assert [[id(p) for p in g["params"]] for g in made[0][0]] == [[id(p) for p in g["params"]] for g in groups]
