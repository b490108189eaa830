"""CPU tier for fine-tuning (plans built on meta tensors, no GPU): yms.finetune's freeze / norm_eval /
unfreeze, which ops of a plan run a backward and which buffers need a gradient under a freeze pattern,
the plan-cache key, the unchanged default plan, and the routes of eval-mode BatchNorm layers."""
import pytest
import torch

from yms import _lib as L
from yms import finetune, runner
from yms.plan import BNConvBase, HeadGroup, Rt, SiblingConvOp, View
from yolov8.yolov8 import YOLOv8

MODELS = [("n", 3), ("ms-s", 80)]
PATTERNS = [[], ["backbone"], ["backbone", "neck"], ["neck.conv1"], ["head.cls"]]


def _x():
    return torch.empty(2, 3, 64, 64, device="meta")


def _plan(m, dt=torch.bfloat16):
    return runner.get_plan(m, [_x()], dt, True)


def _bns(m):
    return {n: b for n, b in m.named_modules() if isinstance(b, torch.nn.BatchNorm2d)}


@pytest.mark.parametrize("v,nc", MODELS)
@pytest.mark.parametrize("patterns", PATTERNS[1:] + [["conv1", "head.box.2"]])
def test_freeze_matches_the_reference_rule(v, nc, patterns):
    m = YOLOv8(v, nc).train()
    fixed = [n for n, p in m.named_parameters() if not p.requires_grad]
    assert fixed == ["head.dfl.conv.weight"]
    want = [n for n, _ in m.named_parameters() if any(p in n for p in patterns)]
    assert want and finetune.freeze(m, patterns, norm_eval=False) == want
    assert {n for n, p in m.named_parameters() if not p.requires_grad} == set(want + fixed)
    assert all(b.training for b in _bns(m).values())           # norm_eval=False leaves the modes alone


def test_norm_eval_set_survives_train_and_unfreeze_restores():
    m = YOLOv8("n", 3).train()
    finetune.freeze(m, ["backbone"])
    bns = _bns(m)
    kept = {n for n in bns if n.startswith("backbone.")}
    assert kept and {n for n, b in bns.items() if not b.training} == kept

    def modes():
        return {n for n, b in bns.items() if not b.training}

    assert modes() == kept and m.train() is m and modes() == kept and m.training
    m.eval()
    assert modes() == set(bns) and not m.training
    m.train()
    assert modes() == kept
    # norm_eval adds modules without freezing anything
    frozen = [n for n, p in m.named_parameters() if not p.requires_grad]
    hit = finetune.norm_eval(m, ["neck.conv1"])
    assert hit == ["neck.conv1.bn"] and modes() == kept | {"neck.conv1.bn"}
    assert [n for n, p in m.named_parameters() if not p.requires_grad] == frozen
    m.train()
    assert modes() == kept | {"neck.conv1.bn"}
    finetune.unfreeze(m)
    assert not modes() and [n for n, p in m.named_parameters() if not p.requires_grad] == ["head.dfl.conv.weight"]
    m.eval()
    m.train()
    assert not modes()
    # a model nothing was recorded on: train() is nn.Module.train()
    m2 = YOLOv8("n", 3)
    assert m2.train() is m2 and all(b.training for b in _bns(m2).values())
    assert finetune.norm_eval(m2) == list(_bns(m2))             # None: every BN module


def _outs(op):
    y = getattr(op, "y", None)
    return [y] if isinstance(y, View) else [getattr(op, "v")]


def _ins(op):
    vs = []
    for k, val in vars(op).items():
        if k not in ("y", "members"):
            vs += [u for u in (val if isinstance(val, (list, tuple)) else (val,)) if isinstance(u, View)]
    return vs


def _overlap(a, b):
    return a.buf is b.buf and a.off < b.off + b.c and b.off < a.off + a.c


def _expected_runs(plan):
    """The rule, restated on channel slices: an op needs a backward iff it, or an op whose output it reads
    (transitively), has a parameter that requires a gradient."""
    params = plan.params()
    runs = []
    for i, op in enumerate(plan.ops):
        own = any(params[pi].requires_grad for pi in op.grad_params())
        up = any(runs[j] for j in range(i) for a in _ins(op) for o in _outs(plan.ops[j]) if _overlap(a, o))
        runs.append(own or up)
    return runs


@pytest.mark.parametrize("v,nc", MODELS)
@pytest.mark.parametrize("patterns", PATTERNS)
def test_which_ops_run_a_backward(v, nc, patterns):
    m = YOLOv8(v, nc).train()
    finetune.freeze(m, patterns, norm_eval=False)
    p = _plan(m)
    want = _expected_runs(p)
    assert [op.runs_bwd for op in p.ops] == want
    names = {id(mod): n for n, mod in m.named_modules()}
    if not patterns or patterns in (["neck.conv1"], ["head.cls"]):
        assert all(want)                    # a frozen layer in the middle: everything upstream still runs
    if patterns[:1] == ["backbone"]:
        for op, r in zip(p.ops, want):
            bb = [names[id(mod)].startswith("backbone") for mod in op.bn_modules()]
            assert not (any(bb) and r)
        assert 0 < sum(want) < len(want)
    # buffers: a gradient is needed iff the producer of any slot runs (the input of the model: never here)
    for bf in p.bufs:
        prod = [r for op, r in zip(p.ops, want) for o in _outs(op) if o.buf is bf and hasattr(op, "y")]
        assert bf.needs_grad == any(prod), bf.idx
    # the walk the runner takes: only steps with something to run, in reverse
    steps = [s for s in reversed(p.sched) if any(op.runs_bwd for op in getattr(s, "ops", (s,)))]
    assert p.bwd_sched == steps


@pytest.mark.parametrize("v,nc", MODELS)
def test_first_trainable_consumers_take_no_input_gradient(v, nc):
    """Backbone frozen: the neck's first consumers of backbone-only buffers run (weight gradient) but
    launch no input gradient, and nothing in the backward names a backbone layer's memory."""
    m = YOLOv8(v, nc).train()
    finetune.freeze(m, ["backbone"], norm_eval=False)
    p = _plan(m)
    edge = [op for op in p.ops if op.runs_bwd and hasattr(op, "x") and not op.x.buf.needs_grad]
    assert edge and all(any(p.params()[pi].requires_grad for pi in op.grad_params()) for op in edge)
    calls = []
    rt = Rt(p, 1 << 40, None, True)
    rt.gbase, rt.prepacked = 1 << 41, True
    ptrs = {i: (1 << 43) + 4096 * i for i, prm in enumerate(p.params()) if prm.requires_grad}
    rt.pgrad = ptrs.get
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(L, "call", lambda name, *a: calls.append((name, a)))
        for op in edge:
            calls.clear()
            op.bwd(rt)
            kinds = {n for n, _ in calls}
            assert any("wgrad" in n for n in kinds) and not any("dgrad" in n for n in kinds), kinds
        calls.clear()
        for s in p.bwd_sched:
            s.bwd(rt)
    n_bwd = len(calls)
    # the same model unfrozen launches more
    finetune.unfreeze(m)
    q = _plan(m)
    assert q is not p and len(q.bwd_sched) == len(q.sched) > len(p.bwd_sched)
    assert n_bwd > 0


def test_cache_key_separates_freeze_and_bn_mode_patterns():
    m = YOLOv8("n", 3).train()
    p0 = _plan(m)
    assert _plan(m) is p0
    finetune.freeze(m, ["backbone"], norm_eval=False)
    p1 = _plan(m)
    assert p1 is not p0 and _plan(m) is p1
    m.backbone.conv1.bn.eval()                   # by hand: no helper, no version to bump
    p2 = _plan(m)
    assert p2 is not p1 and _plan(m) is p2 and sum(op.bn_eval for op in p2.ops) == 1
    m.backbone.conv1.bn.train()
    assert _plan(m) is p1
    m.head.cls[0][0].conv.weight.requires_grad = False         # the reference's freeze_layers does just this
    assert _plan(m) not in (p0, p1, p2)
    m.head.cls[0][0].conv.weight.requires_grad = True
    finetune.unfreeze(m)
    assert _plan(m) is p0
    # an eval plan has no such state in its key
    m.eval()
    e = runner.get_plan(m, [_x()], torch.bfloat16, False)
    finetune.freeze(m, ["neck"])
    assert runner.get_plan(m, [_x()], torch.bfloat16, False) is e


def _summary(p):
    return ([type(s).__name__ for s in p.sched], [type(s).__name__ for s in p.bwd_sched], p.arena_bytes, p.garena_bytes,
            p.eval_bytes, p.scratch_req, p.scratch, p.gscratch, p.zero_ranges, p.gzero_ranges, p.pgrad_order,
            [(b.off, b.needs_grad) for b in p.bufs],
            [(getattr(op, "z", None), getattr(op, "acc_x", None), getattr(op, "acc_res", None),
              getattr(op, "bnred_key", None)) for op in p.ops])


@pytest.mark.parametrize("v,nc", MODELS)
def test_default_plan_is_the_plan_without_the_skip(v, nc, monkeypatch):
    m = YOLOv8(v, nc).train()
    p = _plan(m)
    monkeypatch.setenv("YMS_BWD_SKIP", "0")
    q = _plan(m)
    assert q is not p and not q.opts.bwd_skip and p.opts.bwd_skip
    assert _summary(p) == _summary(q)
    assert all(op.runs_bwd and not op.bn_eval and not op.infer for op in p.ops)
    assert "zcoef" not in p.gscratch
    monkeypatch.setenv("YMS_BN_FROZEN", "0")
    assert not runner.get_plan(m, [_x()], torch.bfloat16, True).opts.bn_frozen


@pytest.mark.parametrize("v,nc", MODELS)
def test_eval_bn_in_the_frozen_prefix_has_no_z_and_no_statistics(v, nc):
    m = YOLOv8(v, nc).train()
    base = _plan(m)
    finetune.freeze(m, ["backbone"])
    p = _plan(m)
    prefix = [op for op in p.ops if op.infer]
    assert prefix and all(isinstance(op, BNConvBase) and op.bn_eval and not op.runs_bwd and op.z is None
                          and not op.z_padding(p.es) for op in prefix)
    assert {n.split(".")[0] for op in prefix for mod in op.bn_modules() for n, q in m.named_modules() if q is mod} == {"backbone"}
    assert p.arena_bytes < base.arena_bytes
    rest = [op for op in p.ops if isinstance(op, BNConvBase) and not op.infer]
    assert rest and all(op.z is not None and not op.bn_eval for op in rest)
    # every BN module in eval mode, nothing frozen: z stays (the backward needs it), no statistics scratch,
    # a zeroed coefficient table and one arrival counter per layer for the running-statistics backward
    finetune.unfreeze(m)
    finetune.norm_eval(m)
    q = _plan(m)
    bn = [op for op in q.ops if isinstance(op, BNConvBase)]
    assert all(op.bn_eval and op.runs_bwd and not op.infer and op.z is not None for op in bn)
    assert not q.scratch_req.get("stats") and q.scratch_req["zcoef"] == 8 * max(op.c for op in bn)
    zc = (q.gscratch["zcoef"], q.scratch_req["zcoef"])
    assert zc in q.gzero_ranges and len({op.fz_cnt for op in bn}) == len(bn)
    assert not any(getattr(op, "bnred_by", None) is not None for op in q.ops)      # no pairing with an eval-mode producer
    # the running buffers' counters: only train-mode modules are bumped
    nbt = {n: int(b.num_batches_tracked) for n, b in _bns(m).items()}
    runner._bump_bn_counters(q)
    assert {n: int(b.num_batches_tracked) for n, b in _bns(m).items()} == nbt
    runner._bump_bn_counters(base)
    assert all(int(b.num_batches_tracked) == nbt[n] + 1 for n, b in _bns(m).items())


def test_eval_bn_backward_route_by_shape():
    """An eval-mode BN layer's backward: one launch of yms_bn_frozen_act_bwd, except where dgamma / dbeta are
    wanted and the last block's table sum outweighs the saved re-read (profiles/bn_frozen_bwd_micro.txt: the five
    measured layer shapes, (25600, 256) the one on the three-pass side); the stem and the sibling pairs always
    take the three passes, and YMS_BN_FROZEN=0 sends everything there."""
    from yms.plan import ConvOp

    class _Shape:
        one_pass = BNConvBase.one_pass

        def __init__(self, npix, c):
            self.npix, self.c, self.bwd_rows = npix, c, L.lib().yms_bn_bwd_rows(npix, c)

    for npix, c, with_sums in [(409600, 64, True), (102400, 128, True), (25600, 256, False), (409600, 320, True),
                               (25600, 80, True)]:
        s = _Shape(npix, c)
        assert s.one_pass(False) and s.one_pass(True) == with_sums, (npix, c)
    # on a plan: count the launches of one backward walk under both settings of the switch
    m = YOLOv8("s", 80).train()
    finetune.norm_eval(m)
    x = torch.empty(64, 3, 640, 640, device="meta")

    def launches(frozen_params):
        p = runner.get_plan(m, [x], torch.bfloat16, True)
        ptrs, off = {}, 0
        for i in p.pgrad_order:
            if p.params()[i].requires_grad:
                ptrs[i] = (1 << 43) + 4 * off
                off += p.params()[i].numel()
        rt = Rt(p, 1 << 40, None, True)
        rt.gbase, rt.prepacked = 1 << 41, True
        rt.pgrad = ptrs.get
        rt.stem_x = {i: torch.zeros(1) for i in p.stem_inputs}
        names = []
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(L, "call", lambda name, *a: names.append(name))
            for s in p.bwd_sched:
                s.bwd(rt)
        return p, names

    p, names = launches(False)
    convs = [op for op in p.ops if isinstance(op, ConvOp) and op.stem_input is None]
    slow = [op for op in convs if not op.one_pass(True)]
    assert slow and len(slow) < len(convs) and len(p.stem_inputs) == 1
    assert names.count("yms_bn_frozen_act_bwd") == len(convs) - len(slow)
    assert names.count("yms_bn_act_bwd_apply") == len(slow) + 3              # + the three sibling pairs (the stem fuses its apply)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("YMS_BN_FROZEN", "0")
        _, names0 = launches(False)
    assert "yms_bn_frozen_act_bwd" not in names0 and names0.count("yms_bn_act_bwd_apply") == len(convs) + 3
    # frozen gamma / beta: no sums, every eligible layer in one launch
    for n, q in m.named_parameters():
        if ".bn." in n:
            q.requires_grad = False
    _, names = launches(True)
    assert names.count("yms_bn_frozen_act_bwd") == len(convs)


def test_bnred_does_not_pair_across_the_boundary():
    """The consumer's input gradient computes its producer's BN-backward reduce only where both run."""
    m = YOLOv8("s", 80).train()
    p0 = _plan(m)
    pairs0 = [(op.bnred_for, op) for op in p0.ops if getattr(op, "bnred_for", None) is not None]
    assert pairs0
    finetune.freeze(m, ["backbone"], norm_eval=False)
    p = _plan(m)
    pairs = [(op.bnred_for, op) for op in p.ops if getattr(op, "bnred_for", None) is not None]
    assert len(pairs) < len(pairs0) and all(q.runs_bwd and c.runs_bwd for q, c in pairs)
    assert not any(getattr(op, "bnred_by", None) is not None for op in p.ops if not op.runs_bwd)
    # ... and not with a producer whose BatchNorm is in eval mode: that one pair goes, the others stay
    finetune.unfreeze(m)
    i = p0.ops.index(pairs0[0][0])
    pairs0[0][0].mod.bn.eval()
    pe = _plan(m)
    assert pe.ops[i].bn_eval and pe.ops[i].bnred_by is None
    assert sum(getattr(op, "bnred_for", None) is not None for op in pe.ops) == len(pairs0) - 1


def test_a_pair_in_mixed_modes_runs_unfused_and_an_unservable_layer_raises_by_name():
    m = YOLOv8("n", 80).train()
    assert sum(isinstance(op, SiblingConvOp) for op in _plan(m).ops) == 3
    m.head.cls[1][0].bn.eval()                   # one member of a pair: two ConvOps there, no group
    p = _plan(m)
    assert sum(isinstance(op, SiblingConvOp) for op in p.ops) == 2 and not p.groups and len(p.ops) == 64
    assert [op.bn_eval for op in p.ops if op.bn_modules() and op.bn_modules()[0] is m.head.cls[1][0]] == [True]
    m.head.box[1][0].bn.eval()                   # both: fused again, on the three-pass route
    p = _plan(m)
    assert [op.bn_eval for op in p.ops if isinstance(op, SiblingConvOp)] == [False, True, False] and p.groups
    # eval mode without running statistics means batch statistics in torch: not served, by name
    m.neck.conv1.bn.running_mean = None
    m.neck.conv1.bn.running_var = None
    m.neck.conv1.bn.eval()
    with pytest.raises(RuntimeError, match=r"neck\.conv1\.bn is in eval mode without running statistics"):
        _plan(m)


def test_head_group_sends_skipped_members_through_their_own_path(monkeypatch):
    monkeypatch.setenv("YMS_HEAD_GROUP", "2")
    m = YOLOv8("n", 3).train()
    p = _plan(m)
    g = [s for s in p.sched if isinstance(s, HeadGroup)][0]
    ptrs, off = {}, 0
    for i in p.pgrad_order:                      # the runner's flat gradient arena: sibling members adjacent
        ptrs[i] = 4096 + 4 * off
        off += p.params()[i].numel()
    rt = Rt(p, 0, None, True)
    rt.pgrad = ptrs.get
    assert g.bwd_grouped(rt)
    finetune.freeze(m, ["backbone", "neck", "head.box.0", "head.cls.0"], norm_eval=False)      # level 0: nothing to do
    q = _plan(m)
    gq = [s for s in q.sched if isinstance(s, HeadGroup)][0]
    assert q.bwd_sched == [gq] and not all(op.runs_bwd for op in gq.ops) and any(op.runs_bwd for op in gq.ops)
    rt = Rt(q, 0, None, True)
    rt.pgrad = ptrs.get
    assert not gq.bwd_grouped(rt)
