"""GPU tier of the AdamW / exp-momentum EMA / on-device schedule additions to yms.optim (csrc/optim.hip,
yms_optim_step_ext): single AdamW steps, per-group decay under clipping, the second EMA rule, the
schedule across its edges, through a skipped step and inside a captured graph, resume, state-dict
interchange with torch.optim.AdamW, and the old entry point's paths.

The method, the inputs (SHAPES: 1, 3, chunk - 1 / + 0 / + 1, three chunks + 5, 4-D, odd gradient offsets,
one unaligned parameter, one frozen) and the helpers are test_optim_gpu's.  u = 2^-24; "fp64
restatement" = the formulas of include/yms.h written below in torch.float64 on the CPU.  Every bound
is on ABSOLUTE-value magnitudes, counts the roundings of the fp32 evaluation and was fixed before any run:

  AdamW  moments as Adam's with d = |g|: 4u(|m| + |g|), 16u(b2 v + (1 - b2) g^2); parameter
         16u(|p| + upd), upd = lr wd |p| + lr / (bc1 den) (b1 |m| + (1 - b1)|g|) (the decay multiply adds two
         roundings of size u|p|); twice each against torch.optim.AdamW.  torch.optim.AdamW itself, in fp32 on
         the CPU, sits within half of each on all 18 (t, wd, gscale) cases (largest ratios: parameter 0.200,
         exp_avg 0.239, exp_avg_sq 0.170), and for wd = 0.05 the Adam (L2) restatement lies outside the
         parameter bound in every live tensor (by at least 140x), so the test tells the two apart.
  clip   the fp32 norm is within 1e-5 of the fp64 one (asserted), which moves g by that fraction:
         + 1e-5 (1 - b1)|g| on m, + 2.1e-5 (1 - b2) g^2 on v, + 2e-5 upd on p (m and den both move).
  EMA    4u(|e| + |p'|): the three roundings of the lerp plus the cast of mu.
  sched  the scheduled arm against the same class driven from the host: the same fp32 evaluation from
         coefficients that differ by an fp64 rounding (the device's cos and fused multiply-adds) before the
         cast to float, so the per-step single-arm bounds from the host arm's pre-step state hold;
         opt.scheduled against the host formula to relative 1e-12.
Where both arms evaluate on the device (capture, resume, the old paths) the bar is bit-equality.
On an MI355X the kernels reached 0.52 of the EMA bound and at most 0.48 of any other (each test
prints its ratios)."""
import copy
import math

import pytest
import torch

import test_optim_gpu as T
from yms import _lib as L
from yms import optim as O

pytestmark = pytest.mark.gpu

U, B1, B2, EPS, LRS, MOM = T.U, T.B1, T.B2, T.EPS, T.LRS, T.MOM
LIVE, FROZEN, SPLIT = T.LIVE, T.FROZEN, T.SPLIT
N = len(T.SHAPES)
WD = 0.05
Segment = O.Segment


# ---- fp64 restatements --------------------------------------------------------------------------
def adamw64(p, g, m, v, lr, wd, t, coef=1.0, b1=B1, decay_coef=1.0):
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    d = g * coef
    p1 = p * (1.0 - lr * wd * decay_coef)
    m2 = b1 * m + (1 - b1) * d
    v2 = B2 * v + (1 - B2) * d * d
    bc1, bc2 = 1 - b1 ** t, 1 - B2 ** t
    den = v2.sqrt() / math.sqrt(bc2) + EPS
    return p1 - (lr / bc1) * m2 / den, m2, v2, den, bc1


def adamw_bounds(p, g, m, v, lr, wd, t, b1=B1):
    _, _, _, den, bc1 = adamw64(p, g, m, v, lr, wd, t, b1=b1)
    p, g, m, v = p.double().abs(), g.double().abs(), m.double().abs(), v.double()
    upd = lr * wd * p + lr / (bc1 * den) * (b1 * m + (1 - b1) * g)
    return 16 * U * (p + upd), 4 * U * (m + g), 16 * U * (B2 * v + (1 - B2) * g * g), upd


def _outside(other, want, bound):
    """Does the restatement `other` differ from `want` by more than the bound somewhere?"""
    return bool(((other - want).abs() > bound).any())


def _adam_state(m0, v0, t):
    return {i: {"step": torch.tensor(float(t - 1)), "exp_avg": m0[i], "exp_avg_sq": v0[i]} for i in range(N)}


def _state(opt, params, key):
    return [opt.state[p][key] for p in params]


# ---- 1. single steps ----------------------------------------------------------------------------
@pytest.mark.parametrize("gscale", [1e-4, 1.0, 50.0])
@pytest.mark.parametrize("wd", [0.0, WD])
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_adamw_single_step(t, wd, gscale):
    p0, g0, m0, v0 = T._data(gscale)
    if t == 1:                           # torch's state before its first step
        m0, v0 = [torch.zeros_like(x) for x in m0], [torch.zeros_like(x) for x in v0]
    params = T._params(p0)
    T._set_grads(params, g0)
    opt = O.AdamW(T._groups(params), lr=LRS[0], betas=(B1, B2), eps=EPS, weight_decay=wd)
    T._load_state(opt, _adam_state(m0, v0, t))
    opt.step()
    assert opt.last_launches == 2
    tp = [torch.nn.Parameter(x.cuda()) for x in p0]
    topt = torch.optim.AdamW(T._groups(tp), lr=LRS[0], betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
    for i in LIVE:
        tp[i].grad = g0[i].cuda()
        topt.state[tp[i]].update(step=torch.tensor(float(t - 1)), exp_avg=m0[i].cuda(), exp_avg_sq=v0[i].cuda())
    topt.step()
    for i in LIVE:
        a = (p0[i], g0[i], m0[i], v0[i], T._lr(i), wd, t)
        p64, m64, v64, _, _ = adamw64(*a)
        bp, bm, bv, _ = adamw_bounds(*a)
        st, ts = opt.state[params[i]], topt.state[tp[i]]
        T._within(params[i], p64, bp, f"p[{i}]")
        T._within(st["exp_avg"], m64, bm, f"m[{i}]")
        T._within(st["exp_avg_sq"], v64, bv, f"v[{i}]")
        T._within(params[i], tp[i].detach().double().cpu(), 2 * bp, f"p[{i}] vs torch")
        T._within(st["exp_avg"], ts["exp_avg"].double().cpu(), 2 * bm, f"m[{i}] vs torch")
        T._within(st["exp_avg_sq"], ts["exp_avg_sq"].double().cpu(), 2 * bv, f"v[{i}] vs torch")
        if wd:                           # Adam's L2 decay is a different result, by more than the bound
            assert _outside(T.adam64(*a)[0], p64, bp), i
    assert torch.equal(params[FROZEN].detach().cpu(), p0[FROZEN])
    assert torch.equal(opt.state[params[FROZEN]]["exp_avg"].cpu(), m0[FROZEN])
    assert torch.equal(opt.state[params[FROZEN]]["exp_avg_sq"].cpu(), v0[FROZEN])
    assert float(opt.state_dict()["state"][0]["step"]) == t
    assert opt.state_dict()["param_groups"][0]["decoupled_weight_decay"] is True


# ---- 2. per-group decay, clipping ----------------------------------------------------------------
def test_adamw_decay_is_per_group_and_never_clipped():
    t = 5
    p0, g0, m0, v0 = T._data()
    norm = T._norm64(g0)
    params = T._params(p0)
    T._set_grads(params, g0)
    opt = O.AdamW(T._groups(params, weight_decay=0.0), lr=LRS[0], betas=(B1, B2), eps=EPS, weight_decay=WD,
                  clip_grad_norm=0.5 * norm)
    T._load_state(opt, _adam_state(m0, v0, t))
    opt.step()
    assert opt.last_launches == 3
    got = opt.grad_norm.item()
    assert abs(got - norm) <= 1e-5 * norm
    coef = 0.5 * norm / (norm + 1e-6)
    for i in LIVE:
        wd = WD if i < SPLIT else 0.0
        a = (p0[i], g0[i], m0[i], v0[i], T._lr(i), wd, t)
        p64, m64, v64, _, _ = adamw64(*a, coef=coef)
        bp, bm, bv, upd = adamw_bounds(*a)
        g = g0[i].double().abs()
        bp = bp + 2e-5 * upd
        st = opt.state[params[i]]
        T._within(params[i], p64, bp, f"clipped p[{i}] wd={wd}")
        T._within(st["exp_avg"], m64, bm + 1e-5 * (1 - B1) * g, f"clipped m[{i}]")
        T._within(st["exp_avg_sq"], v64, bv + 2.1e-5 * (1 - B2) * g * g, f"clipped v[{i}]")
        # what the test can tell apart: the other group's decay, a decay scaled by the clip factor, no clipping
        other = adamw64(p0[i], g0[i], m0[i], v0[i], T._lr(i), WD - wd, t, coef=coef)[0]
        assert _outside(other, p64, bp), i
        assert _outside(adamw64(*a)[0], p64, bp), i
        if wd:
            assert _outside(adamw64(*a, coef=coef, decay_coef=coef)[0], p64, bp), i


# ---- 3. the exp-momentum EMA ----------------------------------------------------------------------
def _ema_run(k, **ema_kw):
    """One SGD step with the EMA at update count k and EMA values distinct from the weights.
    -> (toy, optimizer, EMA before, EMA after)"""
    p0, g0, _, _ = T._data()
    params = T._params(p0)
    T._set_grads(params, g0)
    toy = T.Toy(params)
    opt = O.SGD(T._groups(params), lr=LRS[0], momentum=MOM, nesterov=True, weight_decay=5e-4)
    opt.attach_ema(toy, **ema_kw)
    sd = opt.state_dict()
    sd["yms"]["ema_step"] = k
    sd["yms"]["ema"] = {name: v * 0.75 + 0.125 for name, v in sd["yms"]["ema"].items()}
    opt.load_state_dict(sd)
    before = opt.ema_state_dict()
    toy.stat.add_(0.5)                   # the forward writes the BN statistics
    opt.step()
    assert opt.last_launches == 2
    return toy, opt, before, opt.ema_state_dict()


@pytest.mark.parametrize("gamma", [2000.0, 1.0])
@pytest.mark.parametrize("k", [0, 1, 2000, 10 ** 6])
def test_exp_momentum_ema(k, gamma):
    m = 0.0002
    toy, opt, e, e2 = _ema_run(k, rule="exp_momentum", momentum=m, gamma=gamma)
    sd = opt.state_dict()["yms"]
    assert (sd["ema_rule"], sd["ema_momentum"], sd["ema_gamma"], sd["ema_step"]) == ("exp_momentum", m, gamma, k + 1)
    live = toy.state_dict()
    assert list(e2) == list(live) and "stat" in e2
    mu = (1.0 - m) * math.exp(-(k + 1) / gamma) + m
    for name in e2:
        if name == "count":              # the integer buffer is the live one
            assert torch.equal(e2[name], live[name])
            continue
        old, new = e[name].double().cpu(), live[name].double().cpu()    # the kernel's own p'
        T._within(e2[name], (1.0 - mu) * old + mu * new, 4 * U * (old.abs() + new.abs()), f"ema {name} k={k}")
    # the default rule on the same inputs is another EMA: the flag is read
    _, _, _, d2 = _ema_run(k, decay=0.9999, tau=gamma)
    assert not any(torch.equal(d2[name], e2[name]) for name in e2 if name != "count")
    before = {n: v.clone() for n, v in live.items()}
    with opt.ema_applied():
        for n, v in toy.state_dict().items():
            assert torch.equal(v, e2[n]), n
    for n, v in toy.state_dict().items():
        assert torch.equal(v, before[n]), n
    for n, v in opt.ema_state_dict().items():
        assert torch.equal(v, e2[n]), n


# ---- 4. the schedule -----------------------------------------------------------------------------
SGD_SEGS = [Segment(0, 3, 0.1, 1.0), Segment(4, 7, 1.0, 0.05, shape="cosine", groups=[1]),
            Segment(0, 5, 0.8 / MOM, 1.0, target="momentum"), Segment(2, 2, 5.0, 7.0)]
SGD_KW = dict(lr=LRS[0], momentum=MOM, nesterov=True, weight_decay=5e-4)


def _host_drive(opt, segs, n, bases):
    """What a host scheduler would do before call n: base * factor into param_groups.  -> [(lr, momentum)]"""
    out = []
    for gi, (grp, (lr, mom)) in enumerate(zip(opt.param_groups, bases)):
        lr_n = lr * O.schedule_factor(segs, n, gi, "lr")
        mom_n = mom * O.schedule_factor(segs, n, gi, "momentum")
        grp["lr"] = lr_n
        if "betas" in grp:
            grp["betas"] = (mom_n, grp["betas"][1])
        else:
            grp["momentum"] = mom_n
        out.append((lr_n, mom_n))
    return out


def _check_scheduled(opt, want):
    got = opt.scheduled.cpu()
    assert got.dtype == torch.float64 and got.shape == (len(want), 2)
    for gi, row in enumerate(want):
        for j in (0, 1):
            assert abs(got[gi, j].item() - row[j]) <= 1e-12 * abs(row[j]), (gi, j, got[gi, j].item(), row[j])


def test_sgd_schedule_across_its_edges():
    p0, g0, b0, _ = T._data()
    pa, pb = T._params(p0), T._params(p0)
    T._set_grads(pa, g0)
    T._set_grads(pb, g0)
    a = O.SGD(T._groups(pa), schedule=SGD_SEGS, **SGD_KW)
    b = O.SGD(T._groups(pb), **SGD_KW)
    bases = [(LRS[0], MOM), (LRS[1], MOM)]
    seen = set()
    for n in range(10):
        pre_p, pre_b = T._cpu(pb), (T._cpu(_state(b, pb, "momentum_buffer")) if n else b0)
        hyp = _host_drive(b, SGD_SEGS, n, bases)
        seen.add(hyp[1])
        a.step()
        b.step()
        assert a.last_launches == 2 and b.last_launches == 2
        _check_scheduled(a, hyp)
        for i in LIVE:
            lr, mom = hyp[0 if i < SPLIT else 1]
            bp, bb, _ = T.sgd_bounds(pre_p[i], g0[i], pre_b[i], lr, mom, 5e-4, True, n == 0)
            T._within(pa[i], pb[i].detach().double().cpu(), bp, f"step {n} p[{i}]")
            T._within(a.state[pa[i]]["momentum_buffer"], b.state[pb[i]]["momentum_buffer"].double().cpu(), bb,
                      f"step {n} b[{i}]")
        assert torch.equal(pa[FROZEN], pb[FROZEN])
    assert len(seen) == 8                # group 1 ran at 8 different (lr, momentum): every edge was crossed
    assert [grp["lr"] for grp in a.param_groups] == list(LRS)       # param_groups keep the bases
    a.set_schedule(None)
    with pytest.raises(RuntimeError, match="no schedule"):
        a.scheduled


def test_adamw_schedule_of_lr_and_beta1():
    segs = [Segment(0, 3, 0.1, 1.0, groups=[0]), Segment(1, 4, 1.0, 0.5, shape="cosine"),
            Segment(0, 3, 0.5, 1.0, target="momentum")]
    p0, g0, m0, v0 = T._data()
    pa, pb = T._params(p0), T._params(p0)
    T._set_grads(pa, g0)
    T._set_grads(pb, g0)
    kw = dict(lr=LRS[0], betas=(B1, B2), eps=EPS, weight_decay=WD)
    a = O.AdamW(T._groups(pa), schedule=segs, **kw)
    b = O.AdamW(T._groups(pb), **kw)
    for opt in (a, b):
        T._load_state(opt, _adam_state(m0, v0, 3))
    bases = [(LRS[0], B1), (LRS[1], B1)]
    for n in range(4):
        pre = [T._cpu(x) for x in (pb, _state(b, pb, "exp_avg"), _state(b, pb, "exp_avg_sq"))]
        # the loaded state says two updates were made: the schedule index starts there, as on resume
        hyp = _host_drive(b, segs, n + 2, bases)
        a.step()
        b.step()
        _check_scheduled(a, hyp)
        for i in LIVE:
            lr, b1 = hyp[0 if i < SPLIT else 1]
            bp, bm, bv, _ = adamw_bounds(pre[0][i], g0[i], pre[1][i], pre[2][i], lr, WD, n + 3, b1=b1)
            sa, sb = a.state[pa[i]], b.state[pb[i]]
            T._within(pa[i], pb[i].detach().double().cpu(), bp, f"step {n} p[{i}]")
            T._within(sa["exp_avg"], sb["exp_avg"].double().cpu(), bm, f"step {n} m[{i}]")
            T._within(sa["exp_avg_sq"], sb["exp_avg_sq"].double().cpu(), bv, f"step {n} v[{i}]")
            if n == 0:                   # the scheduled arm follows the restatement at the scheduled beta1, not at the base
                args = (pre[0][i], g0[i], pre[1][i], pre[2][i], lr, WD, 3)
                T._within(pa[i], adamw64(*args, b1=b1)[0], bp, f"scheduled beta1 p[{i}]")
                assert b1 < 0.8 and _outside(adamw64(*args)[0], adamw64(*args, b1=b1)[0], bp), i


# ---- 5. a skipped step advances the schedule -----------------------------------------------------
def test_skipped_step_advances_the_schedule():
    segs = [Segment(0, 5, 0.1, 1.0)]
    p0, g0, _, _ = T._data()

    def new(**kw):
        params = T._params(p0)
        T._set_grads(params, g0)
        toy = T.Toy(params)
        opt = O.SGD(T._groups(params), skip_nonfinite=True, **SGD_KW, **kw)
        opt.attach_ema(toy)
        return params, opt

    snap = lambda params, opt: (T._cpu(params), T._cpu(_state(opt, params, "momentum_buffer")),
                                T._cpu(opt.ema_state_dict().values()))
    pa, a = new(schedule=segs)
    pb, b = new()                        # host-driven, counts every call
    pc, c = new()                        # host-driven, does not count the skipped call: must NOT agree
    bases = [(LRS[0], MOM), (LRS[1], MOM)]
    told = False
    for n in range(5):
        pre_p, pre_b = T._cpu(pb), T._cpu(_state(b, pb, "momentum_buffer"))
        hyp = _host_drive(b, segs, n, bases)
        _host_drive(c, segs, n - (n > 2), bases)
        if n == 2:
            s0 = snap(pa, a)
            keep = g0[5][7].item()
            for ps in (pa, pb, pc):
                ps[5].grad[7] = float("inf")
        for opt in (a, b, c):
            opt.step()
            assert opt.last_launches == 3
        _check_scheduled(a, hyp)
        if n == 2:                       # nothing was written, the call was counted as skipped
            for x, y in zip(s0, snap(pa, a)):
                for u, v in zip(x, y):
                    assert torch.equal(u, v)
            assert a.skipped_steps.item() == 1 and a.state_dict()["yms"]["step"] == 2
            for ps in (pa, pb, pc):
                ps[5].grad[7] = keep
            continue
        for i in LIVE:
            lr, mom = hyp[0 if i < SPLIT else 1]
            bp, bb, _ = T.sgd_bounds(pre_p[i], g0[i], pre_b[i], lr, mom, 5e-4, True, n == 0)
            T._within(pa[i], pb[i].detach().double().cpu(), bp, f"call {n} p[{i}]")
            T._within(a.state[pa[i]]["momentum_buffer"], b.state[pb[i]]["momentum_buffer"].double().cpu(), bb,
                      f"call {n} b[{i}]")
            if n == 3:
                told |= _outside(pc[i].detach().double().cpu(), pb[i].detach().double().cpu(), bp)
    assert told                          # factor(2) at call 3 is outside the bound: the test sees the difference
    sd = a.state_dict()["yms"]
    assert (sd["step"], sd["skipped"], sd["ema_step"]) == (4, 1, 4)


# ---- 6. graph capture -----------------------------------------------------------------------------
def test_captured_step_follows_the_schedule_without_a_host_call():
    segs = [Segment(0, 4, 0.1, 1.0), Segment(4, 10, 1.0, 0.05, shape="cosine", groups=[1]),
            Segment(0, 6, 0.5, 1.0, target="momentum")]
    p0, g0, _, _ = T._data()

    def new():
        params = T._params(p0)
        arena = T._set_grads(params, g0)
        opt = O.AdamW(T._groups(params), lr=LRS[0], weight_decay=WD, clip_grad_norm=100.0, schedule=segs)
        opt.attach_ema(T.Toy(params), rule="exp_momentum", gamma=3.0)
        return params, opt, arena

    ep, eopt, ea = new()
    sched = []
    for _ in range(7):
        eopt.step()
        sched.append(eopt.scheduled.clone())
    gp, gopt, ga = new()
    gopt.step()
    gopt.step()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gopt.step()
    assert gopt.last_launches == 3 and gopt.table_builds == 1
    with pytest.raises(RuntimeError, match="before capturing"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            gopt.step()                  # (captured, never replayed)
            gopt.set_schedule(segs[:1])  # an upload: refused during capture, and the schedule stays
    for r in range(5):
        graph.replay()
        assert torch.equal(gopt.scheduled, sched[2 + r]), r
    torch.cuda.synchronize()
    assert len({tuple(s.flatten().tolist()) for s in sched}) == 7
    for x, y in zip(ep, gp):
        assert torch.equal(x, y)
    for key in ("exp_avg", "exp_avg_sq"):
        for x, y in zip(_state(eopt, ep, key), _state(gopt, gp, key)):
            assert torch.equal(x, y)
    for x, y in zip(eopt.ema_state_dict().values(), gopt.ema_state_dict().values()):
        assert torch.equal(x, y)
    assert float(gopt.state_dict()["state"][0]["step"]) == 7


# ---- 7. resume ------------------------------------------------------------------------------------
def test_resume_with_adamw_ema_and_schedule_is_exact():
    segs = [Segment(0, 4, 0.1, 1.0), Segment(2, 6, 1.0, 0.05, shape="cosine"), Segment(0, 5, 0.5, 1.0, target="momentum")]
    p0, g0, _, _ = T._data()

    def new(values):
        params = T._params(values)
        T._set_grads(params, g0)
        toy = T.Toy(params)
        opt = O.AdamW(T._groups(params, weight_decay=0.0), lr=LRS[0], weight_decay=WD, clip_grad_norm=10.0,
                      skip_nonfinite=True, schedule=segs)
        opt.attach_ema(toy, rule="exp_momentum", momentum=0.0002, gamma=5.0)
        return params, toy, opt

    pa, ta, a = new(p0)
    for _ in range(6):
        a.step()
    pb, tb, b = new(p0)
    for _ in range(3):
        b.step()
    sd = copy.deepcopy(b.state_dict())
    pc, tc, c = new(T._cpu(pb))
    c.load_state_dict(sd)
    for _ in range(3):
        c.step()
    for x, y in zip(pa, pc):
        assert torch.equal(x, y)
    for key in ("exp_avg", "exp_avg_sq"):
        for x, y in zip(_state(a, pa, key), _state(c, pc, key)):
            assert torch.equal(x, y)
    ea, ec = a.ema_state_dict(), c.ema_state_dict()
    for k in ea:
        assert torch.equal(ea[k], ec[k]), k
    assert not torch.equal(ea["ps.0"], pa[0])
    assert torch.equal(a.scheduled, c.scheduled)
    out = c.state_dict()
    assert float(out["state"][0]["step"]) == 6 and out["yms"]["ema_step"] == 6 and out["yms"]["ema_rule"] == "exp_momentum"


# ---- 8. state dicts move between torch.optim.AdamW and yms.optim.AdamW ------------------------------
def test_adamw_state_dict_moves_between_torch_and_yms():
    p0, g0, _, _ = T._data()
    g1 = [g.flip(0) * 0.5 for g in g0]
    kw = dict(lr=LRS[0], betas=(B1, B2), eps=EPS, weight_decay=WD)
    tp = [torch.nn.Parameter(t.cuda()) for t in p0]
    topt = torch.optim.AdamW(T._groups(tp), foreach=False, **kw)
    for _ in range(2):
        for i in LIVE:
            tp[i].grad = g0[i].cuda()
        topt.step()

    def compare(params, opt, tparams, toptim, pre, g, t, what):
        for i in LIVE:
            bp, bm, bv, _ = adamw_bounds(pre[0][i], g[i], pre[1][i], pre[2][i], T._lr(i), WD, t)
            st, ts = opt.state[params[i]], toptim.state[tparams[i]]
            T._within(params[i], tparams[i].detach().double().cpu(), 2 * bp, f"p[{i}] vs torch {what}")
            T._within(st["exp_avg"], ts["exp_avg"].double().cpu(), 2 * bm, f"m[{i}] vs torch {what}")
            T._within(st["exp_avg_sq"], ts["exp_avg_sq"].double().cpu(), 2 * bv, f"v[{i}] vs torch {what}")

    # torch -> yms, then both take the same third step
    params = [torch.nn.Parameter(t.detach().clone()) for t in tp]
    opt = O.AdamW(T._groups(params), **kw)
    opt.load_state_dict(copy.deepcopy(topt.state_dict()))
    for i in LIVE:
        assert torch.equal(opt.state[params[i]]["exp_avg"], topt.state[tp[i]]["exp_avg"])
        assert torch.equal(opt.state[params[i]]["exp_avg_sq"], topt.state[tp[i]]["exp_avg_sq"])
    pre = [T._cpu(x) for x in (params, _state(opt, params, "exp_avg"), _state(opt, params, "exp_avg_sq"))]
    T._set_grads(params, g1)
    opt.step()
    for i in LIVE:
        tp[i].grad = g1[i].cuda()
    topt.step()
    compare(params, opt, tp, topt, pre, g1, 3, "after a torch state")
    assert float(opt.state_dict()["state"][0]["step"]) == 3
    # yms -> torch, then both take the same fourth step
    tq = [torch.nn.Parameter(t.detach().clone()) for t in params]
    topt2 = torch.optim.AdamW(T._groups(tq), foreach=False, **kw)
    topt2.load_state_dict(copy.deepcopy(opt.state_dict()))     # torch keeps the tensors it is given
    assert float(topt2.state[tq[0]]["step"]) == 3
    pre = [T._cpu(x) for x in (params, _state(opt, params, "exp_avg"), _state(opt, params, "exp_avg_sq"))]
    for i in LIVE:
        tq[i].grad = g0[i].cuda()
    topt2.step()
    T._set_grads(params, g0)
    opt.step()
    compare(params, opt, tq, topt2, pre, g0, 4, "after a yms state")


# ---- 9. the old paths ----------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["SGD", "Adam"])
def test_old_paths_still_go_through_yms_optim_step(cls, monkeypatch):
    p0, g0, m0, v0 = T._data()

    def new():
        params = T._params(p0)
        arena = T._set_grads(params, g0)
        if cls == "SGD":
            opt = O.SGD(T._groups(params), clip_grad_norm=1.0, **SGD_KW)
            T._load_state(opt, {i: {"momentum_buffer": m0[i]} for i in range(N)}, count=1)
        else:
            opt = O.Adam(T._groups(params), lr=LRS[0], weight_decay=5e-4, clip_grad_norm=1.0)
            T._load_state(opt, _adam_state(m0, v0, 3))
        opt.attach_ema(T.Toy(params))
        return params, opt, arena

    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    pa, a, _ = new()
    a.step()
    assert calls == ["yms_optim_grad_norm", "yms_optim_step"]
    monkeypatch.undo()
    results = [a]
    params = [pa]
    for ext in (False, True):            # the entry points themselves, on the same table
        pb, b, _ = new()
        (table, nchunks, partials, _), base = b._step_table()
        b.sync_hyper()
        st = L.stream_ptr()
        head = (b._KIND, table.data_ptr(), nchunks, base, b._hyper.data_ptr())
        tail = (partials.data_ptr(), partials.numel(), st)
        L.call("yms_optim_grad_norm", table.data_ptr(), nchunks, base, partials.data_ptr(), st)
        if ext:                          # ext == NULL: bit-identical to yms_optim_step
            L.call("yms_optim_step_ext", *head, None, b._counters.data_ptr(), None, *tail)
        else:
            L.call("yms_optim_step", *head, b._counters.data_ptr(), *tail)
        results.append(b)
        params.append(pb)
    torch.cuda.synchronize()
    for pb, b in zip(params[1:], results[1:]):
        for x, y in zip(pa, pb):
            assert torch.equal(x, y)
        for key in a._STATE_KEYS:
            for x, y in zip(_state(a, pa, key), _state(b, pb, key)):
                assert torch.equal(x, y)
        for x, y in zip(a.ema_state_dict().values(), b.ema_state_dict().values()):
            assert torch.equal(x, y)
        assert a._counts()[:3] == b._counts()[:3] and a.grad_norm.item() == b.grad_norm.item()
    assert not torch.equal(pa[0].detach().cpu(), p0[0])
