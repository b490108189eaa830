"""GPU tier of yms.optim (csrc/optim.hip): single SGD / Adam steps, the EMA, clipping, the non-finite
skip, determinism and launch counts, the model's eval cache, checkpoints and graph capture.

u = 2^-24.  "fp64 restatement" = the formulas of include/yms.h written below in torch.float64 on the
CPU.  Every bound is on ABSOLUTE-value magnitudes (a near-cancellation in g + wd p is bounded by its
operands, not by its result), counts the roundings of the fp32 evaluation and was fixed before any
run; torch's own CPU fp32 optimizers reach at most half of any of them on these inputs, and so did
the kernels on an MI355X (0.48 at most; each test prints its ratios)."""
import copy
import functools
import math

import pytest
import torch

from oracle import model_ref as M
from yms import checkpoint as CK
from yms import optim as O
from yms import set_compute_dtype
from yolov8.yolov8 import YOLOv8

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C = 4096                                # elements per table chunk
# the issue's sizes (1, 3, chunk -1 / +0 / +1, 3 chunks + 5, a 4-D weight) plus short and two-chunk tensors
SHAPES = [(1,), (3,), (C - 1,), (C,), (C + 1,), (3 * C + 5,), (16, 8, 3, 3), (7,), (64,), (257,), (2 * C,), (1000,)]
FROZEN = 9                              # no gradient
UNALIGNED_PARAM = 4                     # a parameter that is itself a view at an odd element offset
ALIGNED_GRAD = 10                       # the one gradient at a 16-B aligned arena offset (float4 gradient reads)
SPLIT = 6                               # parameters [0, 6) are group 0, the rest group 1
LRS = (0.01, 0.003)
MOM = 0.937
B1, B2, EPS = 0.9, 0.999, 1e-8
LIVE = [i for i in range(len(SHAPES)) if i != FROZEN]


@functools.lru_cache(maxsize=None)
def _data(gscale=1.0):
    """Shared fp32 CPU inputs (never modified): parameters, gradients, two state tensors."""
    gen = torch.Generator().manual_seed(1234)
    r = lambda s: torch.randn(s, generator=gen)
    p = [r(s) for s in SHAPES]
    g = [r(s) * gscale for s in SHAPES]
    m = [r(s) * gscale * 0.5 for s in SHAPES]
    v = [(torch.rand(s, generator=gen) + 0.01) * gscale * gscale for s in SHAPES]
    return p, g, m, v


def _grad_offsets():
    offs, off = [], 1
    for i, s in enumerate(SHAPES):
        if i == ALIGNED_GRAD:
            off = (off + 3) // 4 * 4
        elif off % 2 == 0:
            off += 1
        offs.append(off)
        off += math.prod(s)
    return offs, off


def _params(p_cpu):
    out = []
    for i, t in enumerate(p_cpu):
        if i == UNALIGNED_PARAM:
            d = torch.empty(t.numel() + 1, device="cuda")[1:].view(t.shape)
            d.copy_(t)
        else:
            d = t.cuda()
        out.append(torch.nn.Parameter(d))
    assert out[UNALIGNED_PARAM].data_ptr() % 16 == 4 and out[UNALIGNED_PARAM].is_contiguous()
    return out


def _set_grads(params, g_cpu, flat=True):
    """Gradients as views of one flat arena at odd element offsets (one aligned); FROZEN has none."""
    offs, total = _grad_offsets()
    arena = torch.zeros(total, device="cuda")
    for i, (p, g) in enumerate(zip(params, g_cpu)):
        if i == FROZEN:
            p.grad = None
            continue
        if flat:
            view = arena[offs[i]:offs[i] + g.numel()].view(g.shape)
            view.copy_(g)
            p.grad = view
        else:
            p.grad = g.cuda()
    return arena


def _groups(params, **second):
    return [{"params": params[:SPLIT], "lr": LRS[0]}, dict({"params": params[SPLIT:], "lr": LRS[1]}, **second)]


def _load_state(opt, per_param, count=None):
    """Put state into the optimizer the public way: a torch-format state dict."""
    sd = opt.state_dict()
    sd["state"] = {i: {k: (t.clone() if isinstance(t, torch.Tensor) else t) for k, t in st.items()}
                   for i, st in per_param.items()}
    if count is None:
        del sd["yms"]
    else:
        sd["yms"] = {"step": count}
    opt.load_state_dict(sd)


def _cpu(ts):
    return [t.detach().cpu().clone() for t in ts]


def _lr(i):
    return LRS[0] if i < SPLIT else LRS[1]


# ---- fp64 restatements --------------------------------------------------------------------------
def sgd64(p, g, b, lr, mom, wd, nesterov, first, coef=1.0):
    p, g, b = p.double(), g.double(), b.double()
    d = g * coef + wd * p
    b2 = d if first else mom * b + d
    return p - lr * (d + mom * b2 if nesterov else b2), b2


def sgd_bounds(p, g, b, lr, mom, wd, nesterov, first):
    p, g, b = p.double().abs(), g.double().abs(), b.double().abs()
    c1, c2 = (1 + mom, mom * mom) if nesterov else (1.0, mom)
    if first:
        c2 = 0.0
    upd = lr * (c1 * (g + wd * p) + c2 * b)
    return 8 * U * (p + upd), 4 * U * ((0.0 if first else mom) * b + g + wd * p), upd


def adam64(p, g, m, v, lr, wd, t, coef=1.0):
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    d = g * coef + wd * p
    m2 = B1 * m + (1 - B1) * d
    v2 = B2 * v + (1 - B2) * d * d
    bc1, bc2 = 1 - B1 ** t, 1 - B2 ** t
    den = v2.sqrt() / math.sqrt(bc2) + EPS
    return p - (lr / bc1) * m2 / den, m2, v2, den, bc1


def adam_bounds(p, g, m, v, lr, wd, t):
    _, _, _, den, bc1 = adam64(p, g, m, v, lr, wd, t)
    p, g, m, v = p.double().abs(), g.double().abs(), m.double().abs(), v.double()
    d = g + wd * p
    upd = lr / (bc1 * den) * (B1 * m + (1 - B1) * d)
    return 16 * U * (p + upd), 4 * U * (m + d), 16 * U * (B2 * v + (1 - B2) * d * d), upd


def _within(got, want, bound, what):
    err = (got.detach().double().cpu() - want).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max err / bound = {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)


# ---- single steps -------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("nesterov", [True, False])
def test_sgd_single_step(nesterov, first, wd):
    p0, g0, b0, _ = _data()
    params = _params(p0)
    _set_grads(params, g0)
    opt = O.SGD(_groups(params), lr=LRS[0], momentum=MOM, nesterov=nesterov, weight_decay=wd)
    # nonzero momentum in both cases: the first update must ignore it
    _load_state(opt, {i: {"momentum_buffer": b0[i]} for i in range(len(params))}, count=0 if first else 1)
    opt.step()
    assert opt.last_launches == 2
    # torch.optim.SGD on the same tensors
    tp = [torch.nn.Parameter(t.cuda()) for t in p0]
    topt = torch.optim.SGD(_groups(tp), lr=LRS[0], momentum=MOM, nesterov=nesterov, weight_decay=wd, foreach=False)
    for i in LIVE:
        tp[i].grad = g0[i].cuda()
        if not first:
            topt.state[tp[i]]["momentum_buffer"] = b0[i].cuda()
    topt.step()
    for i in LIVE:
        a = (p0[i], g0[i], b0[i], _lr(i), MOM, wd, nesterov, first)
        p64, b64 = sgd64(*a)
        bp, bb, _ = sgd_bounds(*a)
        _within(params[i], p64, bp, f"p[{i}]")
        _within(opt.state[params[i]]["momentum_buffer"], b64, bb, f"b[{i}]")
        _within(params[i], tp[i].detach().double().cpu(), 2 * bp, f"p[{i}] vs torch")
        _within(opt.state[params[i]]["momentum_buffer"], topt.state[tp[i]]["momentum_buffer"].double().cpu(), 2 * bb,
                f"b[{i}] vs torch")
    assert torch.equal(params[FROZEN].detach().cpu(), p0[FROZEN])
    assert torch.equal(opt.state[params[FROZEN]]["momentum_buffer"].cpu(), b0[FROZEN])


@pytest.mark.parametrize("gscale", [1e-4, 1.0, 50.0])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_adam_single_step(t, wd, gscale):
    p0, g0, m0, v0 = _data(gscale)
    if t == 1:                           # torch's state before its first step
        m0, v0 = [torch.zeros_like(x) for x in m0], [torch.zeros_like(x) for x in v0]
    params = _params(p0)
    _set_grads(params, g0)
    opt = O.Adam(_groups(params), lr=LRS[0], betas=(B1, B2), eps=EPS, weight_decay=wd)
    _load_state(opt, {i: {"step": torch.tensor(float(t - 1)), "exp_avg": m0[i], "exp_avg_sq": v0[i]}
                      for i in range(len(params))})
    opt.step()
    assert opt.last_launches == 2
    tp = [torch.nn.Parameter(x.cuda()) for x in p0]
    topt = torch.optim.Adam(_groups(tp), lr=LRS[0], betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
    for i in LIVE:
        tp[i].grad = g0[i].cuda()
        topt.state[tp[i]].update(step=torch.tensor(float(t - 1)), exp_avg=m0[i].cuda(), exp_avg_sq=v0[i].cuda())
    topt.step()
    for i in LIVE:
        a = (p0[i], g0[i], m0[i], v0[i], _lr(i), wd, t)
        p64, m64, v64, _, _ = adam64(*a)
        bp, bm, bv, _ = adam_bounds(*a)
        st, ts = opt.state[params[i]], topt.state[tp[i]]
        _within(params[i], p64, bp, f"p[{i}]")
        _within(st["exp_avg"], m64, bm, f"m[{i}]")
        _within(st["exp_avg_sq"], v64, bv, f"v[{i}]")
        _within(params[i], tp[i].detach().double().cpu(), 2 * bp, f"p[{i}] vs torch")
        _within(st["exp_avg"], ts["exp_avg"].double().cpu(), 2 * bm, f"m[{i}] vs torch")
        _within(st["exp_avg_sq"], ts["exp_avg_sq"].double().cpu(), 2 * bv, f"v[{i}] vs torch")
    assert torch.equal(params[FROZEN].detach().cpu(), p0[FROZEN])
    assert torch.equal(opt.state[params[FROZEN]]["exp_avg"].cpu(), m0[FROZEN])
    assert torch.equal(opt.state[params[FROZEN]]["exp_avg_sq"].cpu(), v0[FROZEN])
    assert float(opt.state_dict()["state"][0]["step"]) == t


# ---- EMA ----------------------------------------------------------------------------------------
class Toy(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        self.ps = torch.nn.ParameterList(params)
        self.register_buffer("stat", torch.randn(300, generator=torch.Generator().manual_seed(5)).cuda())
        self.register_buffer("count", torch.tensor(3))


@pytest.mark.parametrize("tau", [2000.0, 1.0])
def test_ema_follows_parameters_and_buffers(tau):
    p0, g0, _, _ = _data()
    params = _params(p0)
    _set_grads(params, g0)
    toy = Toy(params)
    opt = O.SGD(_groups(params), lr=LRS[0], momentum=MOM, nesterov=True, weight_decay=5e-4)
    opt.attach_ema(toy, decay=0.9999, tau=tau)
    e = opt.ema_state_dict()
    assert list(e) == list(toy.state_dict())
    for k, v in toy.state_dict().items():
        assert torch.equal(e[k], v), k                     # seeded from the current values
    for k in (1, 2, 3):
        toy.stat.add_(0.5)                                  # the forward writes the BN statistics
        opt.step()
        assert opt.last_launches == 2
        e2, live = opt.ema_state_dict(), toy.state_dict()
        delta = 0.9999 * (1.0 - math.exp(-k / tau))
        for name in e:
            if name == "count":
                assert torch.equal(e2[name], live[name])
                continue
            old, new = e[name].double().cpu(), live[name].double().cpu()   # the kernel's own p'
            _within(e2[name], delta * old + (1 - delta) * new, 8 * U * (old.abs() + new.abs()), f"ema {name} k={k}")
        e = e2
    assert not torch.equal(e["stat"], toy.stat)
    before = {k: v.clone() for k, v in toy.state_dict().items()}
    vers = [p._version for p in params]
    with opt.ema_applied():
        for k, v in toy.state_dict().items():
            assert torch.equal(v, e[k]), k
        assert all(p._version > v0 for p, v0 in zip(params, vers))
    for k, v in toy.state_dict().items():
        assert torch.equal(v, before[k]), k
    for k, v in opt.ema_state_dict().items():
        assert torch.equal(v, e[k]), k


# ---- clipping and the non-finite skip -------------------------------------------------------------
def _norm64(g0):
    return math.sqrt(sum((g0[i].double() ** 2).sum().item() for i in LIVE))


def _sgd_with_state(p0, g0, b0, **kw):
    params = _params(p0)
    arena = _set_grads(params, g0)
    opt = O.SGD(_groups(params), lr=LRS[0], momentum=MOM, nesterov=True, weight_decay=5e-4, **kw)
    _load_state(opt, {i: {"momentum_buffer": b0[i]} for i in range(len(params))}, count=1)
    return params, opt, arena


def test_clip_grad_norm():
    p0, g0, b0, _ = _data()
    norm = _norm64(g0)
    params, opt, _ = _sgd_with_state(p0, g0, b0, clip_grad_norm=0.5 * norm)
    opt.step()
    assert opt.last_launches == 3
    got = opt.grad_norm.item()
    print(f"grad_norm rel err = {abs(got - norm) / norm:.3g}")
    assert abs(got - norm) <= 1e-5 * norm
    coef = 0.5 * norm / (norm + 1e-6)
    for i in LIVE:
        a = (p0[i], g0[i], b0[i], _lr(i), MOM, 5e-4, True, False)
        p64, b64 = sgd64(*a, coef=coef)
        bp, bb, upd = sgd_bounds(*a)
        _within(params[i], p64, bp + 1e-5 * upd, f"clipped p[{i}]")
        _within(opt.state[params[i]]["momentum_buffer"], b64,
                bb + 1e-5 * (g0[i].double().abs() + 5e-4 * p0[i].double().abs()), f"clipped b[{i}]")
    # a limit above the norm changes nothing, bit for bit
    pa, oa, _ = _sgd_with_state(p0, g0, b0, clip_grad_norm=2.0 * norm)
    pb, ob, _ = _sgd_with_state(p0, g0, b0)
    oa.step()
    ob.step()
    assert (oa.last_launches, ob.last_launches) == (3, 2)
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
        assert torch.equal(oa.state[x]["momentum_buffer"], ob.state[y]["momentum_buffer"])


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_step_is_skipped(bad):
    p0, g0, m0, v0 = _data()
    state = {i: {"step": torch.tensor(0.0), "exp_avg": m0[i], "exp_avg_sq": v0[i]} for i in range(len(SHAPES))}

    def new():
        params = _params(p0)
        arena = _set_grads(params, g0)
        toy = Toy(params)
        opt = O.Adam(_groups(params), lr=LRS[0], weight_decay=5e-4, skip_nonfinite=True)
        opt.attach_ema(toy)
        _load_state(opt, state)
        return params, toy, opt, arena

    params, toy, opt, arena = new()
    snap = lambda: (_cpu(params), _cpu(opt.state[p]["exp_avg"] for p in params),
                    _cpu(opt.state[p]["exp_avg_sq"] for p in params), _cpu(opt.ema_state_dict().values()))
    s0 = snap()
    keep = params[5].grad[7].clone()
    params[5].grad[7] = bad
    opt.step()
    assert opt.last_launches == 3
    for a, b in zip(s0, snap()):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert opt.skipped_steps.item() == 1
    sd = opt.state_dict()
    assert float(sd["state"][0]["step"]) == 0 and sd["yms"]["ema_step"] == 0 and sd["yms"]["skipped"] == 1
    assert not math.isfinite(opt.grad_norm.item())
    # the next finite step is update number one: the same as on an optimizer that never skipped
    params[5].grad[7] = keep
    opt.step()
    rp, rtoy, ropt, _ = new()
    ropt.step()
    for a, b in zip(snap(), (_cpu(rp), _cpu(ropt.state[p]["exp_avg"] for p in rp),
                             _cpu(ropt.state[p]["exp_avg_sq"] for p in rp), _cpu(ropt.ema_state_dict().values()))):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert float(opt.state_dict()["state"][0]["step"]) == 1 and opt.skipped_steps.item() == 1
    assert not torch.equal(params[0].detach().cpu(), p0[0])


# ---- determinism, launch counts, the fallback ------------------------------------------------------
def test_deterministic_and_launch_count_independent_of_tensor_count():
    p0, g0, b0, _ = _data()
    runs = []
    for flat in (True, True, False):
        params = _params(p0)
        _set_grads(params, g0, flat=flat)
        opt = O.SGD(_groups(params), lr=LRS[0], momentum=MOM, nesterov=True, weight_decay=5e-4, clip_grad_norm=1.0)
        _load_state(opt, {i: {"momentum_buffer": b0[i]} for i in range(len(params))}, count=1)
        opt.step()
        runs.append((_cpu(params), _cpu(opt.state[p]["momentum_buffer"] for p in params),
                     opt.grad_norm.cpu().view(torch.int32).item(), opt.last_launches))
    for other in runs[1:]:               # the same step again, and through the absolute-address table
        for a, b in zip(runs[0][:2], other[:2]):
            for x, y in zip(a, b):
                assert torch.equal(x, y)
        assert other[2:] == runs[0][2:]
    assert runs[0][3] == 3
    # the YOLOv8-n parameter set: the same launch counts as for 12 tensors
    model = YOLOv8("n", 3).cuda()
    mp = [p for p in model.parameters() if p.requires_grad]
    assert len(mp) > 100
    arena = torch.randn(sum(p.numel() for p in mp), device="cuda") * 0.01
    off = 0
    for p in mp:
        p.grad = arena[off:off + p.numel()].view(p.shape)
        off += p.numel()
    for kw, n in ((dict(), 2), (dict(clip_grad_norm=10.0), 3), (dict(skip_nonfinite=True), 3)):
        opt = O.SGD(mp, lr=0.01, momentum=MOM, nesterov=True, **kw)
        opt.attach_ema(model)
        opt.step()
        assert opt.last_launches == n and opt.table_builds == 1
        opt.step()
        assert opt.last_launches == n and opt.table_builds == 1
    plain = O.Adam(mp)
    plain.step()
    assert plain.last_launches == 2
    torch.cuda.synchronize()


# ---- the model: versions, eval cache, table cache -------------------------------------------------
def _model(sd):
    m = YOLOv8("n", 3).cuda()
    m.load_state_dict(sd)
    m.head.stride = torch.tensor([8.0, 16.0, 32.0])
    set_compute_dtype(m, torch.bfloat16)
    return m


def _train_step(m, opt, seed):
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(seed)).cuda()
    m.train()
    opt.zero_grad(set_to_none=True)
    loss = sum((o.float() ** 2).mean() for o in m(x))
    loss.backward()
    opt.step()


def test_model_step_bumps_versions_and_rebuilds_the_eval_cache():
    m = _model(M.init_params("n", 3))
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(9)).cuda()
    m.eval()
    with torch.no_grad():
        y0 = m(x).clone()                # the eval cache now holds the initial weights
    opt = O.SGD(m.parameters(), lr=0.01, momentum=MOM, nesterov=True, weight_decay=5e-4)
    vers = {k: p._version for k, p in m.named_parameters()}
    _train_step(m, opt, 0)
    written = [k for k, p in m.named_parameters() if p.grad is not None]
    assert len(written) > 100
    storages = {p.grad.untyped_storage().data_ptr() for p in m.parameters() if p.grad is not None}
    assert len(storages) == 1, "the backward's gradients are views of one flat arena"
    for k, p in m.named_parameters():
        if p.grad is not None:
            assert p._version > vers[k], k
    m.eval()
    with torch.no_grad():
        y1 = m(x).clone()
    m2 = _model(m.state_dict())
    m2.eval()
    with torch.no_grad():
        y2 = m2(x)
    assert torch.equal(y1, y2)           # inference sees the stepped weights
    assert not torch.equal(y1, y0)
    # the table cache: fresh gradients of the same layout hit it; a new freeze pattern misses once
    assert opt.table_builds == 1
    _train_step(m, opt, 1)
    assert opt.table_builds == 1
    frozen = dict(m.named_parameters())["head.cls.1.1.bn.weight"]
    frozen.requires_grad_(False)
    _train_step(m, opt, 2)
    assert frozen.grad is None and opt.table_builds == 2
    _train_step(m, opt, 3)
    assert opt.table_builds == 2
    torch.cuda.synchronize()


# ---- checkpoints ----------------------------------------------------------------------------------
def test_resume_with_adam_and_ema_is_exact(tmp_path):
    def new(sd):
        m = YOLOv8("n", 80).cuda()
        m.load_state_dict(sd)
        opt = O.Adam(m.parameters(), lr=1e-3, weight_decay=5e-4, clip_grad_norm=10.0, skip_nonfinite=True)
        opt.attach_ema(m, tau=5)
        return m, opt

    m, opt = new(M.init_params("n", 80))
    for s in range(2):
        _train_step(m, opt, s)
    f = str(tmp_path / "ck.pt")
    CK.save_checkpoint(f, m, opt, epoch=1)
    _train_step(m, opt, 2)
    m2, opt2 = new(M.init_params("n", 80))
    info = CK.load_checkpoint(f, m2, opt2)
    assert info["epoch"] == 1 and info["has_optimizer"]
    _train_step(m2, opt2, 2)
    torch.cuda.synchronize()
    for (k, a), b in zip(m.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), k
    ea, eb = opt.ema_state_dict(), opt2.ema_state_dict()
    assert list(ea) == list(m.state_dict())
    for k in ea:
        assert torch.equal(ea[k], eb[k]), k
    assert not torch.equal(ea["backbone.conv0.conv.weight"], m.state_dict()["backbone.conv0.conv.weight"])
    sd = opt2.state_dict()
    assert float(sd["state"][0]["step"]) == 3 and sd["yms"]["ema_step"] == 3


def test_sgd_state_dict_moves_between_torch_and_yms():
    p0, g0, _, _ = _data()
    g1 = [g.flip(0) * 0.5 for g in g0]
    kw = dict(lr=LRS[0], momentum=MOM, nesterov=True, weight_decay=5e-4)
    tp = [torch.nn.Parameter(t.cuda()) for t in p0]
    topt = torch.optim.SGD(_groups(tp), foreach=False, **kw)
    for i in LIVE:
        tp[i].grad = g0[i].cuda()
    topt.step()
    # torch -> yms
    params = [torch.nn.Parameter(t.detach().clone()) for t in tp]
    opt = O.SGD(_groups(params), **kw)
    opt.load_state_dict(topt.state_dict())
    p1 = _cpu(params)
    b1 = [opt.state[p]["momentum_buffer"].cpu().clone() for p in params]
    for i in LIVE:
        assert torch.equal(b1[i], topt.state[tp[i]]["momentum_buffer"].cpu())
    _set_grads(params, g1)
    opt.step()
    for i in LIVE:
        a = (p1[i], g1[i], b1[i], _lr(i), MOM, 5e-4, True, False)
        _within(params[i], sgd64(*a)[0], sgd_bounds(*a)[0], f"p[{i}] after a torch state")
    # yms -> torch, then both take the same step
    tq = [torch.nn.Parameter(t.detach().clone()) for t in params]
    topt2 = torch.optim.SGD(_groups(tq), foreach=False, **kw)
    topt2.load_state_dict(copy.deepcopy(opt.state_dict()))     # torch keeps the tensors it is given
    p2 = _cpu(params)
    b2 = [opt.state[p]["momentum_buffer"].cpu().clone() for p in params]
    for i in LIVE:
        tq[i].grad = g0[i].cuda()
    topt2.step()
    _set_grads(params, g0)
    opt.step()
    for i in LIVE:
        a = (p2[i], g0[i], b2[i], _lr(i), MOM, 5e-4, True, False)
        bp, bb, _ = sgd_bounds(*a)
        _within(params[i], tq[i].detach().double().cpu(), 2 * bp, f"p[{i}] vs torch after a yms state")
        _within(opt.state[params[i]]["momentum_buffer"], topt2.state[tq[i]]["momentum_buffer"].double().cpu(), 2 * bb,
                f"b[{i}] vs torch after a yms state")


# ---- graph capture ----------------------------------------------------------------------------------
def test_captured_step_sees_a_new_learning_rate():
    p0, g0, _, _ = _data()

    def new():
        params = _params(p0)
        arena = _set_grads(params, g0)
        opt = O.Adam(_groups(params), lr=LRS[0], weight_decay=5e-4, clip_grad_norm=100.0)
        opt.attach_ema(Toy(params))
        return params, opt, arena

    def set_lr(opt, scale):
        for g, lr in zip(opt.param_groups, LRS):
            g["lr"] = lr * scale

    ep, eopt, ea = new()                 # eager: four steps, the last at another learning rate
    for s in range(4):
        set_lr(eopt, 0.1 if s == 3 else 1.0)
        eopt.step()
    gp, gopt, ga = new()
    gopt.step()
    gopt.step()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gopt.step()
    assert gopt.last_launches == 3 and gopt.table_builds == 1
    graph.replay()
    with pytest.raises(RuntimeError, match="sync_hyper"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            gopt.step()                  # (captured, never replayed)
            set_lr(gopt, 0.1)
            gopt.step()                  # param_groups differ from the device copy: no upload inside a capture
    gopt.sync_hyper()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(ep, gp):
        assert torch.equal(x, y)
    for x, y in zip(eopt.ema_state_dict().values(), gopt.ema_state_dict().values()):
        assert torch.equal(x, y)
    assert float(gopt.state_dict()["state"][0]["step"]) == 4


def test_table_miss_during_capture_raises():
    p0, g0, _, _ = _data()
    params = _params(p0)
    _set_grads(params, g0)
    opt = O.SGD(_groups(params), lr=LRS[0], momentum=MOM)
    opt.step()
    before = _cpu(params)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="warm-up"):
        with torch.cuda.graph(graph):
            opt.step()                   # the warmed-up table: captured
            params[0].grad = None        # another gradient pattern: its table is not on the device
            opt.step()
    torch.cuda.synchronize()
    assert opt.table_builds == 1
    for x, y in zip(before, _cpu(params)):
        assert torch.equal(x, y)         # nothing ran
