"""The head's grouped launches at plan level (Options.head_group, YMS_HEAD_GROUP): one training step
(forward, ComputeLoss, backward) and one eval forward of YOLOv8-n, with the head's three levels run
stage by stage as grouped launches (forward + backward, forward only) and off.  A grouped launch
decomposes every member exactly as its solo launch does, so the head maps, every parameter gradient,
the BatchNorm running buffers and the decoded output must be EQUAL bit for bit; the plans are
different cache entries.  (Parity with the oracle is the golden / oracle model tests' job: they run
the grouped path, the default.)"""
import pytest
import torch

from oracle import model_ref as M
from yms import set_compute_dtype
from yms.plan import HEAD_GROUP_DEFAULT, HeadGroup
from yolov8.tools.loss import ComputeLoss
from yolov8.yolov8 import YOLOv8

pytestmark = pytest.mark.gpu


def _run(mode, nc, dtype, x, sd, monkeypatch):
    if mode is None:
        monkeypatch.delenv("YMS_HEAD_GROUP", raising=False)
    else:
        monkeypatch.setenv("YMS_HEAD_GROUP", str(mode))
    m = YOLOv8("n", nc).cuda()
    m.load_state_dict(sd)
    m.train()
    if dtype != torch.float32:
        set_compute_dtype(m, dtype)
    crit = ComputeLoss(m.head, nc, "cuda", (64, 64))
    tg = torch.tensor([[0, 1, 0.5, 0.5, 0.4, 0.3], [1, 2, 0.3, 0.6, 0.2, 0.5], [1, 0, 0.7, 0.2, 0.3, 0.3]], device="cuda")
    outs = m(x)
    out = {f"map{i}": o.detach().clone() for i, o in enumerate(outs)}
    total, _ = crit(outs, tg)
    total.backward()
    out["loss"] = total.detach().clone()
    for k, p in m.named_parameters():
        if k != "head.dfl.conv.weight":
            assert p.grad is not None, k
            out["grad:" + k] = p.grad.clone()
    for k, b in m.named_buffers():
        out["buf:" + k] = b.clone()
    train_plan = next(iter(m.__dict__["_yms_plans"].values()))
    m.eval()
    m.head.stride = torch.tensor([8.0, 16.0, 32.0])
    out["decoded"] = m(x).clone()
    torch.cuda.synchronize()
    plans = list(m.__dict__["_yms_plans"].values())
    assert len(plans) == 2
    for p in plans:
        groups = [s for s in p.sched if isinstance(s, HeadGroup)]
        want = HEAD_GROUP_DEFAULT if mode is None else mode
        assert p.opts.head_group == want and len(groups) == (1 if want else 0)
        assert len(p.sched) == len(p.ops) - (15 - 1 if want else 0)     # 3 levels x 5 ops run as one step
    return out, m, train_plan


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("nc", [3, 80])
def test_head_group_is_bit_identical(nc, dtype, monkeypatch):
    sd = M.init_params("n", nc)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(nc)).cuda()
    off, _, _ = _run(0, nc, dtype, x, sd, monkeypatch)
    for mode in (2, 1):
        got, _, _ = _run(mode, nc, dtype, x, sd, monkeypatch)
        assert got.keys() == off.keys()
        for k in off:
            assert torch.equal(got[k], off[k]), f"head_group={mode}: {k} differs from the ungrouped run"
    assert all(torch.isfinite(v.float()).all() for v in off.values())


def test_head_group_switch_is_part_of_the_plan_key(monkeypatch):
    sd = M.init_params("n", 3)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)).cuda()
    _, m, p_on = _run(None, 3, torch.bfloat16, x, sd, monkeypatch)
    monkeypatch.setenv("YMS_HEAD_GROUP", "0")
    m.train()
    m(x)
    plans = list(m.__dict__["_yms_plans"].values())
    p_off = [p for p in plans if p.training and p is not p_on]
    assert len(plans) == 3 and len(p_off) == 1 and p_off[0].opts.head_group == 0
    assert not any(isinstance(s, HeadGroup) for s in p_off[0].sched)
    monkeypatch.delenv("YMS_HEAD_GROUP")
    m(x)
    assert len(m.__dict__["_yms_plans"]) == 3       # back on the first plan


def test_frozen_member_runs_the_members_own_backward(monkeypatch):
    """A frozen head parameter: the grouped backward steps aside (HeadGroup.bwd_grouped) and the step
    still equals the ungrouped one."""
    sd = M.init_params("n", 3)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(2)).cuda()
    res = []
    for mode in ("0", "2"):
        monkeypatch.setenv("YMS_HEAD_GROUP", mode)
        m = YOLOv8("n", 3).cuda()
        m.load_state_dict(sd)
        dict(m.named_parameters())["head.cls.1.1.bn.weight"].requires_grad_(False)
        m.train()
        set_compute_dtype(m, torch.bfloat16)
        outs = m(x)
        sum((o.float() ** 2).mean() for o in outs).backward()
        torch.cuda.synchronize()
        res.append({k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    assert res[0].keys() == res[1].keys() and "head.cls.1.1.bn.weight" not in res[0]
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k
