"""The head's sibling first convs (yolov8_head.py:84-85, 99-100: box[i][0] and cls[i][0] both read
x_i) run as one SiblingConvOp (yms/plan.py): outputs in the slots of one buffer, one BN backward
pass, one input gradient and one weight gradient over both.  Checked against the unfused plan
(YMS_HEAD_FUSE=0, one ConvOp per module) on the same weights and batch: the forward maps and the BN
running buffers are bit-identical (each member's conv, statistics and finalize are unchanged; the
affine pass is elementwise), and the parameter gradients agree to the accumulation-order rounding
(fp32: the reduce's per-block pixel order differs with the channel count; 16-bit: the unfused
input gradient rounds dx twice, store then accumulate; checked through the drift from fp32).  The
fused fp32 path is also covered by every fp32 oracle / golden model test, which run it by default."""
import pytest
import torch

from yms import set_compute_dtype
from yms.plan import SiblingConvOp
from yolov8.yolov8 import YOLOv8

pytestmark = pytest.mark.gpu


def _step(fuse, dtype, version, nc, x, sd, monkeypatch):
    monkeypatch.setenv("YMS_HEAD_FUSE", "1" if fuse else "0")
    m = YOLOv8(version, nc).cuda()
    m.load_state_dict(sd)
    m.train()
    if dtype != torch.float32:
        set_compute_dtype(m, dtype)
    outs = m(x)
    plans = list(m.__dict__["_yms_plans"].values())
    assert any(isinstance(op, SiblingConvOp) for op in plans[0].ops) == fuse
    g = torch.Generator(device="cuda").manual_seed(3)
    loss = sum((o.float() * torch.randn(o.shape, device="cuda", generator=g)).sum() for o in outs)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().float().clone() for k, p in m.named_parameters() if p.grad is not None}
    bufs = {k: b.detach().clone() for k, b in m.named_buffers()}
    return [o.detach().float().clone() for o in outs], grads, bufs


@pytest.mark.parametrize("version,nc,size", [("s", 80, 256), ("n", 3, 192), ("ms-s", 80, 256)])
def test_sibling_head_convs_match_unfused(version, nc, size, monkeypatch):
    torch.manual_seed(0)
    sd = YOLOv8(version, nc).state_dict()
    x = torch.randn(2, 3, size, size, generator=torch.Generator().manual_seed(1)).cuda()
    # fp32: the fused and unfused plans agree to accumulation-order rounding
    o1, g32, b1 = _step(True, torch.float32, version, nc, x, sd, monkeypatch)
    o0, g0, b0 = _step(False, torch.float32, version, nc, x, sd, monkeypatch)
    for a, b in zip(o1, o0):
        assert torch.equal(a, b)
    for k in b0:
        assert torch.equal(b1[k], b0[k]), k
    assert g32.keys() == g0.keys() and any(k.startswith("head.cls.0.0") for k in g0)
    for k in g0:
        d = ((g32[k] - g0[k]).norm() / (g0[k].norm() + 1e-30)).item()
        assert d <= 2e-5, (k, d)
    # bf16: forward and running buffers still bit-identical; the gradients' drift from the fp32
    # gradients is no larger fused than unfused (random-init graphs amplify any rounding difference
    # on its way back through the BN layers, so the two bf16 runs are compared through their drift)
    o1, g1, b1 = _step(True, torch.bfloat16, version, nc, x, sd, monkeypatch)
    o0, g0, b0 = _step(False, torch.bfloat16, version, nc, x, sd, monkeypatch)
    for a, b in zip(o1, o0):
        assert torch.equal(a, b)
    for k in b0:
        assert torch.equal(b1[k], b0[k]), k
    # (nc = 3: the z buffers' padding channels start zeroed -- arena garbage there used to turn the
    # input gradient NaN through zero weight rows, fused or not.  A fresh arena is usually zero pages,
    # so this only watches for it: tests/test_arena_poison_gpu.py fills the arenas with NaN and
    # test_gate_reports_unzeroed_z_padding there takes exactly this zeroing away)
    for gg in (g1, g0):
        bad = [k for k, t in gg.items() if not torch.isfinite(t).all()]
        assert not bad, bad[:5]
    d1 = torch.tensor([((g1[k] - g32[k]).norm() / (g32[k].norm() + 1e-30)).item() for k in g32])
    d0 = torch.tensor([((g0[k] - g32[k]).norm() / (g32[k].norm() + 1e-30)).item() for k in g32])
    assert d1.median() <= 1.2 * d0.median() and d1.max() <= 1.5 * d0.max(), (d1.median(), d0.median(), d1.max(), d0.max())


# ---- the non-adjacent fallback of SiblingConvOp.bwd (some member parameters frozen) -----------------
def _freeze_names(pattern):
    cls_bn = lambda i: [f"head.cls.{i}.0.bn.weight"]
    box_w = lambda i: [f"head.box.{i}.0.conv.weight"]
    cls_all = lambda i: [f"head.cls.{i}.0.conv.weight", f"head.cls.{i}.0.bn.weight", f"head.cls.{i}.0.bn.bias"]
    if pattern == "cls_bn_weight":       # dgamma / dbeta through the scratch table and per-member copies
        return sum((cls_bn(i) for i in range(3)), [])
    if pattern == "box_conv_weight":     # per-member weight gradient of the cls member only (dz at offset 64)
        return sum((box_w(i) for i in range(3)), [])
    if pattern == "cls_all":
        return sum((cls_all(i) for i in range(3)), [])
    return cls_bn(0) + box_w(1)          # mixed: level 2 keeps the adjacent path


def _step_frozen(fuse, dtype, nc, x, sd, frozen, monkeypatch):
    monkeypatch.setenv("YMS_HEAD_FUSE", "1" if fuse else "0")
    m = YOLOv8("n", nc).cuda()
    m.load_state_dict(sd)
    pd = dict(m.named_parameters())
    for k in frozen:
        pd[k].requires_grad_(False)      # before the first forward
    m.train()
    if dtype != torch.float32:
        set_compute_dtype(m, dtype)
    outs = m(x)
    plans = list(m.__dict__["_yms_plans"].values())
    assert any(isinstance(op, SiblingConvOp) for op in plans[0].ops) == fuse
    sum((o.double() ** 2).mean() for o in outs).backward()     # the oracle's loss (_oracle_grads)
    torch.cuda.synchronize()
    for k in frozen:
        assert pd[k].grad is None, k
    grads = {k: p.grad.detach().float().clone() for k, p in pd.items() if p.grad is not None}
    assert set(grads) == {k for k, p in pd.items() if p.requires_grad}
    bad = [k for k, t in grads.items() if not torch.isfinite(t).all()]
    assert not bad, bad[:5]
    return grads


_ORACLE = {}


def _oracle(nc):
    """fp64 CPU gradients of every parameter (one run per nc, shared by the freeze patterns)"""
    if nc not in _ORACLE:
        from oracle import model_ref as M
        from test_model_gpu import _oracle_grads
        sd = M.init_params("n", nc)
        x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(1))
        _ORACLE[nc] = (sd, x, _oracle_grads("n", nc, sd, x, torch.float64))
    return _ORACLE[nc]


@pytest.mark.parametrize("pattern", ["cls_bn_weight", "box_conv_weight", "cls_all", "mixed"])
@pytest.mark.parametrize("nc", [3, 80])
def test_sibling_fallback_with_frozen_members(pattern, nc, monkeypatch):
    """Members' parameter gradients not adjacent in the gradient arena (some frozen before the first
    forward): SiblingConvOp.bwd finalizes dgamma / dbeta into its scratch table and copies each
    member's slice out, and runs one weight gradient per unfrozen member on dz at its channel offset.
    Frozen parameters get no gradient, every other gradient is finite; fp32: within 2e-5 (relative L2)
    of the unfused plan with the same parameters frozen, and within 1e-3 of the fp64 CPU oracle (the
    gradient of an unfrozen parameter does not depend on what else is frozen); bf16: the drift from
    the fp32 gradients is no larger than the unfused plan's (median <= 1.2x, maximum <= 1.5x)."""
    from test_model_gpu import _rel
    sd, x, g64 = _oracle(nc)
    frozen = _freeze_names(pattern)
    xd = x.cuda()
    g32 = _step_frozen(True, torch.float32, nc, xd, sd, frozen, monkeypatch)
    g0 = _step_frozen(False, torch.float32, nc, xd, sd, frozen, monkeypatch)
    assert g32.keys() == g0.keys() and not set(frozen) & set(g32)
    assert any(k.startswith("head.cls.0.0") or k.startswith("head.box.0.0") for k in g32)
    for k in g0:
        d = ((g32[k] - g0[k]).norm() / (g0[k].norm() + 1e-30)).item()
        assert d <= 2e-5, (k, d)
    worst = max((_rel(g32[k], g64[k]), k) for k in g32)
    assert worst[0] < 1e-3, worst
    g1 = _step_frozen(True, torch.bfloat16, nc, xd, sd, frozen, monkeypatch)
    gb0 = _step_frozen(False, torch.bfloat16, nc, xd, sd, frozen, monkeypatch)
    d1 = torch.tensor([((g1[k] - g32[k]).norm() / (g32[k].norm() + 1e-30)).item() for k in g32])
    d0 = torch.tensor([((gb0[k] - g32[k]).norm() / (g32[k].norm() + 1e-30)).item() for k in g32])
    assert d1.median() <= 1.2 * d0.median() and d1.max() <= 1.5 * d0.max(), (d1.median(), d0.median(), d1.max(), d0.max())


@pytest.mark.parametrize("nc", [1, 17])
def test_sibling_bf16_grads_finite_ragged_nc(nc, monkeypatch):
    """The z buffers' padding channels (65 -> 72, 81 -> 88) start zeroed: arena garbage there used to
    turn the input gradient NaN through zero weight rows (asserted for nc = 3 above).  The deterministic
    check, on arenas filled with NaN, is tests/test_arena_poison_gpu.py (nc = 3 and 17)."""
    torch.manual_seed(0)
    sd = YOLOv8("n", nc).state_dict()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)).cuda()
    _, g, _ = _step(True, torch.bfloat16, "n", nc, x, sd, monkeypatch)
    bad = [k for k, t in g.items() if not torch.isfinite(t).all()]
    assert not bad, bad[:5]
