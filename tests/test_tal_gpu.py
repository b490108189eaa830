"""The task-aligned loss kernels (csrc/tal_loss.hip via yolov8.tools.tal_loss) against the
restatement tests/tal_ref.py on the seeded inputs of tests/tal_cases.py: the assignment exactly
(tests/test_tal_cpu.py asserts that every decision of the restatement on these inputs has a margin
above 1e-4 relative, or is an exact tie built on purpose), the target scores, the four values and
the per-level gradient.

Tolerances are the project's loss tolerances (tests/test_loss_gpu.py): values 2e-5 relative (floor
1e-3), gradients 2e-4 relative L2 per level for fp32 maps; 1e-4 / 4e-3 for bf16 / f16 maps (both
sides see the rounded maps; the gradient is stored in the 16-bit type, half-ulp 2^-9 per element);
5e-5 / 5e-4 on the full 640 grid.  The restatement evaluated in fp32 on the CPU differs from its
fp64 self by at most 5.8e-7 (values), 5.9e-7 (gradients) and 2.1e-6 (target scores, relative to the
largest) over these cases, so metric^6 and the division by tss need no more than that.  Target
scores are held to the value tolerance relative to the largest score."""
import pytest
import torch

import tal_cases as C
from yolov8.tools.tal_loss import TaskAlignedLoss, tal_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"

TOL = {torch.float32: (2e-5, 2e-4), torch.bfloat16: (1e-4, 4e-3), torch.float16: (1e-4, 4e-3)}


def _channels_last(p, dtype):
    """NCHW-shaped channels-last view of an NHWC buffer, like the plan's head outputs."""
    return p.to(DEV, dtype).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _run(c, need_grad=True, assignment=True):
    preds = [_channels_last(m, c["dtype"]) for m in c["maps"]]
    return tal_loss(preds, c["targets"].to(DEV), c["nc"], c["img"], c["strides"], c["topk"], c["alpha"], c["beta"],
                    need_grad=need_grad, return_assignment=assignment)


def _compare(name, vtol=None, gtol=None):
    c, r, rgrads = C.reference(name)
    tv, tg = TOL[c["dtype"]]
    vtol, gtol = vtol or tv, gtol or tg
    out, grads, (agt, asc) = _run(c)
    B = c["maps"][0].shape[0]
    assert agt.shape == (B, r["gt"].shape[1]) and torch.equal(agt.cpu().long(), r["gt"]), name
    serr = ((asc.cpu().double() - r["t"]).abs().max() / r["t"].max().clamp_min(1e-30)).item()
    o = out.cpu().double()
    ref = torch.stack([r["total"], r["box"], r["cls"], r["dfl"]])
    assert torch.isfinite(o).all()
    verr = ((o - ref).abs() / ref.abs().clamp_min(1e-3)).max().item()
    gerr = [((g.float().cpu().double() - rg).norm() / rg.norm().clamp_min(1e-30)).item() for g, rg in zip(grads, rgrads)]
    print(f"{name}: values {verr:.3g} scores {serr:.3g} grads {[f'{e:.3g}' for e in gerr]}")
    assert serr < vtol, (name, serr)
    assert verr < vtol, (name, o.tolist(), ref.tolist())
    assert max(gerr) < gtol, (name, gerr)
    return c, grads


@pytest.mark.parametrize("name", [n for n in C.CASES if n != "full640"])
def test_tal_vs_restatement(name):
    """composite: B = 3, nc = 5, (64, 96), levels (8,12) (4,6) (2,3) with an empty image, a GT without a
    candidate, two classes sharing anchors, the third-GT case, #inside < 10 and ignored rows; m0 / m1;
    nc 1 / 7 / 33 / 80; 1 and 4 levels; 5 anchors; topk 1 and other exponents; bf16 / f16 maps; 300
    and 5000 target rows (the kernels stage no target rows, so there is no row limit to straddle:
    these run the per-row grid and the contested anchors' scan of the whole list at both sizes);
    exact zero-metric ties."""
    c, grads = _compare(name)
    C_ = 64 + c["nc"]
    for g in grads:                       # padding channels of the NHWC buffer: zero gradient
        ld = g.stride(3)
        if ld != C_:
            base = torch.as_strided(g, (g.shape[0], g.shape[2], g.shape[3], ld), (g.stride(0), g.stride(2), ld, 1))
            assert (base[..., C_:] == 0).all()
    if name == "nc7_ld72":
        assert grads[0].stride(3) == 72
    if name == "composite":
        c_, r, _ = C.reference(name)
        assert int(r["gt"][C.THIRD_IMG, C.STAR]) == len(c_["targets"]) - 3     # what the kernel was just held to


def test_tal_640_full_grid_nc80():
    """The bench's anchor grid (8400 anchors, three levels), nc = 80, B = 2, 8 GTs per image."""
    _compare("full640", 5e-5, 5e-4)


@pytest.mark.parametrize("name", ["composite", "bf16"])
def test_tal_value_only_and_determinism(name):
    """need_grad=False gives the same values; two runs are bit-identical (values, gradients,
    assignment, scores)."""
    c = C.CASES[name]()
    a = _run(c)
    b = _run(c)
    v = _run(c, need_grad=False, assignment=False)
    assert v[1] is None and torch.equal(v[0], a[0])
    assert torch.equal(a[0], b[0]) and torch.equal(a[2][0], b[2][0]) and torch.equal(a[2][1], b[2][1])
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("gscale", [1.0, 2.5, 0.0])
def test_tal_backward_scales_by_incoming_grad(dtype, gscale):
    """(total * g).backward() equals the g = 1 gradients times g.to(dtype) bit for bit, padding
    channels included (yms_scale_by_device_scalar, as ComputeLoss's backward)."""
    c = C.CASES["nc7_ld72"]()
    tg = c["targets"].to(DEV)
    crit = TaskAlignedLoss(None, c["nc"], DEV, c["img"])
    ref_preds = [_channels_last(p, dtype).requires_grad_(True) for p in c["maps"]]
    crit.loss_tensor(ref_preds, tg)[0].backward()
    preds = [_channels_last(p, dtype).requires_grad_(True) for p in c["maps"]]
    total = crit.loss_tensor(preds, tg)[0]
    (total * gscale).backward()
    g = torch.tensor(gscale, device=DEV)
    for p, r in zip(preds, ref_preds):
        want = r.grad * g.to(dtype)
        assert p.grad.dtype == dtype and torch.equal(p.grad, want)


def test_tal_terms_not_differentiable_and_cpu_raises():
    c = C.CASES["nc7_ld72"]()
    preds = [_channels_last(p, torch.float32).requires_grad_(True) for p in c["maps"]]
    crit = TaskAlignedLoss(None, c["nc"], DEV, c["img"])
    total, terms = crit.loss_tensor(preds, c["targets"].to(DEV))
    assert terms.shape == (3,) and not terms.requires_grad
    with pytest.raises(RuntimeError):
        terms[0].backward()
    total.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in preds)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tal_loss(c["maps"], c["targets"], c["nc"], c["img"])


def test_task_aligned_loss_module_backward_through_model_and_compute_loss_unchanged():
    """TaskAlignedLoss on YOLOv8("n", 80) at 2 x 3 x 128 x 128 under bf16 autocast: backward reaches
    every parameter with finite values.  ComputeLoss on the same head maps gives the same bits before
    and after the new loss ran."""
    from yolov8.tools.loss import det_loss
    from yolov8.yolov8 import YOLOv8
    torch.manual_seed(0)
    m = YOLOv8("n", 80).to(DEV).train()
    crit = TaskAlignedLoss(m.head, 80, DEV, (128, 128))
    x = torch.randn(2, 3, 128, 128, device=DEV)
    # GTs of the size an untrained head predicts (DFL logits ~ 0: ~7.5 bins per side), so that the
    # overlaps, and with them the box and DFL terms' weights, are positive
    tg = torch.tensor([[0, 3, 0.5, 0.5, 0.8, 0.8], [0, 7, 0.45, 0.55, 0.7, 0.9], [1, 1, 0.5, 0.5, 0.9, 0.75],
                       [1, 60, 0.55, 0.5, 0.75, 0.8]], device=DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        outs = m(x)
    maps = [o.detach() for o in outs]
    before = det_loss(maps, tg, 80, (128, 128))
    loss, items = crit(outs, tg)
    assert set(items) == {"loss_box", "loss_cls", "loss_dfl", "total_loss"}
    print("items", items)
    assert items["loss_box"] > 0 and items["loss_dfl"] > 0
    assert abs(items["total_loss"] - 2 * (7.5 * items["loss_box"] + 0.5 * items["loss_cls"] +
                                          1.5 * items["loss_dfl"])) < 1e-4 * abs(items["total_loss"])
    loss.backward()
    named = [(k, p.grad) for k, p in m.named_parameters() if p.requires_grad]
    assert all(g is not None and torch.isfinite(g).all() for _, g in named)
    # the class term touches every anchor, so everything but the box branches (and the fixed DFL
    # projection) has a non-zero gradient; a level's box branch only where it holds foreground
    live = {k for k, g in named if float(g.abs().sum()) > 0}
    assert {k for k, _ in named if not k.startswith(("head.box", "head.dfl"))} <= live
    assert any(k.startswith("head.box") for k in live)
    after = det_loss(maps, tg, 80, (128, 128))
    assert torch.equal(before[0], after[0])
    for a, b in zip(before[1], after[1]):
        assert torch.equal(a, b)
