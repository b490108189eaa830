"""The dynamic soft-label loss kernels (csrc/dsl_loss.hip via yolov8.tools.dsl_loss) against the
restatement tests/dsl_ref.py on the seeded inputs of tests/dsl_cases.py: the assignment and every
dynamic k exactly (tests/test_dsl_cpu.py asserts that every decision of the restatement on these inputs
has a margin above 1e-4 relative, every IoU sum one above 1e-3 from an integer, or is an exact tie built
on purpose), the soft labels, the five values and the per-level gradient.

Tolerances are the project's loss tolerances (tests/test_tal_gpu.py): values 2e-5 relative (floor
1e-3), gradients 2e-4 relative L2 per level for fp32 maps; 1e-4 / 4e-3 for bf16 / f16 maps (both
sides see the rounded maps; the gradient is stored in the 16-bit type, half-ulp 2^-9 per element);
5e-5 / 5e-4 on the full 640 grid.  The restatement evaluated in fp32 on the CPU differs from its
fp64 self by at most 2.4e-7 (values), 1.9e-7 (gradients) and 5.1e-7 (soft labels, relative to the
largest) over these cases, so every tolerance is more than 10x the restatement's own rounding and
stands as it is.  Soft labels are held to the value tolerance relative to the largest label."""
import ctypes

import pytest
import torch

import dsl_cases as C
from yolov8.tools.dsl_loss import DynamicSoftLabelLoss, dsl_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"

TOL = {torch.float32: (2e-5, 2e-4), torch.bfloat16: (1e-4, 4e-3), torch.float16: (1e-4, 4e-3)}


def _channels_last(p, dtype):
    """NCHW-shaped channels-last view of an NHWC buffer, like the plan's head outputs."""
    return p.to(DEV, dtype).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _run(c, need_grad=True, assignment=True):
    preds = [_channels_last(m, c["dtype"]) for m in c["maps"]]
    return dsl_loss(preds, c["targets"].to(DEV), c["nc"], c["img"], c["strides"], c["topk"], c["radius"],
                    c["iou_weight"], c["beta"], c["gains"], need_grad=need_grad, return_assignment=assignment)


def _compare(name, vtol=None, gtol=None):
    c, r, rgrads = C.reference(name)
    tv, tg = TOL[c["dtype"]]
    vtol, gtol = vtol or tv, gtol or tg
    out, grads, (agt, asc, dk) = _run(c)
    B = c["maps"][0].shape[0]
    assert agt.shape == (B, r["gt"].shape[1]) and torch.equal(agt.cpu().long(), r["gt"]), name
    assert torch.equal(dk.cpu().long(), r["k"]), (name, dk.tolist(), r["k"].tolist())
    serr = ((asc.cpu().double() - r["t"]).abs().max() / r["t"].max().clamp_min(1e-30)).item()
    o = out.cpu().double()
    ref = torch.stack([r["total"], r["box"], r["cls"], r["dfl"], r["norm"]])
    assert o.shape == (5,) and torch.isfinite(o).all()
    verr = ((o - ref).abs() / ref.abs().clamp_min(1e-3)).max().item()
    gerr = [((g.float().cpu().double() - rg).norm() / rg.norm().clamp_min(1e-30)).item() for g, rg in zip(grads, rgrads)]
    print(f"{name}: values {verr:.3g} labels {serr:.3g} grads {[f'{e:.3g}' for e in gerr]}")
    assert serr < vtol, (name, serr)
    assert verr < vtol, (name, o.tolist(), ref.tolist())
    assert max(gerr) < gtol, (name, gerr)
    return c, grads


@pytest.mark.parametrize("name", [n for n in C.CASES if n != "full640"])
def test_dsl_vs_restatement(name):
    """composite: B = 3, nc = 5, (64, 96), levels (8,12) (4,6) (2,3) with an empty image, a GT without a
    centre that still selects, two classes sharing anchors, ignored rows and a contested anchor whose
    winner had not selected it; m0 / m1; nc 1 / 7 / 33 / 80; 1 and 4 levels; 5 anchors (fewer candidates
    than topk); topk 1; radius 1, iou_weight 1, beta 1; beta 3; dfl gain 1.5; bf16 / f16 maps; 300 and
    5000 target rows (no row limit to straddle); the saturated-prior ties."""
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
        assert int(r["gt"][C.WIN_IMG, C.STAR]) == len(c_["targets"]) - 3       # what the kernel was just held to


def test_dsl_640_full_grid_nc80():
    """The bench's anchor grid (8400 anchors, three levels), nc = 80, B = 2, 8 GTs per image."""
    _compare("full640", 5e-5, 5e-4)


@pytest.mark.parametrize("name", ["composite", "bf16"])
def test_dsl_value_only_and_determinism(name):
    """need_grad=False gives the same values; two runs are bit-identical (values, gradients,
    assignment, labels, dynamic k)."""
    c = C.CASES[name]()
    a = _run(c)
    b = _run(c)
    v = _run(c, need_grad=False, assignment=False)
    assert v[1] is None and torch.equal(v[0], a[0])
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", ["composite", "bf16", "m0"])
def test_dsl_workspace_independence(name):
    """yms_dsl_loss called directly with the workspace pre-filled with 0x00 and then 0xFF bytes: every
    output is bit-identical, so no result depends on workspace memory the call did not write itself."""
    from yms import _lib as L
    c = C.CASES[name]()
    dt = c["dtype"]
    nc, n = c["nc"], len(c["maps"])
    Cn = 64 + nc
    ld = (Cn + 7) // 8 * 8
    maps = []
    for m in c["maps"]:
        t = torch.zeros((m.shape[0], m.shape[2], m.shape[3], ld), dtype=dt, device=DEV)
        t[..., :Cn] = m.to(DEV, dt).permute(0, 2, 3, 1)
        maps.append(t)
    B = maps[0].shape[0]
    hs, ws = [m.shape[1] for m in maps], [m.shape[2] for m in maps]
    A = sum(h * w for h, w in zip(hs, ws))
    tg = c["targets"].to(DEV, torch.float32).reshape(-1, 6).contiguous()
    M = tg.shape[0]
    wsb = L.lib().yms_dsl_loss_ws_bytes(B, A, nc, M)
    results = []
    for fill in (0x00, 0xFF):
        ws_t = torch.full((wsb,), fill, dtype=torch.uint8, device=DEV)
        grads = [torch.zeros_like(m) for m in maps]
        out = torch.full((5,), float("nan"), device=DEV)
        agt = torch.full((B, A), -7, dtype=torch.int32, device=DEV)
        asc = torch.full((B, A), float("nan"), device=DEV)
        dk = torch.full((max(M, 1),), -7, dtype=torch.int32, device=DEV)
        L.call("yms_dsl_loss", L.dtype_code(dt), B, nc, n, (ctypes.c_void_p * n)(*[m.data_ptr() for m in maps]),
               (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads]), (ctypes.c_int * n)(*hs), (ctypes.c_int * n)(*ws),
               (ctypes.c_float * n)(*c["strides"]), ld, tg.data_ptr() if M else None, M,
               ctypes.c_float(float(c["img"][1])), ctypes.c_float(float(c["img"][0])), c["topk"],
               ctypes.c_float(c["radius"]), ctypes.c_float(c["iou_weight"]), ctypes.c_float(c["beta"]),
               (ctypes.c_float * 3)(*c["gains"]), ws_t.data_ptr(), wsb, out.data_ptr(), agt.data_ptr(), asc.data_ptr(),
               dk.data_ptr(), L.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        results.append([out, agt, asc, dk[:M]] + grads)
    for x, y in zip(*results):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert torch.isfinite(results[0][0]).all() and (results[0][1] >= -1).all() and (results[0][3] >= 0).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("gscale", [1.0, 2.5, 0.0])
def test_dsl_backward_scales_by_incoming_grad(dtype, gscale):
    """(total * g).backward() equals the g = 1 gradients times g.to(dtype) bit for bit, padding
    channels included (yms_scale_by_device_scalar, as ComputeLoss's backward)."""
    c = C.CASES["nc7_ld72"]()
    tg = c["targets"].to(DEV)
    crit = DynamicSoftLabelLoss(None, c["nc"], DEV, c["img"])
    ref_preds = [_channels_last(p, dtype).requires_grad_(True) for p in c["maps"]]
    crit.loss_tensor(ref_preds, tg)[0].backward()
    preds = [_channels_last(p, dtype).requires_grad_(True) for p in c["maps"]]
    total = crit.loss_tensor(preds, tg)[0]
    (total * gscale).backward()
    g = torch.tensor(gscale, device=DEV)
    for p, r in zip(preds, ref_preds):
        want = r.grad * g.to(dtype)
        assert p.grad.dtype == dtype and torch.equal(p.grad, want)


def test_dsl_terms_not_differentiable_and_cpu_raises():
    c = C.CASES["nc7_ld72"]()
    preds = [_channels_last(p, torch.float32).requires_grad_(True) for p in c["maps"]]
    crit = DynamicSoftLabelLoss(None, c["nc"], DEV, c["img"])
    total, terms = crit.loss_tensor(preds, c["targets"].to(DEV))
    assert terms.shape == (3,) and not terms.requires_grad
    with pytest.raises(RuntimeError):
        terms[0].backward()
    total.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in preds)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dsl_loss(c["maps"], c["targets"], c["nc"], c["img"])


def test_dynamic_soft_label_loss_module_backward_through_model_and_other_losses_unchanged():
    """DynamicSoftLabelLoss on YOLOv8("n", 80) at 2 x 3 x 128 x 128 under bf16 autocast: backward reaches
    every parameter with finite values and loss_box > 0.  det_loss and tal_loss on the same head maps
    give the same bits before and after the new loss ran."""
    from yolov8.tools.loss import det_loss
    from yolov8.tools.tal_loss import tal_loss
    from yolov8.yolov8 import YOLOv8
    torch.manual_seed(0)
    m = YOLOv8("n", 80).to(DEV).train()
    crit = DynamicSoftLabelLoss(m.head, 80, DEV, (128, 128))
    x = torch.randn(2, 3, 128, 128, device=DEV)
    # GTs of the size an untrained head predicts (DFL logits ~ 0: ~7.5 bins per side), so that the IoUs,
    # and with them the box term's weights, are positive
    tg = torch.tensor([[0, 3, 0.5, 0.5, 0.8, 0.8], [0, 7, 0.45, 0.55, 0.7, 0.9], [1, 1, 0.5, 0.5, 0.9, 0.75],
                       [1, 60, 0.55, 0.5, 0.75, 0.8]], device=DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        outs = m(x)
    maps = [o.detach() for o in outs]
    before = det_loss(maps, tg, 80, (128, 128)), tal_loss(maps, tg, 80, (128, 128))
    loss, items = crit(outs, tg)
    assert set(items) == {"loss_box", "loss_cls", "loss_dfl", "total_loss"}
    print("items", items)
    assert items["loss_box"] > 0 and items["loss_dfl"] > 0
    assert abs(items["total_loss"] - (2 * items["loss_box"] + items["loss_cls"])) < 1e-4 * abs(items["total_loss"])
    loss.backward()
    named = [(k, p.grad) for k, p in m.named_parameters() if p.requires_grad]
    assert all(g is not None and torch.isfinite(g).all() for _, g in named)
    # the class term touches every anchor, so everything but the box branches (and the fixed DFL
    # projection) has a non-zero gradient; a level's box branch only where it holds foreground
    live = {k for k, g in named if float(g.abs().sum()) > 0}
    assert {k for k, _ in named if not k.startswith(("head.box", "head.dfl"))} <= live
    assert any(k.startswith("head.box") for k in live)
    after = det_loss(maps, tg, 80, (128, 128)), tal_loss(maps, tg, 80, (128, 128))
    for bf, af in zip(before, after):
        assert torch.equal(bf[0], af[0])
        for a, b in zip(bf[1], af[1]):
            assert torch.equal(a, b)
