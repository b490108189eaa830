"""csrc/det_loss.hip at its assignment and gradient edges, through yolov8.tools.loss.det_loss, against
the fp64 oracle (oracle/loss_ref.py) on the dtype-rounded maps.  The inputs come from
tests/loss_cases.py; tests/test_loss_cases_cpu.py shows on the CPU that each has the property it is
named for (target counts past assign_kernel's 256-row staging round and its 4096-row LDS list, exact
top-k ties across the cut, DFL targets below 0 / at or above 15 / integer, ...).

Every comparison runs once per loss term -- det_loss with lambdas (1,0,0), (0,1,0), (0,0,1) against
the oracle's loss_box / loss_cls / loss_dfl backward, and the default weights against the total --
and per (image, level) block of DFL lanes and of class lanes, so a wrong small term (CIoU's alpha v,
the DFL two-bin term, one image's factor 2 or 1 / n_fg) cannot hide under another term's or another
image's norm:

  * the foreground set (anchors with a non-zero DFL-lane gradient) equals the oracle's, per image;
  * per block, max|g - r| <= GTOL * max|r| of that block; a block whose reference is all zero is all
    zero (background DFL lanes are therefore exactly 0);
  * each loss value within VTOL of the oracle's, relative (floor 1e-3 as in tests/test_loss_gpu.py).

GTOL is the project's: fp32 2e-4; bf16 4e-3 = 2 x the 2^-9 half-ulp of the stored gradient; f16
1e-3 = 2 x 2^-11 by the same rule.  That rule is about normal numbers: below 2^-14 an f16 gradient
is stored with the absolute spacing 2^-24 whatever its size (B = 260 images at 1 / (B n_fg) per
anchor get there), so an f16 block is allowed max(GTOL * max|r|, 2^-24) = 2 x the half-spacing 2^-25
-- the same rule, and only blocks whose largest reference element is itself subnormal are affected
(2^-24 / 1e-3 ~ 2^-14).  fp32 and bf16 subnormals (< 1e-38) are never reached.  VTOL is 2e-5 (1e-4
for the 16-bit maps).  Row order, ignored rows, buffer layout, need_grad and repetition must not
change one bit.
"""
import pytest
import torch

import loss_cases as C
from yms import _lib as L
from yolov8.tools.loss import det_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
IOUS = ["ciou", "giou", "diou", "iou"]
GTOL = {F32: 2e-4, BF16: 4e-3, F16: 1e-3}
VTOL = {F32: 2e-5, BF16: 1e-4, F16: 1e-4}
GFLOOR = {F32: 0.0, BF16: 0.0, F16: 2.0 ** -24}       # the stored gradient's subnormal spacing (docstring)


def _channels_last(p, dtype):
    """NCHW-shaped channels-last view of a tightly packed NHWC buffer."""
    return p.to(DEV, dtype).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _wide(p, dtype, extra=24):
    """The same map as a slot of a wider NHWC buffer: lanes [C, r8(C)) zero, foreign NaNs beyond."""
    B, Cc, H, W = p.shape
    r8 = (Cc + 7) // 8 * 8
    buf = torch.full((B, H, W, r8 + extra), float("nan"), dtype=dtype, device=DEV)
    buf[..., :Cc] = p.to(DEV, dtype).permute(0, 2, 3, 1)
    buf[..., Cc:r8] = 0
    return buf[..., :Cc].permute(0, 3, 1, 2)


def _run(case, dtype, lambdas=C.TERMS["total"], iou_type="ciou", pos_weight=None, need_grad=True, targets=None,
         view=_channels_last):
    preds = [view(m, dtype) for m in case["maps"]]
    tg = case["targets"] if targets is None else targets
    # whatever the kernels read from their workspace they must have written: hand the allocator
    # blocks of the workspace's size full of 0xff (NaN as float, -1 as int) to give back
    A = sum(m.shape[2] * m.shape[3] for m in case["maps"])
    nbytes = L.lib().yms_det_loss_ws_bytes(case["maps"][0].shape[0], A, case["nc"], tg.shape[0])
    poison = [torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV) for _ in range(4)]
    del poison
    return det_loss(preds, tg.to(DEV), case["nc"], case["img"], case["strides"], iou_type=iou_type,
                    pos_weight=pos_weight, lambdas=lambdas, need_grad=need_grad)


def _same(a, b):
    return torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


_REFS = {}


def _reference(key, case, dtype, iou_type="ciou", pos_weight=None):
    k = (key, dtype, iou_type)
    if k not in _REFS:
        _REFS[k] = C.reference(case, dtype, iou_type, pos_weight)
    return _REFS[k]


def _check(key, case, dtype, iou_type="ciou", pos_weight=None, view=_channels_last):
    """Every term of det_loss against the oracle: values, foreground sets, per-block gradients."""
    ref = _reference(key, case, dtype, iou_type, pos_weight)
    gtol, vtol = GTOL[dtype], VTOL[dtype]
    want_fg = ref["fg"]
    runs = {}
    for term, lam in C.TERMS.items():
        out, grads = runs[term] = _run(case, dtype, lam, iou_type, pos_weight, view=view)
        o = out.cpu().double()
        assert torch.isfinite(o).all(), (term, o.tolist())
        v = ref["values"]
        want = torch.tensor([sum(w * v[n] for w, n in zip(lam, ("loss_box", "loss_cls", "loss_dfl"))),
                             v["loss_box"], v["loss_cls"], v["loss_dfl"]], dtype=torch.float64)
        verr = ((o - want).abs() / want.abs().clamp_min(1e-3)).max().item()
        gs = [g.float().cpu().double() for g in grads]
        assert all(torch.isfinite(g).all() for g in gs), term
        worst = 0.0
        for lvl, (g, r) in enumerate(zip(gs, ref["grads"][term])):
            for kind, gb, rb in zip(("dfl", "cls"), C.grad_blocks(g), C.grad_blocks(r)):
                err, top = (gb - rb).abs().amax(1), rb.abs().amax(1)
                zero = top == 0
                assert not gb[zero].any(), (term, lvl, kind, "gradient where the oracle has none")
                ratio = (err[~zero] / top[~zero])
                if ratio.numel():
                    worst = max(worst, ratio.max().item())
                bad = torch.nonzero((err > (gtol * top).clamp_min(GFLOOR[dtype])) & ~zero).flatten().tolist()
                assert not bad, (term, "level", lvl, kind, "images", bad[:8], (err / top)[bad[:8]].tolist(), gtol)
        print(f"{key} {dtype} {iou_type} {term}: value err {verr:.2e} (tol {vtol:.0e}), "
              f"worst block {worst:.2e} (tol {gtol:.0e})")
        assert verr < vtol, (term, o.tolist(), want.tolist())
        if term != "loss_cls":          # foreground = anchors with any non-zero DFL-lane gradient
            B = gs[0].shape[0]
            got_fg = torch.cat([(g[:, :4 * C.DFL] != 0).any(1).reshape(B, -1) for g in gs], 1)
            assert torch.equal(got_fg, want_fg), (term, torch.nonzero(got_fg != want_fg).tolist()[:8])
    return runs


def _pruned(case, dtype):
    case, dropped = C.pruned(case, dtype)
    assert dropped == 0
    return case


# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [300, 4300])
def test_many_targets(n, dtype):
    """Two staging rounds of assign_kernel's compaction (300 rows) and its unstaged scan (> 4096)."""
    case, dropped = C.many_pruned(n, dtype)
    assert dropped <= 0.02 * n and case["targets"].shape[0] > (256 if n == 300 else 4096)
    _check(f"many{n}", case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("iou_type", IOUS[1:])
def test_many_targets_iou_types(iou_type, dtype):
    _check("many300", C.many_pruned(300, dtype)[0], dtype, iou_type)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,M", [(300, 256), (4300, 4096)])
def test_ignored_rows_change_nothing(n, M, dtype):
    """Rows of no image of the batch (ids B, B + 7, -1) move M across a staging round (256 -> 257)
    and across the LDS list (4096 -> 4097, the unstaged scan): bit-identical results."""
    case = C.many_pruned(n, dtype)[0]
    tg = case["targets"][:M]
    assert tg.shape[0] == M
    base = _run(case, dtype, targets=tg)
    B = case["maps"][0].shape[0]
    extra = [[i, 1, 0.5, 0.5, 0.3, 0.3] for i in (B, B + 7, -1)]
    for rows in ([extra[0]], [extra[1]], [extra[2]], extra):
        assert _same(base, _run(case, dtype, targets=torch.cat([tg, torch.tensor(rows)])))
    # in front and in the middle as well: the image's own order is what counts
    mixed = torch.cat([torch.tensor(extra[:1]), tg[:100], torch.tensor(extra[1:]), tg[100:]])
    assert _same(base, _run(case, dtype, targets=mixed))


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_permutation_across_images_changes_nothing(dtype):
    """Only the order of the rows inside one image carries meaning."""
    case = C.many_pruned(300, dtype)[0]
    tg = case["targets"]
    base = _run(case, dtype)
    by_image = tg[torch.sort(tg[:, 0], stable=True).indices]
    assert not torch.equal(by_image, tg)
    assert _same(base, _run(case, dtype, targets=by_image))
    backwards = torch.cat([tg[tg[:, 0] == b] for b in (2, 1, 0)])
    assert _same(base, _run(case, dtype, targets=backwards))


@pytest.mark.parametrize("dtype", DTYPES)
def test_swapping_anchor_sharing_gts_follows_the_oracle(dtype):
    """The later GT's box wins the shared anchors: swapping the two changes the result, and both
    orders match the oracle."""
    case = _pruned(C.swap_case(), dtype)
    tg = case["targets"]
    M = tg.shape[0]
    swapped = dict(case, targets=tg[list(range(M - 2)) + [M - 1, M - 2]])
    a = _check("swap", case, dtype)["total"]
    b = _check("swapped", swapped, dtype)["total"]
    assert not torch.equal(a[0], b[0]) and not all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale", [1, 2])
def test_topk_ties_go_to_the_lower_anchor(scale, dtype):
    """Bit-equal IoUs across the rank 10 / 11 cut: between lanes of a wave (scale 1 and 2), between
    waves and between the two anchors of one top-k thread (scale 2).  The all-zero DFL logits are
    exact in every dtype."""
    _check(f"tie{scale}", C.tie_case(scale), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("iou_type", IOUS)
def test_dfl_bin_edges(iou_type, dtype):
    """Side targets below 0 (both bins 0), at or above 15 (both bins 15) and integer (right weight 0)."""
    case = C.dfl_edge_case()
    neg, hi, integer = C.dfl_side_conditions(case, dtype)
    assert neg and hi and integer
    _check("dfl_edges", _pruned(case, dtype), dtype, iou_type)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [65, 260])
def test_many_images_few_anchors(B, dtype):
    """More images than one flags_kernel block (64) and than finalize_kernel's threads (256); five
    anchors in all (k < 10 for want of anchors, idle top-k threads), images without GT."""
    _check(f"batch{B}", _pruned(C.batch_case(B), dtype), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nl", [1, 4])
def test_level_counts(nl, dtype):
    _check(f"levels{nl}", _pruned(C.levels_case(nl), dtype), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nc", [1, 33, 80])
def test_class_counts(nc, dtype):
    """nc = 1; two class words with a last 8-chunk one class wide and one box carrying classes 2 and
    32; classes 31 / 32 / 79 on shared anchors."""
    _check(f"classes{nc}", _pruned(C.classes_case(nc), dtype), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pos_weight_across_class_words(dtype):
    _check("classes33pw", _pruned(C.classes_case(33), dtype), dtype, pos_weight=torch.linspace(0.5, 3.0, 33))


@pytest.mark.parametrize("dtype", DTYPES)
def test_saturated_logits(dtype):
    """Class logits of +-50, one DFL bin per side 40 above the rest: finite and equal to the oracle."""
    _check("saturated", _pruned(C.saturated_case(), dtype), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_slot_of_a_wider_buffer(dtype):
    """Maps given as channels-last views into a buffer 24 lanes wider than round_up(64 + nc, 8), NaN
    in the foreign lanes: bit-identical to the tightly packed call, the input untouched, and the
    gradient buffers exactly zero in every lane >= 64 + nc."""
    case = C.many_pruned(300, dtype)[0]
    Cc = 4 * C.DFL + case["nc"]
    r8 = (Cc + 7) // 8 * 8
    packed = _run(case, dtype)
    preds = [_wide(m, dtype) for m in case["maps"]]
    before = [p._base.clone() for p in preds]
    wide = det_loss(preds, case["targets"].to(DEV), case["nc"], case["img"], case["strides"])
    assert _same(packed, wide)
    for p, b in zip(preds, before):
        assert p.stride(3) == r8 + 24 and torch.isnan(p._base[..., r8:]).all()
        assert torch.equal(p._base[..., :r8], b[..., :r8])
    for ld, grads in ((r8, packed[1]), (r8 + 24, wide[1])):
        for g in grads:
            assert g._base.shape[-1] == ld and not g._base[..., Cc:].any()
    _check("many300", case, dtype, view=_wide)


@pytest.mark.parametrize("dtype", DTYPES)
def test_value_only_and_repeatable(dtype):
    """need_grad=False returns the same four values, and a second run the same bits."""
    case = C.many_pruned(300, dtype)[0]
    first = _run(case, dtype)
    assert _same(first, _run(case, dtype))
    out, grads = _run(case, dtype, need_grad=False)
    assert grads is None and torch.equal(out, first[0])
