"""The inputs of tests/test_loss_edges_gpu.py meet the conditions they were built for -- checked with
the fp64 oracle alone (oracle/loss_ref.py), no GPU: the pruned share, the target counts on both sides
of assign_kernel's 256-row staging round and 4096-row LDS list, interleaved images, anchor-sharing
GTs, top-k ties across the cut with exact arithmetic, and the DFL bin edges among the foreground."""
import pytest
import torch

import loss_cases as C
from oracle import loss_ref as R

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _sets(case, dtype):
    return C.chosen_sets(C.rounded(case["maps"], dtype), case["targets"].double(), case["img"], case["strides"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,floor", [(300, 256), (4300, 4096)])
def test_many_cases_after_pruning(n, floor, dtype):
    case, dropped = C.many_pruned(n, dtype)
    tg = case["targets"]
    assert dropped <= 0.02 * n, dropped                  # the margin is a condition on the inputs, not a filter
    assert tg.shape[0] > floor                           # past the staging round / the LDS list
    ids = tg[:, 0].int()
    assert set(ids.tolist()) == {0, 1, 2}
    assert int((ids[1:] != ids[:-1]).sum()) > tg.shape[0] // 2      # rows of different images interleave
    # what pruning promises: every kept row is at least the margin away from another assignment
    _, again = C.prune_ambiguous(C.rounded(case["maps"], dtype), tg, case["img"], case["strides"])
    assert again == 0
    ch = _sets(case, dtype)
    rows0 = C.image_rows(tg, 0).tolist()
    assert any(set(ch[i]) & set(ch[j]) for i in rows0[:20] for j in rows0[:20] if i < j)   # shared anchors
    assert any(len(s) == R.TOPK for s in ch.values()) and any(len(s) < R.TOPK for s in ch.values())


def test_prune_ambiguous_drops_a_row_on_the_boundary():
    """A GT whose 10th and 11th IoUs are equal (the tie case's second GT) has distance 0 and is
    dropped; the others stay, and a row of no image of the batch is kept."""
    case = C.tie_case()
    tg = torch.cat([case["targets"], torch.tensor([[5, 0, 0.5, 0.5, 0.2, 0.2], [-1, 0, 0.5, 0.5, 0.2, 0.2]])])
    kept, dropped = C.prune_ambiguous(C.rounded(case["maps"], torch.float32), tg, case["img"], case["strides"])
    assert dropped == 1 and torch.equal(kept, tg[[0, 2, 3, 4]])


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_cases_need_no_pruning(dtype):
    """The constructed cases keep every row (so the row each was built around is still there)."""
    cases = [C.swap_case(), C.dfl_edge_case(), C.batch_case(65), C.batch_case(260), C.levels_case(1),
             C.levels_case(4), C.classes_case(1), C.classes_case(33), C.classes_case(80), C.saturated_case()]
    for case in cases:
        assert C.pruned(case, dtype)[1] == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_swap_case_shares_anchors_in_its_last_rows(dtype):
    case = C.swap_case()
    ch = _sets(case, dtype)
    M = case["targets"].shape[0]
    assert case["targets"][M - 2, 0] == case["targets"][M - 1, 0] == 0
    assert case["targets"][M - 2, 1] != case["targets"][M - 1, 1]
    assert set(ch[M - 2]) & set(ch[M - 1])
    assert not torch.equal(case["targets"][M - 2, 2:], case["targets"][M - 1, 2:])   # the overwrite is visible


@pytest.mark.parametrize("scale", [1, 2])
def test_tie_case_is_exact_and_straddles_the_cut(scale):
    case = C.tie_case(scale)
    img, strides, tg = case["img"], case["strides"], case["targets"]
    m32 = [m.float() for m in case["maps"]]
    m64 = [m.double() for m in case["maps"]]
    pb32, _, _ = C.decoded(m32, strides)
    pb64, anc, _ = C.decoded(m64, strides)
    assert torch.equal(pb32.double(), pb64)                         # 15 x 15 boxes, exactly, in both
    assert torch.equal(pb64[0, :, 2:], torch.full((anc.shape[0], 2), 15.0, dtype=torch.float64))
    g = C.gt_boxes(tg.double(), torch.arange(tg.shape[0]), img, torch.float64)
    ge = torch.cat([g[:, :2] - g[:, 2:] / 2, g[:, :2] + g[:, 2:] / 2], 1)
    pe = torch.cat([pb64[0, :, :2] - 7.5, pb64[0, :, :2] + 7.5], 1)
    assert torch.equal(ge, ge.round()) and torch.equal(pe - pe.floor(), torch.full_like(pe, 0.5))
    # so no GT edge equals a predicted edge (where torch splits the min / max gradient and the kernel does not)
    assert not (ge[:, None, 0::2, None] == pe[None, :, None, 0::2]).any()
    assert not (ge[:, None, 1::2, None] == pe[None, :, None, 1::2]).any()
    # the same chosen sets from the fp32 and the fp64 oracle
    ch32 = C.chosen_sets(m32, tg.float(), img, strides)
    ch64 = C.chosen_sets(m64, tg.double(), img, strides)
    assert ch32 == ch64
    # at least one GT whose tied group straddles the k cut, in both precisions
    for maps, t in ((m32, tg.float()), (m64, tg.double())):
        cuts = [C.tied_at_cut(col) for col in C.row_ious(maps, t, img, strides).values()]
        assert any(inside and outside for inside, outside in cuts), cuts
    if scale == 1:      # the issue's hand-checked row: eight anchors tied, 19 and 20 chosen
        inside, outside = C.tied_at_cut(C.row_ious(m64, tg.double(), img, strides)[1])
        assert inside == [19, 20] and len(inside) + len(outside) == 8
    if scale == 2:      # ... and one tie inside a single top-k thread (anchors a and a + 256)
        inside, outside = C.tied_at_cut(C.row_ious(m64, tg.double(), img, strides)[3])
        assert (inside, outside) == ([17], [273])
        # ... and one between waves of the block (anchors 0-63 / 64-127 of the first 256)
        inside, outside = C.tied_at_cut(C.row_ious(m64, tg.double(), img, strides)[0])
        assert max(inside) < 64 <= max(outside) < 256
    # nothing near the IoU threshold either
    for col in C.row_ious(m64, tg.double(), img, strides).values():
        assert (col - R.IOU_MIN).abs().min() > 1e-3


@pytest.mark.parametrize("dtype", DTYPES)
def test_dfl_edge_case_has_all_three_side_conditions(dtype):
    neg, hi, integer = C.dfl_side_conditions(C.dfl_edge_case(), dtype)
    assert neg >= 1 and hi >= 1 and integer >= 1, (neg, hi, integer)


@pytest.mark.parametrize("B", [65, 260])
def test_batch_case_shape(B):
    case = C.batch_case(B)
    assert sum(m.shape[2] * m.shape[3] for m in case["maps"]) == 5          # fewer than 10 anchors in all
    ids = set(case["targets"][:, 0].int().tolist())
    assert max(ids) >= B - 3 and 0 < B - len(ids) < B // 2                   # some images have no GT
    ref = C.reference(case, torch.float32)
    nfg = ref["fg"].sum(1)
    assert (nfg[64:] > 0).any() and (nfg == 0).any() and int(nfg.max()) == 5
    if B > 256:
        assert (nfg[256:] > 0).any()                                         # finalize_kernel's second pass


def test_classes_cases_cross_the_class_words():
    for nc, labs in ((33, [2, 32]), (80, [31, 32, 79])):
        case = C.classes_case(nc)
        a = C.assignment(C.rounded(case["maps"], torch.float32), case["targets"].double(), nc, case["img"],
                         case["strides"])
        ts = a[1][2]
        assert (ts[:, labs].sum(1) == len(labs)).any()           # one anchor carries all of them


def test_reference_terms_add_up():
    """reference(): the per-term gradients combine to the total's with the loss weights."""
    ref = C.reference(C.swap_case(), torch.float32)
    v = ref["values"]
    assert abs(v["total"] - (7.5 * v["loss_box"] + 0.5 * v["loss_cls"] + 1.5 * v["loss_dfl"])) < 1e-12
    for lvl in range(3):
        s = 7.5 * ref["grads"]["loss_box"][lvl] + 0.5 * ref["grads"]["loss_cls"][lvl] + \
            1.5 * ref["grads"]["loss_dfl"][lvl]
        assert torch.allclose(s, ref["grads"]["total"][lvl], rtol=1e-12, atol=1e-15)
        dfl, cls = C.grad_blocks(ref["grads"]["loss_cls"][lvl])
        assert not dfl.any() and cls.all()                       # BCE touches the class lanes only, all of them
        dfl, cls = C.grad_blocks(ref["grads"]["loss_dfl"][lvl])
        assert dfl.any() and not cls.any()
