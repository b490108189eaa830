"""Pins tests/dsl_ref.py, the plain-torch restatement that defines YOLO-MS's own loss
(yolov8.tools.dsl_loss, csrc/dsl_loss.hip: dynamic soft-label assigner, QFL, GIoU), to a case worked
by hand and to the assigner's edge rules, and checks the condition under which an fp32 kernel can be
asked for the exact assignment: the margins of every seeded input of tests/dsl_cases.py."""
import ctypes
import math

import pytest
import torch

import dsl_cases as C
import dsl_ref as R

EPS = 1e-7


def _iou(p, g, giou=False):
    """scalar IoU / GIoU of xyxy boxes, written out independently of dsl_ref"""
    iw = max(min(p[2], g[2]) - max(p[0], g[0]), 0.0)
    ih = max(min(p[3], g[3]) - max(p[1], g[1]), 0.0)
    inter = iw * ih
    un = (p[2] - p[0]) * (p[3] - p[1]) + (g[2] - g[0]) * (g[3] - g[1]) - inter + EPS
    if not giou:
        return inter / un
    ca = (max(p[2], g[2]) - min(p[0], g[0])) * (max(p[3], g[3]) - min(p[1], g[1])) + EPS
    return inter / un - (ca - un) / ca


def _sig(x):
    return 1 / (1 + math.exp(-x))


def _qfl(x, y, beta=2.0):
    bce = (1 - y) * x + math.log1p(math.exp(-abs(x))) + max(-x, 0.0)
    return bce * abs(y - _sig(x)) ** beta


def _cost(logits, cls, iou, centre, gtc, stride=8.0, radius=3.0, w=3.0):
    c = sum(_qfl(x, iou if k == cls else 0.0) for k, x in enumerate(logits))
    d = math.hypot(centre[0] - gtc[0], centre[1] - gtc[1])
    return c - math.log(iou + EPS) * w + 10.0 ** min(d / stride - radius, 30.0)


HAND_BOXES = [(0, 0, 16, 8), (4, 0, 16, 8), (0, 0, 8, 16), (8, 8, 16, 16)]
HAND_LOGITS = [(1.0, -1.0), (0.0, 0.0), (2.0, 4.0), (-2.0, -2.0)]
HAND_CENTRES = [(4, 4), (12, 4), (4, 12), (12, 12)]
HAND_GTS = [(0, (0, 0, 16, 8)), (1, (0, 0, 16, 16))]


def _hand_case():
    m = torch.zeros(1, 66, 2, 2, dtype=torch.float64)
    # per anchor the sides (left, top, right, bottom) in bins of 8 px: x.5 = two-hot bins x | x + 1, 1.0 = one-hot
    sides = {(0, 0): (0.5, 0.5, 1.5, 0.5), (0, 1): (1.0, 0.5, 0.5, 0.5), (1, 0): (0.5, 1.5, 0.5, 0.5),
             (1, 1): (0.5, 0.5, 0.5, 0.5)}
    for (y, x), ss in sides.items():
        for side, v in enumerate(ss):
            lo = int(math.floor(v))
            m[0, side * 16 + lo, y, x] = 50.0
            if v != lo:
                m[0, side * 16 + lo + 1, y, x] = 50.0
        c0, c1 = HAND_LOGITS[y * 2 + x]
        m[0, 64, y, x] = c0
        m[0, 65, y, x] = c1
    tg = torch.tensor([[0, 0, 0.5, 0.25, 1.0, 0.5], [0, 1, 0.5, 0.5, 1.0, 1.0]], dtype=torch.float64)
    return m, tg


def test_hand_worked_case():
    """One level, 2 x 2 anchors of stride 8 on a 16 x 16 image, nc = 2, defaults (topk 13, radius 3,
    iou_weight 3, beta 2, gains 2 / 1 / 0).

    Anchors a0..a3 have centres (4,4), (12,4), (4,12), (12,12).  DFL logits are two-hot (50 at two
    neighbouring bins: x.5 bins) or one-hot (a1's left side: 1 bin; the other bins leak ~1e-21).
    Predicted boxes: a0 (0,0,16,8), a1 (4,0,16,8), a2 (0,0,8,16), a3 (8,8,16,16).  Class logits
    (class 0, class 1): a0 (1,-1), a1 (0,0), a2 (2,4), a3 (-2,-2).

    GT0 = class 0, box (0,0,16,8), centre (8,4); GT1 = class 1, the whole image, centre (8,8).  GT1
    contains every centre, so all four anchors are candidates of BOTH GTs (a2, a3 lie outside GT0).
      IoU with GT0: a0 128/(128+1e-7), a1 96/128 = .75, a2 64/192 = 1/3, a3 0: sum 2.083 -> k0 = 2.
      IoU with GT1: a0 .5, a1 .375, a2 .5, a3 .25: sum 1.625 -> k1 = 1.
      cost = sum_c QFL(x_c, y_c) - 3 log(iou + 1e-7) + 10^(dist/8 - 3):
      GT0: a0 = QFL(1, ~1) + QFL(-1, 0) + ~0 + 10^-2.5 ~ 0.05, a1 = QFL(0, .75) + QFL(0, 0) + 0.86 + 10^-2.5
      ~ 1.08, a2 ~ 3.3 + ..., a3 ~ 48: GT0 selects a0, a1.
      GT1: a0 = QFL(1, 0) + QFL(-1, .5) + 2.08 ~ 2.83, a2 = QFL(2, 0) + QFL(4, .5) + 2.08 ~ 4.2, a1 =
      QFL(0, 0) + QFL(0, .375) + 2.94 ~ 3.1, a3 ~ 4.2+: GT1 selects a0.
    a0 is contested and goes to the lowest cost among all GTs: GT0 (which had selected it).  Final:
    a0, a1 -> GT0; a2, a3 background; GT1 gets nothing.  t = (iou00, .75, 0, 0), norm = iou00 + .75.
    Terms: cls = [QFL(1, t0) + QFL(-1, 0) + QFL(0, t1) + QFL(0, 0) + QFL(2, 0) + QFL(4, 0) + 2 QFL(-2, 0)] / norm;
      box = [(1 - GIoU00) t0 + (1 - GIoU10) t1] / norm, both predicted boxes inside GT0 = their enclosing
      box: GIoU = IoU;
      DFL distances in bins: a0 -> GT0 (.5,.5,1.5,.5): every side's two target bins are its two hot bins,
      weights 1/2: CE = log 2 per side.  a1 -> GT0 (1.5,.5,.5,.5): the left side's target bins 1|2 hold
      logits 50|0: CE = (0 + 50) / 2; mean of the 4 sides (25 + 3 log 2) / 4.
      dfl = [log 2 t0 + (25 + 3 log 2) / 4 t1] / norm;  total = 2 box + cls."""
    m, tg = _hand_case()
    r = R.dsl_loss([m], tg, 2, (16, 16), (8.0,))
    ious = [[_iou(b, g) for b in HAND_BOXES] for _, g in HAND_GTS]
    assert ious[0][1] == pytest.approx(0.75) and ious[1] == pytest.approx([0.5, 0.375, 0.5, 0.25])
    assert r["k"].tolist() == [2, 1]
    assert r["k_margins"][0] == pytest.approx(sum(ious[0]) - 2, abs=1e-9)
    assert r["k_margins"][1] == pytest.approx(2 - sum(ious[1]), abs=1e-9)        # the nearest integer is 2
    gtc = [(8, 4), (8, 8)]
    cost = [[_cost(HAND_LOGITS[a], cls, ious[j][a], HAND_CENTRES[a], gtc[j]) for a in range(4)]
            for j, (cls, _) in enumerate(HAND_GTS)]
    assert sorted(range(4), key=lambda a: cost[0][a])[:2] == [0, 1] and min(range(4), key=lambda a: cost[1][a]) == 0
    assert r["picks"] == {0: [0, 1], 1: [0]}
    assert r["gt"].tolist() == [[0, 0, -1, -1]]
    assert list(r["contested_margins"]) == [(0, 0)]
    gap, had = r["contested_margins"][(0, 0)]
    assert had and gap == pytest.approx((cost[1][0] - cost[0][0]) / cost[1][0], rel=1e-9)
    assert r["sel_margins"][0] == pytest.approx((sorted(cost[0])[2] - cost[0][1]) / sorted(cost[0])[2], rel=1e-9)
    assert r["sel_margins"][1] == pytest.approx((sorted(cost[1])[1] - cost[1][0]) / sorted(cost[1])[1], rel=1e-9)
    assert r["exact_ties"] == 0
    t0, t1 = ious[0][0], ious[0][1]
    assert r["t"][0].tolist() == pytest.approx([t0, t1, 0.0, 0.0], rel=1e-9)
    norm = t0 + t1
    assert float(r["norm"]) == pytest.approx(norm, rel=1e-9)
    cls = (_qfl(1, t0) + _qfl(-1, 0) + _qfl(0, t1) + _qfl(0, 0) + _qfl(2, 0) + _qfl(4, 0) + 2 * _qfl(-2, 0)) / norm
    box = ((1 - _iou(HAND_BOXES[0], HAND_GTS[0][1], True)) * t0 + (1 - _iou(HAND_BOXES[1], HAND_GTS[0][1], True)) * t1) / norm
    assert _iou(HAND_BOXES[1], HAND_GTS[0][1], True) == pytest.approx(0.75, rel=1e-8)
    dfl = (math.log(2) * t0 + (25 + 3 * math.log(2)) / 4 * t1) / norm
    assert float(r["cls"]) == pytest.approx(cls, rel=1e-9)
    assert float(r["box"]) == pytest.approx(box, rel=1e-9)
    assert float(r["dfl"]) == pytest.approx(dfl, rel=1e-9)
    assert float(r["total"]) == pytest.approx(2 * box + cls, rel=1e-9)


def _rand(B, nc, shapes, seed):
    return [x.double() for x in C.maps(B, nc, shapes, seed, 1.5)]


def test_no_targets_and_no_candidates():
    """No targets, or only a GT that contains no anchor centre (no candidates in its image): nothing is
    assigned, box = dfl = 0, cls = sum softplus(x) sigmoid(x)^2 (norm = 1), total = cls."""
    B, nc = 2, 3
    maps = _rand(B, nc, [(4, 4), (2, 2)], 1)
    x = torch.cat([m.permute(0, 2, 3, 1).reshape(B, -1, 64 + nc) for m in maps], 1)[..., 64:]
    want = (torch.nn.functional.softplus(x) * torch.sigmoid(x) ** 2).sum()
    for tg in (torch.zeros(0, 6), torch.tensor([[0, 1, 0.5, 0.5, 1 / 32, 1 / 32]])):
        r = R.dsl_loss(maps, tg, nc, (32, 32), (8.0, 16.0))
        assert (r["gt"] == -1).all() and float(r["norm"]) == 1.0 and (r["k"] == 0).all()
        assert float(r["box"]) == 0.0 and float(r["dfl"]) == 0.0
        assert float(r["cls"]) == pytest.approx(float(want), rel=1e-12)
        assert float(r["total"]) == pytest.approx(float(want), rel=1e-12)


def test_ignored_rows_change_nothing():
    """Rows with image -1, image >= B, class >= nc or class < 0 are never assigned and get k = 0: values
    and assignment equal those of the list without them (row numbers aside)."""
    B, nc = 2, 3
    maps = _rand(B, nc, [(4, 4), (2, 2)], 3)
    good = C.rand_targets(B, nc, 2, 4)
    bad = torch.tensor([[-1, 1, .5, .5, .8, .8], [2, 1, .5, .5, .8, .8], [0, 3, .5, .5, .8, .8], [1, -1, .5, .5, .8, .8]])
    mixed = torch.cat([bad[:2], good[:2], bad[2:], good[2:]])
    keep = [2, 3, 6, 7]
    a = R.dsl_loss(maps, good, nc, (32, 32), (8.0, 16.0))
    b = R.dsl_loss(maps, mixed, nc, (32, 32), (8.0, 16.0))
    assert (a["gt"] >= 0).any()
    remap = torch.tensor(keep + [-1])
    assert torch.equal(remap[a["gt"]], b["gt"]) and torch.equal(a["t"], b["t"])
    assert torch.equal(b["k"][keep], a["k"]) and (b["k"][[0, 1, 4, 5]] == 0).all() and (a["k"] >= 1).all()
    for k in ("total", "box", "cls", "dfl", "norm"):
        assert float(a[k]) == float(b[k])


def test_centreless_gt_is_matched_and_shared_candidates():
    """A GT that contains no anchor centre still selects its k = 1 anchor when the image has candidates
    (those of another GT), and keeps it when nobody contests it."""
    maps = _rand(1, 2, [(4, 4)], 2)
    big = [0, 1, 0.3, 0.3, 0.5, 0.5]                          # (1.6, 17.6)^2: holds the centres 4 and 12
    tiny = [0, 0, 24 / 32, 24 / 32, 2 / 32, 2 / 32]           # (23, 25)^2, between the centres 20 and 28
    r = R.dsl_loss(maps, torch.tensor([big, tiny]), 2, (32, 32), (8.0,))
    assert int(r["k"][1]) == 1 and len(r["picks"][1]) == 1
    a = r["picks"][1][0]
    assert a in (0, 1, 4, 5)                                  # a candidate of the image: inside the OTHER GT
    if a not in r["picks"][0]:
        assert int(r["gt"][0, a]) == 1
    alone = R.dsl_loss(maps, torch.tensor([tiny]), 2, (32, 32), (8.0,))
    assert (alone["gt"] == -1).all() and int(alone["k"][0]) == 0
    # the composite's centre-less GT selects too
    c, rc, _ = C.reference("composite")
    assert int(rc["k"][C.CENTRELESS_ROW]) == 1 and len(rc["picks"][C.CENTRELESS_ROW]) == 1


def test_prior_ties_fall_to_the_index():
    """dsl_cases.prior_ties: every cost of the far 1 px GT is the saturated prior, equal in fp64 and in
    fp32; it selects the lowest-index candidate, with margin exactly 0."""
    c, r, _ = C.reference("prior_ties")
    assert r["picks"][1] == [C.PRIOR_TIES_PICK] and int(r["k"][1]) == 1
    assert r["sel_margins"][1] == 0.0 and r["exact_ties"] >= 1
    r32 = R.dsl_loss([m.float() for m in c["maps"]], c["targets"], c["nc"], c["img"], c["strides"], dtype=torch.float32)
    assert r32["picks"][1] == [C.PRIOR_TIES_PICK] and r32["sel_margins"][1] == 0.0
    assert torch.equal(r32["gt"], r["gt"])
    assert float(torch.tensor(10.0, dtype=torch.float32) ** 30 + 100.0) == float(torch.tensor(10.0, dtype=torch.float32) ** 30)
    assert 1e30 + 100.0 == 1e30


def test_composite_holds_what_it_promises():
    c, r, _ = C.reference("composite")
    tg = c["targets"]
    e_row = len(tg) - 3
    assert tg[e_row].tolist() == pytest.approx(C.WIN_ROWS[0])
    # the contested anchor whose winner had not selected it
    assert int(r["gt"][C.WIN_IMG, C.STAR]) == e_row
    gap, had = r["contested_margins"][(C.WIN_IMG, C.STAR)]
    assert not had and gap > 0.1
    assert C.STAR not in r["picks"][e_row] and r["picks"][e_row + 1] == [C.STAR] and r["picks"][e_row + 2] == [C.STAR]
    assert int(r["k"][e_row]) == 3
    assert (r["gt"][1] == -1).all()                                        # the empty image
    g0 = r["gt"][0]
    assert int((g0 == C.N_RAND + 1).sum()) > 0 or int((g0 == C.N_RAND + 2).sum()) > 0     # two classes, shared anchors
    assert set(r["picks"][C.N_RAND + 1]) & set(r["picks"][C.N_RAND + 2])
    for ignored in range(C.N_RAND + 4, C.N_RAND + 8):
        assert int((r["gt"] == ignored).sum()) == 0 and int(r["k"][ignored]) == 0 and ignored not in r["picks"]


@pytest.mark.parametrize("name", ["composite", "nc7_ld72", "level4", "dfl_gain"])
def test_gradients_and_total(name):
    c, r, grads = C.reference(name)
    B = c["maps"][0].shape[0]
    gb, gc, gd = c["gains"]
    assert float(r["total"]) == pytest.approx(gb * float(r["box"]) + gc * float(r["cls"]) + gd * float(r["dfl"]),
                                              rel=1e-12)
    if name != "dfl_gain":
        assert float(r["total"]) == pytest.approx(2 * float(r["box"]) + float(r["cls"]), rel=1e-12)
    flat = torch.cat([g.permute(0, 2, 3, 1).reshape(B, -1, g.shape[1]) for g in grads], 1)
    assert torch.isfinite(flat).all()
    fg = r["gt"] >= 0
    pos = r["t"] > 0
    assert pos.any() and (fg | ~pos).all()
    assert (flat[pos][:, :64].abs().sum(-1) > 0).all() and (flat[:, :, 64:].abs().sum(-1) > 0).all()
    assert (flat[~fg][:, :64] == 0).all()                 # background anchors: no box / DFL gradient


@pytest.mark.parametrize("name", list(C.CASES))
def test_margins_of_every_gpu_input(name):
    """The GPU tests ask the fp32 kernels for the exact assignment and the exact dynamic k.  That is fair
    only where no decision of the restatement hangs on less than fp32 resolves: every selection gap (last
    selected vs first rejected cost) and every contested-anchor gap (best vs second cost) exceeds 1e-4
    relative and every IoU sum is more than 1e-3 from an integer; exact ties occur only in the cases built
    for them, where every other gap still meets the bar.  The restatement evaluated in fp32 reproduces
    the fp64 assignment and every k."""
    c, r, _ = C.reference(name)
    gaps = list(r["sel_margins"].values()) + [g for g, _ in r["contested_margins"].values()]
    if c["exact_ties"]:
        assert r["exact_ties"] > 0
        assert all(g > 1e-4 or g == 0.0 for g in gaps)
    else:
        assert r["exact_ties"] == 0
        assert all(g > 1e-4 for g in gaps), min(gaps)
    assert all(m > 1e-3 for m in r["k_margins"].values()), min(r["k_margins"].values())
    if name not in ("m0",):
        assert len(c["targets"]) > 0
    r32 = R.dsl_loss([m.to(c["dtype"]).float() for m in c["maps"]], c["targets"], c["nc"], c["img"], c["strides"],
                     c["topk"], c["radius"], c["iou_weight"], c["beta"], c["gains"], dtype=torch.float32)
    assert torch.equal(r32["gt"], r["gt"]) and torch.equal(r32["k"], r["k"])


def test_cases_cover_what_the_gpu_tests_rely_on():
    ks = set()
    contested = 0
    for name in C.CASES:
        _, r, _ = C.reference(name)
        ks |= set(r["k"].tolist())
        contested += len(r["contested_margins"])
    assert {0, 1, 2, 3, 4, 5, 6, 7} <= ks and contested > 20
    c, r, _ = C.reference("anchors5")
    assert c["maps"][0].shape[2] * c["maps"][0].shape[3] == 5          # fewer candidates than topk = 13
    assert (r["gt"] >= 0).any()
    assert all(len(C.reference(n)[0]["targets"]) == m for n, m in (("rows300", 300), ("rows5000", 5000), ("m0", 0),
                                                                     ("m1", 1)))


def test_dsl_malformed_calls_never_launch():
    """Every argument check returns before a launch: YMS_ERR_INVALID (1) / YMS_ERR_UNSUPPORTED (2)."""
    from yms import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 16)()
    P = ctypes.addressof(buf)
    lv = (ctypes.c_void_p * 5)(*([P] * 5))
    hs = (ctypes.c_int * 5)(*([2] * 5))
    bad_hs = (ctypes.c_int * 5)(2, 0, 2, 2, 2)
    st = (ctypes.c_float * 5)(*([8.0] * 5))
    bad_st = (ctypes.c_float * 5)(8.0, -1.0, 8.0, 8.0, 8.0)
    gains = (ctypes.c_float * 3)(2.0, 1.0, 0.0)
    F = ctypes.c_float
    good = dict(dtype=L.BF16, batch=1, nc=80, nlevels=3, maps=lv, grads=None, hs=hs, ws=hs, strides=st, ld=144,
                targets=P, n_targets=1, img_w=F(64), img_h=F(64), topk=13, radius=F(3.0), iou_weight=F(3.0),
                beta=F(2.0), gains=gains, ws_buf=P, ws_bytes=1 << 30, out=P, agt=None, asc=None, dk=None, stream=None)
    broken = dict(dtype=dict(dtype=7), batch=dict(batch=0), nc=dict(nc=0), nlevels0=dict(nlevels=0),
                  nlevels5=dict(nlevels=5), maps=dict(maps=None), hs=dict(hs=None), hs0=dict(hs=bad_hs),
                  ws=dict(ws=None), strides=dict(strides=None), stride_neg=dict(strides=bad_st),
                  ld_small=dict(ld=136), ld_mod8=dict(ld=148),
                  targets=dict(targets=None), n_neg=dict(n_targets=-1), topk0=dict(topk=0), topk14=dict(topk=14),
                  radius=dict(radius=F(-1.0)), radius_nan=dict(radius=F(float("nan"))),
                  iou_weight=dict(iou_weight=F(-0.5)), iou_weight_inf=dict(iou_weight=F(float("inf"))),
                  beta_small=dict(beta=F(0.5)), beta_nan=dict(beta=F(float("nan"))), beta_inf=dict(beta=F(float("inf"))),
                  img_w=dict(img_w=F(0.0)), img_h=dict(img_h=F(float("inf"))), gains=dict(gains=None),
                  ws_null=dict(ws_buf=None), ws_small=dict(ws_bytes=16), out=dict(out=None))
    for label, change in broken.items():
        assert lib.yms_dsl_loss(*[change.get(k, v) for k, v in good.items()]) == 1, label
    assert lib.yms_dsl_loss(*[dict(batch=70000).get(k, v) for k, v in good.items()]) == 2
    assert lib.yms_dsl_loss_ws_bytes(0, 10, 80, 1) == 0 and lib.yms_dsl_loss_ws_bytes(2, 8400, 80, 16) > 2 * 8400 * 40
