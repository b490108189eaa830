"""Pins tests/tal_ref.py, the plain-torch restatement that defines the task-aligned loss
(yolov8.tools.tal_loss, csrc/tal_loss.hip), to a case worked by hand and to the assigner's edge
rules, and checks the condition under which an fp32 kernel can be asked for the exact assignment:
the margins of every seeded input of tests/tal_cases.py."""
import ctypes
import math

import pytest
import torch

import tal_cases as C
import tal_ref as R

EPS = 1e-7


def _ciou(p, g):
    """scalar CIoU of xyxy boxes, written out independently of tal_ref.ciou"""
    iw = max(min(p[2], g[2]) - max(p[0], g[0]), 0.0)
    ih = max(min(p[3], g[3]) - max(p[1], g[1]), 0.0)
    inter = iw * ih
    w1, h1, w2, h2 = p[2] - p[0], p[3] - p[1], g[2] - g[0], g[3] - g[1]
    iou = inter / (w1 * h1 + w2 * h2 - inter + EPS)
    cw = max(p[2], g[2]) - min(p[0], g[0])
    ch = max(p[3], g[3]) - min(p[1], g[1])
    rho2 = ((p[0] + p[2] - g[0] - g[2]) / 2) ** 2 + ((p[1] + p[3] - g[1] - g[3]) / 2) ** 2
    v = 4 / math.pi ** 2 * (math.atan(w2 / (h2 + EPS)) - math.atan(w1 / (h1 + EPS))) ** 2
    return iou - rho2 / (cw * cw + ch * ch) - v / (1 - iou + v + EPS) * v


def _sig(x):
    return 1 / (1 + math.exp(-x))


def _bce(x, t):
    return (1 - t) * x + math.log1p(math.exp(-abs(x))) + max(-x, 0.0)


def _two_hot(m, a_yx, side, lo, val=50.0):
    m[0, side * 16 + lo, a_yx[0], a_yx[1]] = val
    m[0, side * 16 + lo + 1, a_yx[0], a_yx[1]] = val


def _hand_case():
    m = torch.zeros(1, 66, 2, 2, dtype=torch.float64)
    for yx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        for side in range(4):
            _two_hot(m, yx, side, 1 if (yx == (0, 0) and side == 2) else 0)
    logits = {(0, 0): (1.0, -1.0), (0, 1): (0.0, 0.0), (1, 0): (0.0, 2.0), (1, 1): (-2.0, -2.0)}
    for yx, (c0, c1) in logits.items():
        m[0, 64, yx[0], yx[1]] = c0
        m[0, 65, yx[0], yx[1]] = c1
    tg = torch.tensor([[0, 0, 0.5, 0.25, 1.0, 0.5], [0, 1, 0.25, 0.5, 0.5, 1.0]], dtype=torch.float64)
    return m, tg, logits


def test_hand_worked_case():
    """One level, 2 x 2 anchors of stride 8 on a 16 x 16 image, nc = 2, topk = 10.

    Anchors a0..a3 have centres (4,4), (12,4), (4,12), (12,12).  DFL logits are two-hot (50 at two
    neighbouring bins, the other bins leak 14 e^-50 ~ 3e-21): every side expects 0.5 bins = 4 px,
    except a0's right side, 1.5 bins = 12 px.  Predicted boxes: a0 (0,0,16,8), a1 (8,0,16,8),
    a2 (0,8,8,16), a3 (8,8,16,16).  Class logits (class 0, class 1): a0 (1,-1), a1 (0,0), a2 (0,2),
    a3 (-2,-2).

    GT0 = class 0, box (0,0,16,8): contains the centres of a0, a1.  GT1 = class 1, box (0,0,8,16):
    contains a0, a2.  Both have 2 < topk candidates, so both claim all of theirs: a0 is contested.
      ov(a0,GT0) = CIoU of identical boxes = 128 / (128 + 1e-7);  ov(a0,GT1) = CIoU((0,0,16,8),
      (0,0,8,16)): IoU 64/192, centre distance^2 32 over diagonal^2 512, aspect term > 0 -> < 1/3.
    a0 goes to GT0 (largest overlap).  Final sets: GT0 {a0, a1}, GT1 {a2}, a3 background.
      m(a, j) = sigmoid(logit[a, class_j])^0.5 ov^6:  m00 = sqrt(sig 1) ov00^6, m10 = sqrt(.5) ov10^6,
      m21 = sqrt(sig 2) ov21^6, with ov10 = CIoU((8,0,16,8), GT0), ov21 = CIoU((0,8,8,16), GT1).
      Mhat0 = m00 (ov10^6 is tiny), Ohat0 = ov00;  Mhat1 = m21, Ohat1 = ov21.
      t0 = m00 ov00 / (m00 + 1e-9), t1 = m10 ov00 / (m00 + 1e-9), t2 = m21 ov21 / (m21 + 1e-9);
      tss = max(t0 + t1 + t2, 1) = t0 + t1 + t2  (t0 ~ 1).
    Terms:  cls = [BCE(1,t0) + BCE(-1,0) + BCE(0,t1) + BCE(0,0) + BCE(0,0) + BCE(2,t2) + 2 BCE(-2,0)] / tss
      box = [(1 - ov00) t0 + (1 - ciou10) t1 + (1 - ciou21) t2] / tss   (ov = CIoU here: all > 0)
      DFL distances in bins: a0 -> GT0 (.5,.5,1.5,.5): every side's two target bins are its two hot
      bins with weights 1/2: CE = log 2 per side.  a1 -> GT0 (1.5,.5,.5,.5): the left side's target
      bins 1|2 hold logits 50|0: CE = (log 2 + (50 + log 2)) / 2; mean of 4 sides = log 2 + 6.25.
      a2 -> GT1 (.5,1.5,.5,.5): the same.  dfl = [log 2 t0 + (log 2 + 6.25)(t1 + t2)] / tss.
      total = 1 * (7.5 box + 0.5 cls + 1.5 dfl)."""
    m, tg, lg = _hand_case()
    r = R.tal_loss([m], tg, 2, (16, 16), (8.0,))
    assert r["gt"].tolist() == [[0, 0, 1, -1]]
    assert r["topk_margins"] == {} and list(r["contested_margins"]) == [(0, 0)]
    g0, g1 = (0, 0, 16, 8), (0, 0, 8, 16)
    ov00, ov01 = _ciou((0, 0, 16, 8), g0), _ciou((0, 0, 16, 8), g1)
    ov10, ov21 = _ciou((8, 0, 16, 8), g0), _ciou((0, 8, 8, 16), g1)
    assert 0 < ov01 < 1 / 3 < ov00 and ov10 > 0 and ov21 > 0
    assert r["contested_margins"][(0, 0)] == pytest.approx((ov00 - ov01) / ov00, rel=1e-9)
    m00, m10, m21 = math.sqrt(_sig(1)) * ov00 ** 6, math.sqrt(0.5) * ov10 ** 6, math.sqrt(_sig(2)) * ov21 ** 6
    assert m00 > m10
    t0, t1, t2 = m00 * ov00 / (m00 + 1e-9), m10 * ov00 / (m00 + 1e-9), m21 * ov21 / (m21 + 1e-9)
    assert r["t"][0].tolist() == pytest.approx([t0, t1, t2, 0.0], rel=1e-9)
    tss = t0 + t1 + t2
    assert tss > 1 and float(r["tss"]) == pytest.approx(tss, rel=1e-9)
    cls = (_bce(1, t0) + _bce(-1, 0) + _bce(0, t1) + _bce(0, 0) + _bce(0, 0) + _bce(2, t2) + 2 * _bce(-2, 0)) / tss
    box = ((1 - ov00) * t0 + (1 - ov10) * t1 + (1 - ov21) * t2) / tss
    dfl = (math.log(2) * t0 + (math.log(2) + 6.25) * (t1 + t2)) / tss
    assert float(r["cls"]) == pytest.approx(cls, rel=1e-9)
    assert float(r["box"]) == pytest.approx(box, rel=1e-9)
    assert float(r["dfl"]) == pytest.approx(dfl, rel=1e-9)
    assert float(r["total"]) == pytest.approx(7.5 * box + 0.5 * cls + 1.5 * dfl, rel=1e-9)


def _rand(B, nc, shapes, seed):
    return [x.double() for x in C.maps(B, nc, shapes, seed, 1.5)]


def test_no_targets_and_no_candidate_gt():
    """No targets, or only a GT that contains no anchor centre: no foreground, box = dfl = 0,
    cls = sum BCE(x, 0) (tss = 1), total = B * 0.5 cls."""
    B, nc = 2, 3
    maps = _rand(B, nc, [(4, 4), (2, 2)], 1)
    x = torch.cat([m.permute(0, 2, 3, 1).reshape(B, -1, 64 + nc) for m in maps], 1)[..., 64:]
    want = torch.nn.functional.softplus(x).sum()
    for tg in (torch.zeros(0, 6), torch.tensor([[0, 1, 0.5, 0.5, 1 / 32, 1 / 32]])):
        r = R.tal_loss(maps, tg, nc, (32, 32), (8.0, 16.0))
        assert (r["gt"] == -1).all() and float(r["tss"]) == 1.0
        assert float(r["box"]) == 0.0 and float(r["dfl"]) == 0.0
        assert float(r["cls"]) == pytest.approx(float(want), rel=1e-12)
        assert float(r["total"]) == pytest.approx(B * 0.5 * float(want), rel=1e-12)


def test_fewer_inside_anchors_than_topk():
    """A GT holding 3 anchor centres gets exactly those 3, whatever their metric."""
    maps = _rand(1, 2, [(4, 4)], 2)
    tg = torch.tensor([[0, 1, 20 / 32, 4 / 32, 22 / 32, 6 / 32]])       # x in (9, 31), y in (1, 7): row 0, gx 1..3
    r = R.tal_loss(maps, tg, 2, (32, 32), (8.0,))
    assert torch.nonzero(r["gt"][0] == 0).flatten().tolist() == [1, 2, 3]
    assert r["topk_margins"] == {}


def test_ignored_rows_change_nothing():
    """Rows with image -1, image >= B, class >= nc or class < 0 are never assigned: values and
    assignment equal those of the list without them (row numbers aside)."""
    B, nc = 2, 3
    maps = _rand(B, nc, [(4, 4), (2, 2)], 3)
    good = C.rand_targets(B, nc, 2, 4)
    bad = torch.tensor([[-1, 1, .5, .5, .8, .8], [2, 1, .5, .5, .8, .8], [0, 3, .5, .5, .8, .8], [1, -1, .5, .5, .8, .8]])
    mixed = torch.cat([bad[:2], good[:2], bad[2:], good[2:]])
    keep = [2, 3, 6, 7]
    a = R.tal_loss(maps, good, nc, (32, 32), (8.0, 16.0))
    b = R.tal_loss(maps, mixed, nc, (32, 32), (8.0, 16.0))
    assert (a["gt"] >= 0).any()
    remap = torch.tensor(keep + [-1])
    assert torch.equal(remap[a["gt"]], b["gt"]) and torch.equal(a["t"], b["t"])
    for k in ("total", "box", "cls", "dfl"):
        assert float(a[k]) == float(b[k])


def test_exact_metric_ties_resolve_by_anchor_index():
    """beta = 0, alpha = 1 and equal class logits: m = sigmoid(x) for every candidate, an exact
    non-zero tie; the all-zero metric case of tal_cases ties at 0.  Both fall to the anchor index."""
    maps = _rand(1, 2, [(4, 4)], 5)
    maps[0][:, 64:] = 0.7
    tg = torch.tensor([[0, 1, 0.5, 0.5, 0.7, 0.7]])                       # (4.8, 27.2)^2 holds the 4 centres at 12 and 20
    r = R.tal_loss(maps, tg, 2, (32, 32), (8.0,), topk=2, alpha=1.0, beta=0.0)
    inside = [a for a in range(16) if 4.8 < (a % 4 + .5) * 8 < 27.2 and 4.8 < (a // 4 + .5) * 8 < 27.2]
    assert len(inside) == 4 and torch.nonzero(r["gt"][0] == 0).flatten().tolist() == inside[:2]
    assert r["topk_margins"] == {0: 0.0}
    c, z, _ = C.reference("zero_metric_ties")
    assert (z["t"] == 0).all() and float(z["tss"]) == 1.0
    cen, _ = R.anchors(c["maps"], c["strides"], torch.float64)
    cen = cen * torch.tensor([8.0] * 64 + [16.0] * 16)[:, None]
    want = torch.full_like(z["gt"], -1)
    holders, claims = {}, {}
    for j, row in enumerate(c["targets"]):
        g = R.gt_box(row, c["img"], torch.float64)
        ins = torch.nonzero((cen[:, 0] > g[0]) & (cen[:, 1] > g[1]) & (cen[:, 0] < g[2]) & (cen[:, 1] < g[3])).flatten()
        assert len(ins) > 10
        for a in ins.tolist():
            holders.setdefault((int(row[0]), a), []).append(j)
        for a in ins[:10].tolist():                       # metric 0 everywhere: the 10 lowest indices
            claims.setdefault((int(row[0]), a), []).append(j)
    for (b, a), js in claims.items():                     # contested: overlap 0 everywhere, the lowest row inside
        want[b, a] = js[0] if len(js) == 1 else holders[(b, a)][0]
    assert any(len(js) > 1 for js in claims.values())
    assert torch.equal(z["gt"], want)


def test_third_gt_takes_the_contested_anchor():
    """tal_cases' construction: STAR is claimed by the two small GTs only (the enclosing GT E alone
    rejects it: its class score there is ~4e-18), and ends up assigned to E, whose overlap is best."""
    c, r, _ = C.reference("composite")
    tg = c["targets"]
    e_row = len(tg) - 3
    assert tg[e_row].tolist() == pytest.approx(C.THIRD_ROWS[0])
    assert int(r["gt"][C.THIRD_IMG, C.STAR]) == e_row
    assert (C.THIRD_IMG, C.STAR) in r["contested_margins"]
    ins = [m.double() for m in c["maps"]]
    alone = R.tal_loss(ins, tg[:e_row + 1], c["nc"], c["img"], c["strides"])
    assert int(alone["gt"][C.THIRD_IMG, C.STAR]) == -1 and int((alone["gt"][C.THIRD_IMG] == e_row).sum()) == 10
    pair = R.tal_loss(ins, torch.cat([tg[:e_row], tg[e_row + 1:]]), c["nc"], c["img"], c["strides"])
    assert int(pair["gt"][C.THIRD_IMG, C.STAR]) in (e_row, e_row + 1)      # without E: one of the small GTs
    # the composite also holds the other edges it promises
    g0 = r["gt"][0]
    n_rand = 2
    assert int((g0 == n_rand).sum()) == 0                                  # the GT without a candidate
    assert 0 < int((g0 == n_rand + 3).sum()) < 10                          # #inside < topk
    assert int((g0 == n_rand + 1).sum()) > 0 and int((g0 == n_rand + 2).sum()) > 0    # two classes sharing anchors
    assert (r["gt"][1] == -1).all()                                        # the empty image
    for ignored in range(n_rand + 4, n_rand + 8):
        assert int((r["gt"] == ignored).sum()) == 0


@pytest.mark.parametrize("name", ["composite", "nc7_ld72", "level4"])
def test_gradients_and_total(name):
    c, r, grads = C.reference(name)
    B = c["maps"][0].shape[0]
    assert float(r["total"]) == pytest.approx(B * (7.5 * float(r["box"]) + 0.5 * float(r["cls"]) +
                                                   1.5 * float(r["dfl"])), rel=1e-12)
    flat = torch.cat([g.permute(0, 2, 3, 1).reshape(B, -1, g.shape[1]) for g in grads], 1)
    assert torch.isfinite(flat).all()
    fg = r["gt"] >= 0
    pos = r["t"] > 0                                      # box / DFL terms are weighted by t
    assert pos.any() and (fg | ~pos).all()
    assert (flat[pos][:, :64].abs().sum(-1) > 0).all() and (flat[fg][:, 64:].abs().sum(-1) > 0).all()
    assert (flat[~fg][:, :64] == 0).all()                 # background anchors: no box / DFL gradient


@pytest.mark.parametrize("name", list(C.CASES))
def test_margins_of_every_gpu_input(name):
    """The GPU tests ask the fp32 kernels for the exact assignment.  That is fair only where no
    decision of the restatement hangs on less than fp32 resolves: every top-k gap (last accepted vs
    first rejected metric) and every contested-anchor gap (best vs second overlap) exceeds 1e-4
    relative, except in the cases whose ties are exact by construction.  Ties at exactly 0 (overlap =
    max(CIoU, 0) = 0 on both sides) fall to the index by definition; they are the same ties in fp32
    as long as the raw CIoU (an O(1) quantity) of the pairs they involve is not within 1e-4 of 0 and
    every accepted positive metric at a decision is a normal fp32 number (> 1e-30); both asserted."""
    c, r, _ = C.reference(name)
    gaps = list(r["topk_margins"].values()) + list(r["contested_margins"].values())
    assert r["sign_margin"] > 1e-4 and r["min_last"] > 1e-30
    if c["exact_ties"]:
        assert not gaps and r["zero_ties"] > 0
    else:
        assert all(g > 1e-4 for g in gaps), min(gaps)
    if name not in ("m0",):
        assert len(c["targets"]) > 0


def test_tal_malformed_calls_never_launch():
    """Every argument check returns before a launch: YMS_ERR_INVALID (1) / YMS_ERR_UNSUPPORTED (2)."""
    from yms import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 16)()
    P = ctypes.addressof(buf)
    lv = (ctypes.c_void_p * 5)(*([P] * 5))
    hs = (ctypes.c_int * 5)(*([2] * 5))
    st = (ctypes.c_float * 5)(*([8.0] * 5))
    lam = (ctypes.c_float * 3)(7.5, 0.5, 1.5)
    good = dict(dtype=L.BF16, batch=1, nc=80, nlevels=3, maps=lv, grads=None, hs=hs, ws=hs, strides=st, ld=144,
                targets=P, n_targets=1, img_w=ctypes.c_float(64), img_h=ctypes.c_float(64), topk=10,
                alpha=ctypes.c_float(0.5), beta=ctypes.c_float(6.0), lambdas=lam, ws_buf=P, ws_bytes=1 << 30, out=P,
                agt=None, asc=None, stream=None)
    broken = dict(dtype=dict(dtype=7), batch=dict(batch=0), nc=dict(nc=0), nlevels0=dict(nlevels=0),
                  nlevels5=dict(nlevels=5), maps=dict(maps=None), ld_small=dict(ld=136), ld_mod8=dict(ld=148),
                  targets=dict(targets=None), n_neg=dict(n_targets=-1), topk0=dict(topk=0), topk11=dict(topk=11),
                  alpha=dict(alpha=ctypes.c_float(-1.0)), beta=dict(beta=ctypes.c_float(float("nan"))),
                  img=dict(img_w=ctypes.c_float(0.0)), lambdas=dict(lambdas=None), ws_null=dict(ws_buf=None),
                  ws_small=dict(ws_bytes=16), out=dict(out=None))
    for label, change in broken.items():
        assert lib.yms_tal_loss(*[change.get(k, v) for k, v in good.items()]) == 1, label
    assert lib.yms_tal_loss(*[dict(batch=70000).get(k, v) for k, v in good.items()]) == 2
    assert lib.yms_tal_loss_ws_bytes(0, 10, 80, 1) == 0 and lib.yms_tal_loss_ws_bytes(2, 8400, 80, 16) > 2 * 8400 * 36
