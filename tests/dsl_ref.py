"""Plain-torch restatement of YOLO-MS's own loss (the RTMDet recipe: dynamic soft-label assigner,
Quality Focal Loss on the class logits, GIoU on the boxes, both weighted by the matched IoU) that
csrc/dsl_loss.hip computes: THE DEFINITION of yolov8.tools.dsl_loss, kept with the tests like
tal_ref.py.  fp64 by default, loops over images and GTs, autograd for the gradients.  mmdet / mmyolo
are not available here, so parity with them is not pinned; this file follows the published algorithm
with these deliberate deviations: IoU / GIoU are the project's formulas (`iou`, `giou` below: eps
1e-7 in the union and in the enclosing area; mmdet clamps at 1e-6); the exponent of the soft centre
prior is capped at 30, which keeps the prior finite in fp32 (1e30 absorbs the other cost terms in
fp32 and fp64 alike); ties, which torch.topk / argmin leave open, go to the lower anchor index
(selection) and to the lower target row (contested anchor); the normaliser is per process, with no
mean over ranks.

Anchors, decode and target rows are tal_ref's.  Per image b, over its valid rows j in target order:

* candidates: the anchors whose centre lies more than 1e-9 px inside AT LEAST ONE GT of the image; one
  set shared by every GT of the image (an anchor inside GT A only is still a candidate of GT B).  No
  candidates: no GT of the image is assigned;
* iou(a, j): plain IoU of the predicted box and the GT, NaN -> 0;
* cost(a, j) = cls + box + prior with cls = sum_c BCEwithlogits(x[a, c], y_c) |y_c - sigmoid(x[a, c])|^beta,
  y = iou(a, j) at class_j and 0 elsewhere; box = -log(iou + 1e-7) iou_weight; prior =
  10^min(dist / stride_a - radius, 30), dist the pixel distance of the anchor centre from the GT centre;
* dynamic k: k_j = max(1, floor(sum of the min(topk, n_cand) largest iou(., j) over the candidates));
* GT j selects its k_j candidates of lowest cost (ties: lower anchor index), also when it contains no
  anchor centre itself;
* an anchor selected once belongs to its selector; one selected several times goes to the GT of lowest
  cost among ALL the image's valid GTs (lowest row on a tie), also one that did not select it;
* t(a) = iou(a, j_assigned) (may be 0), norm = max(sum t, 1); assignment, t and norm carry no gradient;
* cls = sum QFL / norm: BCEwithlogits(x, t) |t - sigmoid(x)|^beta at the assigned anchor's class,
  softplus(x) sigmoid(x)^beta everywhere else; box = sum_fg (1 - GIoU) t / norm; dfl = tal_ref's DFL term
  with weight t / norm; total = box_gain box + cls_gain cls + dfl_gain dfl (no factor B).

dsl_loss(...) also returns the MARGINS its decisions hung on: sel_margins {row: relative gap between
the last selected and the first rejected cost}, contested_margins {(b, a): (relative gap between the
best and the second cost, whether the winner had selected the anchor)}, k_margins {row: distance of
the IoU sum from the nearest integer, or from 1 when the sum is below 1}, and exact_ties, the count of
decisions whose two compared costs were equal.  An fp32 kernel reproduces the assignment exactly only
where these margins are well above fp32 rounding; tests/test_dsl_cpu.py checks that for every input
the GPU tests use."""
import math

import torch

from tal_ref import DFL, EPS, anchors, gt_box, row_valid


def iou(p, g):
    """plain IoU of xyxy boxes (broadcast): yolov8.tools.loss.bbox_iou(xywh=False) in the inputs' dtype"""
    return _iou_terms(p, g)[0]


def _iou_terms(p, g):
    iw = (torch.min(p[..., 2], g[..., 2]) - torch.max(p[..., 0], g[..., 0])).clamp(min=0)
    ih = (torch.min(p[..., 3], g[..., 3]) - torch.max(p[..., 1], g[..., 1])).clamp(min=0)
    inter = iw * ih
    union = (p[..., 2] - p[..., 0]) * (p[..., 3] - p[..., 1]) + (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1]) \
        - inter + EPS
    return inter / union, union


def giou(p, g):
    """bbox_iou(xywh=False, GIoU=True) in the inputs' dtype"""
    i, union = _iou_terms(p, g)
    cw = (torch.max(p[..., 2], g[..., 2]) - torch.min(p[..., 0], g[..., 0])).clamp(min=0)
    ch = (torch.max(p[..., 3], g[..., 3]) - torch.min(p[..., 1], g[..., 1])).clamp(min=0)
    ca = cw * ch + EPS
    return i - (ca - union) / ca


def qfl(x, y, beta):
    """BCEwithlogits(x, y) |y - sigmoid(x)|^beta, elementwise"""
    bce = torch.nn.functional.binary_cross_entropy_with_logits(x, y, reduction="none")
    return bce * (y - torch.sigmoid(x)).abs().pow(beta)


def dsl_loss(maps, targets, nc, img_size, strides=(8.0, 16.0, 32.0), topk=13, radius=3.0, iou_weight=3.0, beta=2.0,
             gains=(2.0, 1.0, 0.0), dtype=torch.float64):
    """maps: [B, 64 + nc, H_l, W_l] tensors (requires_grad for gradients); targets [M, 6].
    -> dict(total, box, cls, dfl, norm, gt [B, A] long (target row or -1), t [B, A], k [M] long,
    picks {row: the anchors it selected, cheapest first}, sel_margins, contested_margins, k_margins,
    exact_ties)."""
    maps = [m if m.dtype == dtype else m.to(dtype) for m in maps]
    B = maps[0].shape[0]
    flat = torch.cat([m.permute(0, 2, 3, 1).reshape(B, -1, 4 * DFL + nc) for m in maps], 1)   # [B, A, C]
    A = flat.shape[1]
    grid, st = anchors(maps, strides, dtype)
    centre = grid * st[:, None]
    dist_logits = flat[..., :4 * DFL].reshape(B, A, 4, DFL)
    cls_logits = flat[..., 4 * DFL:]
    e = (dist_logits.softmax(-1) * torch.arange(DFL, dtype=dtype)).sum(-1)
    gx, gy, s = grid[:, 0], grid[:, 1], st
    pred = torch.stack(((gx - e[..., 0]) * s, (gy - e[..., 1]) * s, (gx + e[..., 2]) * s, (gy + e[..., 3]) * s), -1)

    targets = targets.reshape(-1, 6)
    M = targets.shape[0]
    gt = torch.full((B, A), -1, dtype=torch.long)
    t = torch.zeros((B, A), dtype=dtype)
    ks = torch.zeros(M, dtype=torch.long)
    sel_margins, contested_margins, k_margins, exact_ties, picks = {}, {}, {}, 0, {}
    with torch.no_grad():
        for b in range(B):
            rows = [j for j in range(M) if row_valid(targets[j], B, nc) and int(targets[j, 0]) == b]
            boxes = {j: gt_box(targets[j], img_size, dtype) for j in rows}
            cand = torch.zeros(A, dtype=torch.bool)
            for j in rows:
                g = boxes[j]
                cand |= torch.stack((centre[:, 0] - g[0], centre[:, 1] - g[1], g[2] - centre[:, 0],
                                     g[3] - centre[:, 1])).min(0).values > 1e-9
            cidx = torch.nonzero(cand).flatten().tolist()
            if not cidx:
                continue
            ious, cost, selected = {}, {}, {}
            for j in rows:
                g, c = boxes[j], int(targets[j, 1])
                o = iou(pred[b], g)
                o = torch.where(torch.isnan(o), torch.zeros_like(o), o)
                ious[j] = o
                y = torch.zeros_like(cls_logits[b])
                y[:, c] = o
                c_cls = qfl(cls_logits[b], y, beta).sum(-1)
                c_box = -torch.log(o + EPS) * iou_weight
                d = ((centre[:, 0] - (g[0] + g[2]) / 2) ** 2 + (centre[:, 1] - (g[1] + g[3]) / 2) ** 2).sqrt()
                c_pri = 10.0 ** (d / st - radius).clamp(max=30.0)
                cost[j] = c_cls + c_box + c_pri
                n = min(topk, len(cidx))
                ssum = float(o[cand].topk(n).values.sum())
                k = max(1, int(math.floor(ssum)))
                ks[j] = k
                k_margins[j] = 1.0 - ssum if ssum < 1.0 else min(ssum - math.floor(ssum), math.ceil(ssum) - ssum)
                order = sorted(cidx, key=lambda a: (float(cost[j][a]), a))
                picks[j] = order[:k]
                for a in order[:k]:
                    selected.setdefault(a, []).append(j)
                if len(order) > k:
                    last, rej = float(cost[j][order[k - 1]]), float(cost[j][order[k]])
                    if rej == last:
                        exact_ties += 1
                    sel_margins[j] = (rej - last) / abs(rej)
            for a, js in selected.items():
                if len(js) == 1:
                    gt[b, a] = js[0]
                else:
                    cs = [float(cost[j][a]) for j in rows]               # ascending target row
                    best = min(cs)
                    w = rows[cs.index(best)]                             # first minimum: lowest row
                    gt[b, a] = w
                    second = sorted(cs)[1]
                    if second == best:
                        exact_ties += 1
                    contested_margins[(b, a)] = ((second - best) / abs(second), w in js)
                t[b, a] = ious[int(gt[b, a])][a]
        norm = t.sum().clamp(min=1.0)
        target = torch.zeros((B, A, nc), dtype=dtype)
        fg = torch.nonzero(gt >= 0)
        for b, a in fg.tolist():
            target[b, a, int(targets[gt[b, a], 1])] = t[b, a]

    box_gain, cls_gain, dfl_gain = gains
    # target is 0 off the assigned class (and at it where t = 0): BCE(x, 0) |0 - sigma|^beta = softplus(x) sigma^beta
    cls = qfl(cls_logits, target, beta).sum() / norm
    box = torch.zeros((), dtype=dtype)
    dfl = torch.zeros((), dtype=dtype)
    if len(fg):
        fb, fa = fg[:, 0], fg[:, 1]
        g = torch.stack([gt_box(targets[j], img_size, dtype) for j in gt[fb, fa].tolist()])
        w = t[fb, fa]
        box = ((1.0 - giou(pred[fb, fa], g)) * w).sum() / norm
        c = centre[fa]
        d = (torch.stack((c[:, 0] - g[:, 0], c[:, 1] - g[:, 1], g[:, 2] - c[:, 0], g[:, 3] - c[:, 1]), -1)
             / st[fa, None]).clamp(0, DFL - 1 - 0.01)
        tl = d.floor().long()
        wl, wr = tl.to(dtype) + 1 - d, d - tl.to(dtype)
        logp = dist_logits[fb, fa].log_softmax(-1)
        ce_l = -logp.gather(-1, tl[..., None])[..., 0]
        ce_r = -logp.gather(-1, tl[..., None] + 1)[..., 0]
        dfl = ((ce_l * wl + ce_r * wr).mean(-1) * w).sum() / norm
    total = box_gain * box + cls_gain * cls + dfl_gain * dfl
    return dict(total=total, box=box, cls=cls, dfl=dfl, norm=norm, gt=gt, t=t, k=ks, sel_margins=sel_margins,
                contested_margins=contested_margins, k_margins=k_margins, exact_ties=exact_ties, picks=picks)
