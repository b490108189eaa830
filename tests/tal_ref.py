"""Plain-torch restatement of the task-aligned assigner loss (YOLOv8's published v8DetectionLoss +
TaskAlignedAssigner) that csrc/tal_loss.hip computes: THE DEFINITION of yolov8.tools.tal_loss, kept
with the tests like mosaic_ref.py.  fp64 by default, loops over images and GTs, autograd for the
gradients.  The ultralytics package is not available here, so parity with it is not pinned; this
file follows the published algorithm with two points fixed that the publication leaves open
(top-k ties and the all-zero case: metric descending, then anchor index ascending) and one
deliberate deviation (CIoU is the project's formula, `ciou` below, whose eps sits in the union and
in the arctangents' denominators; ultralytics places it in the heights and the enclosing diagonal:
an effect of order 1e-7).

tal_loss(...) returns the four values (total differentiable w.r.t. the maps), the assignment
(gt [B, A]: target row or -1; t [B, A]: target score) and the MARGINS by which the assignment was
decided: for every GT with a rejected candidate, the relative gap between its last accepted and
first rejected metric; for every contested anchor, the relative gap between the best and second
overlap.  Where the compared values are both exactly 0 (overlap = max(CIoU, 0) = 0) the decision falls
to the index (top-k) or the lowest row (contested anchor) by definition; such ties are counted in
zero_ties, not listed as gaps.  They are the same ties in fp32 as long as the raw CIoU of the pairs
they involve is not close to 0 (a CIoU of +1e-7 has overlap^6 = 1e-42: 0 in fp32, not in fp64):
sign_margin is the smallest |CIoU| over the inside pairs of every GT or anchor decided by a zero tie.
min_last is the smallest positive last-accepted metric, which must stay a normal fp32 number.
An fp32 kernel reproduces the assignment exactly only where these margins are well above
fp32 rounding; tests/test_tal_cpu.py checks that for every input the GPU tests use."""
import math

import torch

DFL = 16
EPS = 1e-7


def ciou(p, g):
    """CIoU of xyxy boxes (broadcast), the arithmetic of yolov8.tools.loss.bbox_iou(xywh=False,
    CIoU=True) in the dtype of its inputs; alpha detached."""
    iw = (torch.min(p[..., 2], g[..., 2]) - torch.max(p[..., 0], g[..., 0])).clamp(min=0)
    ih = (torch.min(p[..., 3], g[..., 3]) - torch.max(p[..., 1], g[..., 1])).clamp(min=0)
    inter = iw * ih
    w1, h1 = p[..., 2] - p[..., 0], p[..., 3] - p[..., 1]
    w2, h2 = g[..., 2] - g[..., 0], g[..., 3] - g[..., 1]
    union = w1 * h1 + w2 * h2 - inter + EPS
    iou = inter / union
    cw = (torch.max(p[..., 2], g[..., 2]) - torch.min(p[..., 0], g[..., 0])).clamp(min=0)
    ch = (torch.max(p[..., 3], g[..., 3]) - torch.min(p[..., 1], g[..., 1])).clamp(min=0)
    rho2 = ((p[..., 0] + p[..., 2]) / 2 - (g[..., 0] + g[..., 2]) / 2) ** 2 + \
        ((p[..., 1] + p[..., 3]) / 2 - (g[..., 1] + g[..., 3]) / 2) ** 2
    d = rho2 / (cw ** 2 + ch ** 2)
    v = (4 / math.pi ** 2) * (torch.atan(w2 / (h2 + EPS)) - torch.atan(w1 / (h1 + EPS))) ** 2
    alpha = (v / (1 - iou + v + EPS)).detach()
    return iou - d - alpha * v


def anchors(maps, strides, dtype):
    """-> centres [A, 2] (pixels), stride [A]; level-major, then row-major."""
    cs, ss = [], []
    for m, s in zip(maps, strides):
        H, W = m.shape[2], m.shape[3]
        gy, gx = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
        cs.append(torch.stack(((gx.reshape(-1) + 0.5), (gy.reshape(-1) + 0.5)), -1))
        ss.append(torch.full((H * W,), float(s), dtype=dtype))
    return torch.cat(cs), torch.cat(ss)


def gt_box(row, img_size, dtype):
    """target row -> xyxy in pixels"""
    img_h, img_w = img_size
    r = row.to(dtype)
    cx, cy, w, h = r[2] * img_w, r[3] * img_h, r[4] * img_w, r[5] * img_h
    return torch.stack((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2))


def row_valid(row, B, nc):
    return 0 <= float(row[0]) < B and 0 <= float(row[1]) < nc


def tal_loss(maps, targets, nc, img_size, strides=(8.0, 16.0, 32.0), topk=10, alpha=0.5, beta=6.0,
             lambdas=(7.5, 0.5, 1.5), dtype=torch.float64):
    """maps: [B, 64 + nc, H_l, W_l] tensors (requires_grad for gradients); targets [M, 6].
    -> dict(total, box, cls, dfl, gt [B, A] long, t [B, A], tss, topk_margins {row: gap},
    contested_margins {(b, a): gap}, sign_margin, min_last, zero_ties)."""
    maps = [m if m.dtype == dtype else m.to(dtype) for m in maps]
    B = maps[0].shape[0]
    flat = torch.cat([m.permute(0, 2, 3, 1).reshape(B, -1, 4 * DFL + nc) for m in maps], 1)   # [B, A, C]
    A = flat.shape[1]
    grid, st = anchors(maps, strides, dtype)                    # grid units
    centre = grid * st[:, None]                                 # pixels
    dist_logits = flat[..., :4 * DFL].reshape(B, A, 4, DFL)
    cls_logits = flat[..., 4 * DFL:]
    e = (dist_logits.softmax(-1) * torch.arange(DFL, dtype=dtype)).sum(-1)      # [B, A, 4]
    gx, gy, s = grid[:, 0], grid[:, 1], st
    pred = torch.stack(((gx - e[..., 0]) * s, (gy - e[..., 1]) * s, (gx + e[..., 2]) * s, (gy + e[..., 3]) * s), -1)

    targets = targets.reshape(-1, 6)
    M = targets.shape[0]
    gt = torch.full((B, A), -1, dtype=torch.long)
    t = torch.zeros((B, A), dtype=dtype)
    topk_margins, contested_margins, sign_margin, min_last, zero_ties = {}, {}, math.inf, math.inf, 0
    with torch.no_grad():
        for b in range(B):
            rows = [j for j in range(M) if row_valid(targets[j], B, nc) and int(targets[j, 0]) == b]
            inside, raw, ov, met, claims = {}, {}, {}, {}, {}
            for j in rows:
                g = gt_box(targets[j], img_size, dtype)
                dmin = torch.stack((centre[:, 0] - g[0], centre[:, 1] - g[1], g[2] - centre[:, 0],
                                    g[3] - centre[:, 1])).min(0).values
                inside[j] = dmin > 1e-9
                o = ciou(pred[b], g)
                raw[j] = o
                ov[j] = torch.where(o > 0, o, torch.zeros_like(o))
                sc = torch.sigmoid(cls_logits[b, :, int(targets[j, 1])])
                met[j] = sc ** alpha * ov[j] ** beta
                cand = torch.nonzero(inside[j]).flatten().tolist()
                cand.sort(key=lambda a: (-float(met[j][a]), a))
                for a in cand[:topk]:
                    claims.setdefault(a, []).append(j)
                if len(cand) > topk:
                    last, rej = float(met[j][cand[topk - 1]]), float(met[j][cand[topk]])
                    if last > 0:
                        topk_margins[j] = (last - rej) / last
                        min_last = min(min_last, last)
                    else:
                        zero_ties += 1
                        sign_margin = min(sign_margin, float(o[inside[j]].abs().min()))
                        min_last = min([min_last] + [float(met[j][a]) for a in cand[:topk] if met[j][a] > 0])
            for a, js in claims.items():
                if len(js) == 1:
                    gt[b, a] = js[0]
                    continue
                holders = [j for j in rows if bool(inside[j][a])]           # ascending target row
                ovs = [float(ov[j][a]) for j in holders]
                best = max(ovs)
                gt[b, a] = holders[ovs.index(best)]                         # first maximum: lowest row
                second = sorted(ovs)[-2]
                if best > 0:
                    contested_margins[(b, a)] = (best - second) / best
                else:
                    zero_ties += 1
                    sign_margin = min(sign_margin, min(abs(float(raw[j][a])) for j in holders))
            for j in rows:
                mine = torch.nonzero(gt[b] == j).flatten()
                if len(mine) == 0:
                    continue
                mhat, ohat = met[j][mine].max(), ov[j][mine].max()
                t[b, mine] = met[j][mine] * ohat / (mhat + 1e-9)
        tss = t.sum().clamp(min=1.0)
        target = torch.zeros((B, A, nc), dtype=dtype)
        fg = torch.nonzero(gt >= 0)                                          # [F, 2] (b, a)
        for b, a in fg.tolist():
            target[b, a, int(targets[gt[b, a], 1])] = t[b, a]

    lam_box, lam_cls, lam_dfl = lambdas
    cls = torch.nn.functional.binary_cross_entropy_with_logits(cls_logits, target, reduction="sum") / tss
    box = torch.zeros((), dtype=dtype)
    dfl = torch.zeros((), dtype=dtype)
    if len(fg):
        fb, fa = fg[:, 0], fg[:, 1]
        g = torch.stack([gt_box(targets[j], img_size, dtype) for j in gt[fb, fa].tolist()])     # [F, 4]
        w = t[fb, fa]
        box = ((1.0 - ciou(pred[fb, fa], g)) * w).sum() / tss
        c = centre[fa]
        d = (torch.stack((c[:, 0] - g[:, 0], c[:, 1] - g[:, 1], g[:, 2] - c[:, 0], g[:, 3] - c[:, 1]), -1)
             / st[fa, None]).clamp(0, DFL - 1 - 0.01)                       # [F, 4]
        tl = d.floor().long()
        wl, wr = tl.to(dtype) + 1 - d, d - tl.to(dtype)
        logp = dist_logits[fb, fa].log_softmax(-1)                          # [F, 4, 16]
        ce_l = -logp.gather(-1, tl[..., None])[..., 0]
        ce_r = -logp.gather(-1, tl[..., None] + 1)[..., 0]
        dfl = ((ce_l * wl + ce_r * wr).mean(-1) * w).sum() / tss
    total = B * (lam_box * box + lam_cls * cls + lam_dfl * dfl)
    return dict(total=total, box=box, cls=cls, dfl=dfl, gt=gt, t=t, tss=tss, topk_margins=topk_margins,
                contested_margins=contested_margins, sign_margin=sign_margin, min_last=min_last,
                zero_ties=zero_ties)
