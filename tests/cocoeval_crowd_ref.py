"""Plain numpy / loop restatement of the published COCOeval's per-image step (pycocotools/cocoeval.py:
computeIoU, evaluateImg) for boxes WITH the annotations' ``iscrowd`` and ``area`` -- TEST
INFRASTRUCTURE ONLY, not collected as a test and sharing no code with the library.  The accumulation and
the summary do not know about either field and are cocoeval_ref's (accumulate_flags, summarize).
pycocotools / torchmetrics are not installed, so parity with them is unpinned; with no crowd and no area
this restatement is pinned bit for bit to cocoeval_ref.coco_eval (tests/test_map_crowd_cpu.py).

What the two fields change, in COCOeval's words:
  _ignore = iscrowd or area outside the range, with area the ANNOTATION's (the mask's on COCO), not w*h;
  ground truths are stably sorted by _ignore, so crowd and out-of-range ones form one group in input order;
  the IoU of a detection with a crowd is intersection / detection area (maskUtils.iou, iscrowd = 1);
  a matched crowd is not skipped by later detections ("if gtm[tind, gind] > 0 and not iscrowd[gind]");
  a detection matched to an ignore ground truth is ignored; npig counts the ground truths that are not.
A detection's own area stays w*h (loadRes)."""
from __future__ import annotations

import numpy as np

from cocoeval_ref import AREA_RNG, IOU_THRS, MAX_DETS, accumulate_flags, summarize


def _xywh(b):
    """fp32 xyxy -> x, y, w, h doubles, the subtraction done in fp32 (torchvision box_convert)"""
    b = np.asarray(b, dtype=np.float32).reshape(-1, 4)
    return (b[:, 0].astype(np.float64), b[:, 1].astype(np.float64),
            (b[:, 2] - b[:, 0]).astype(np.float64), (b[:, 3] - b[:, 1]).astype(np.float64))


def crowd_iou(dboxes, gboxes, crowd):
    """maskUtils.iou(d, g, iscrowd) for boxes: [nd, ng] doubles; union = the detection's area for a crowd"""
    dx, dy, dw, dh = _xywh(dboxes)
    gx, gy, gw, gh = _xywh(gboxes)
    out = np.zeros((len(dx), len(gx)))
    for i in range(len(dx)):
        for j in range(len(gx)):
            w = min(dx[i] + dw[i], gx[j] + gw[j]) - max(dx[i], gx[j])
            h = min(dy[i] + dh[i], gy[j] + gh[j]) - max(dy[i], gy[j])
            if w <= 0 or h <= 0:
                continue
            inter = w * h
            da = dw[i] * dh[i]
            union = da if crowd[j] else da + gw[j] * gh[j] - inter
            out[i, j] = inter / union
    return out


def evaluate_image(dboxes, dscores, dlabels, gboxes, glabels, gcrowd=None, garea=None, iou_thrs=IOU_THRS):
    """COCOeval.evaluateImg for every class and area range of one image.
    gcrowd [ng] (nonzero = crowd, None = none), garea [ng] (None = w*h of the box).
    -> rank [nd], matched [4, T, nd], ignored [4, T, nd] (input order; rank >= 100: False), gt_ignore [4, ng]."""
    dboxes = np.asarray(dboxes, np.float32).reshape(-1, 4)
    gboxes = np.asarray(gboxes, np.float32).reshape(-1, 4)
    dscores = np.asarray(dscores)
    dlabels = np.asarray(dlabels).astype(np.int64)
    glabels = np.asarray(glabels).astype(np.int64)
    nd, ng, T = len(dscores), len(glabels), len(iou_thrs)
    _, _, dw, dh = _xywh(dboxes)
    _, _, gw, gh = _xywh(gboxes)
    darea = dw * dh
    crowd = np.zeros(ng, dtype=bool) if gcrowd is None else np.asarray(gcrowd).reshape(-1) != 0
    area = gw * gh if garea is None else np.asarray(garea, dtype=np.float32).reshape(-1).astype(np.float64)
    assert len(crowd) == ng and len(area) == ng
    rank = np.zeros(nd, dtype=np.int64)
    matched = np.zeros((4, T, nd), dtype=bool)
    ignored = np.zeros((4, T, nd), dtype=bool)
    gt_ignore = np.zeros((4, ng), dtype=bool)
    for a, (lo, hi) in enumerate(AREA_RNG):
        for j in range(ng):
            gt_ignore[a, j] = bool(crowd[j]) or bool(area[j] < lo) or bool(area[j] > hi)
    for c in np.unique(np.concatenate([dlabels, glabels])):
        di = np.nonzero(dlabels == c)[0]
        gi = np.nonzero(glabels == c)[0]
        order = di[np.argsort(-dscores[di], kind="mergesort")]
        rank[order] = np.arange(len(order))
        dt = order[:MAX_DETS[-1]]
        ious_in = crowd_iou(dboxes[dt], gboxes[gi], crowd[gi])
        for a, (lo, hi) in enumerate(AREA_RNG):
            gtind = np.argsort(gt_ignore[a][gi], kind="mergesort")       # not ignored first, input order in each group
            g_ig = gt_ignore[a][gi][gtind]
            g_crowd = crowd[gi][gtind]
            ious = ious_in[:, gtind]
            for ti, t in enumerate(iou_thrs):
                gtm = np.zeros(len(gi), dtype=bool)
                for k, d in enumerate(dt):
                    iou, m = min(t, 1 - 1e-10), -1
                    for g in range(len(gi)):
                        if gtm[g] and not g_crowd[g]:
                            continue
                        if m > -1 and not g_ig[m] and g_ig[g]:
                            break
                        if ious[k, g] < iou:
                            continue
                        iou, m = ious[k, g], g
                    if m == -1:
                        ignored[a, ti, d] = bool(darea[d] < lo) or bool(darea[d] > hi)
                        continue
                    gtm[m] = True
                    matched[a, ti, d] = True
                    ignored[a, ti, d] = g_ig[m]
    return rank, matched, ignored, gt_ignore


def coco_eval(preds, targets, iou_thrs=None):
    """preds: dicts of 'boxes' xyxy, 'scores', 'labels'; targets: 'boxes', 'labels' and optionally 'iscrowd',
    'area' (numpy arrays).  -> dict: per_image [(rank, matched, ignored, gt_ignore)], precision, recall, npig,
    summary."""
    iou_thrs = IOU_THRS if iou_thrs is None else np.asarray(iou_thrs, dtype=np.float64)
    top = 0
    for d in list(preds) + list(targets):
        if len(d["labels"]):
            top = max(top, int(np.max(d["labels"])) + 1)
    K = max(top, 1)
    npig = np.zeros((K, 4), dtype=np.int64)
    flags, acc_in = [], []
    for p, t in zip(preds, targets):
        rank, matched, ignored, gt_ignore = evaluate_image(p["boxes"], p["scores"], p["labels"], t["boxes"], t["labels"],
                                                           t.get("iscrowd"), t.get("area"), iou_thrs)
        flags.append((rank, matched, ignored, gt_ignore))
        acc_in.append((np.asarray(p["scores"]), np.asarray(p["labels"]).astype(np.int64), rank, matched, ignored))
        for j, c in enumerate(np.asarray(t["labels"]).astype(np.int64)):
            for a in range(4):
                if not gt_ignore[a, j]:
                    npig[c, a] += 1
    precision, recall = accumulate_flags(acc_in, npig, K, len(iou_thrs))
    with_gt = [c for c in range(K) if npig[c, 0] > 0]
    return {"per_image": flags, "precision": precision, "recall": recall, "npig": npig,
            "summary": summarize(precision, recall, iou_thrs, with_gt)}


def clustered_crowd(rng, n_img, nc=6, max_det=300):
    """cocoeval_ref.clustered (ground-truth sides log-uniform in [8, 300] px, detections jittered around them
    with sigma 0.08 of the side, scores with exact ties, a floor of random boxes) with two changes:
      about 15 % of the ground truths are crowd, their box enlarged to 2-4x its side about the same centre
        while the detections stay clustered on the original box, so several fall inside one crowd;
      area = u * w*h of the (fp32) box, u ~ U(0.3, 1.0), so boxes cross the 32^2 / 96^2 borders.
    An image keeps its first max_det detections (the random floor comes last)."""
    preds, targets = [], []
    for _ in range(n_img):
        k = int(rng.integers(0, 9))
        c = rng.uniform(40, 600, (k, 2))
        wh = np.exp(rng.uniform(np.log(8), np.log(300), (k, 2)))
        crowd = rng.random(k) < 0.15
        big = wh * np.where(crowd, rng.uniform(2, 4, k), 1.0)[:, None]
        tight = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
        gb = np.concatenate([c - big / 2, c + big / 2], 1).astype(np.float32)
        gl = rng.integers(0, nc, k)
        area = (rng.uniform(0.3, 1.0, k) * (gb[:, 2] - gb[:, 0]).astype(np.float64)
                * (gb[:, 3] - gb[:, 1]).astype(np.float64)).astype(np.float32)
        boxes, scores, labels = [], [], []
        for j in range(k):
            m = int(rng.integers(0, 40))
            boxes.append(tight[j] + rng.normal(0, 0.08, (m, 4)) * np.tile(wh[j], 2))
            scores.append(np.round(rng.beta(2, 5, m) * 16) / 16)          # exact ties
            labels.append(np.where(rng.random(m) < 0.85, gl[j], rng.integers(0, nc, m)))
        fp = int(rng.integers(0, 30))
        boxes.append(rng.uniform(0, 640, (fp, 4)).cumsum(1) % 640)
        scores.append(rng.random(fp))
        labels.append(rng.integers(0, nc, fp))
        b = np.concatenate(boxes).astype(np.float32).reshape(-1, 4)[:max_det]
        b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 1)
        preds.append({"boxes": b, "scores": np.concatenate(scores).astype(np.float32)[:max_det],
                      "labels": np.concatenate(labels).astype(np.int64)[:max_det]})
        targets.append({"boxes": gb.reshape(-1, 4), "labels": gl.astype(np.int64),
                        "iscrowd": crowd.astype(np.uint8), "area": area})
    return preds, targets
