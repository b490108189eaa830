"""Plain numpy / loop restatement of the published COCOeval (pycocotools/cocoeval.py: evaluateImg,
accumulate, summarize) for boxes without crowd -- TEST INFRASTRUCTURE ONLY, not collected as a test
and sharing no code with the library.  pycocotools / torchmetrics are not installed, so parity with
them is unpinned; at thresholds [0.5], area 'all', maxDets 100 this restatement is pinned bit for
bit to oracle/map_ref.py (tests/test_map_coco_cpu.py).

Settings: IoU thresholds 0.50:0.05:0.95 by default, area ranges all / small / medium / large
([0, 1e10], [0, 32^2], [32^2, 96^2], [96^2, 1e10], both ends inclusive, area = w*h in double from the
fp32 w = x2 - x1, h = y2 - y1), maxDets [1, 10, 100], 101 recall thresholds."""
from __future__ import annotations

import numpy as np

from oracle.map_ref import REC_THRS, iou_xyxy

IOU_THRS = np.linspace(.5, .95, int(np.round((.95 - .5) / .05)) + 1, endpoint=True)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "small", "medium", "large"]
MAX_DETS = [1, 10, 100]
EPS = np.spacing(1)


def box_area(b):
    b = np.asarray(b, dtype=np.float32).reshape(-1, 4)
    return (b[:, 2] - b[:, 0]).astype(np.float64) * (b[:, 3] - b[:, 1]).astype(np.float64)


def evaluate_image(dboxes, dscores, dlabels, gboxes, glabels, iou_thrs=IOU_THRS):
    """COCOeval.evaluateImg for every class and area range of one image.
    -> rank [nd] (position in the class' stable descending-score order), matched [4, T, nd] and
    ignored [4, T, nd] booleans in input order (detections of rank >= 100 are not evaluated: False),
    gt_ignore [4, ng]."""
    dboxes = np.asarray(dboxes, np.float32).reshape(-1, 4)
    gboxes = np.asarray(gboxes, np.float32).reshape(-1, 4)
    dscores = np.asarray(dscores)
    dlabels = np.asarray(dlabels).astype(np.int64)
    glabels = np.asarray(glabels).astype(np.int64)
    nd, ng, T = len(dscores), len(glabels), len(iou_thrs)
    rank = np.zeros(nd, dtype=np.int64)
    matched = np.zeros((4, T, nd), dtype=bool)
    ignored = np.zeros((4, T, nd), dtype=bool)
    darea, garea = box_area(dboxes), box_area(gboxes)
    gt_ignore = np.zeros((4, ng), dtype=bool)
    for a, (lo, hi) in enumerate(AREA_RNG):
        gt_ignore[a] = (garea < lo) | (garea > hi)
    for c in np.unique(np.concatenate([dlabels, glabels])):
        di = np.nonzero(dlabels == c)[0]
        gi = np.nonzero(glabels == c)[0]
        order = di[np.argsort(-dscores[di], kind="mergesort")]
        rank[order] = np.arange(len(order))
        dt = order[:MAX_DETS[-1]]
        ious_in = iou_xyxy(dboxes[dt], gboxes[gi]) if len(dt) and len(gi) else np.zeros((len(dt), len(gi)))
        for a, (lo, hi) in enumerate(AREA_RNG):
            g_ig = gt_ignore[a][gi]
            gtind = np.argsort(g_ig, kind="mergesort")          # non-ignored first, each group in input order
            g_ig = g_ig[gtind]
            ious = ious_in[:, gtind]
            d_out = (darea[dt] < lo) | (darea[dt] > hi)
            for ti, t in enumerate(iou_thrs):
                gtm = np.zeros(len(gi), dtype=bool)
                for k in range(len(dt)):
                    iou, m = min(t, 1 - 1e-10), -1
                    for g in range(len(gi)):
                        if gtm[g]:
                            continue
                        if m > -1 and not g_ig[m] and g_ig[g]:
                            break
                        if ious[k, g] < iou:
                            continue
                        iou, m = ious[k, g], g
                    if m == -1:
                        ignored[a, ti, dt[k]] = d_out[k]
                        continue
                    gtm[m] = True
                    matched[a, ti, dt[k]] = True
                    ignored[a, ti, dt[k]] = g_ig[m]
    return rank, matched, ignored, gt_ignore


def accumulate_flags(per_image, npig, n_classes, n_thr):
    """COCOeval.accumulate.  per_image: list of (scores, labels, rank, matched [4, T, nd],
    ignored [4, T, nd]) in evaluation order; npig [K, 4]: non-ignored ground truths.
    -> precision [T, 101, K, 4, 3], recall [T, K, 4, 3], -1 for empty cells."""
    T, R, K = n_thr, len(REC_THRS), n_classes
    precision = -np.ones((T, R, K, 4, len(MAX_DETS)))
    recall = -np.ones((T, K, 4, len(MAX_DETS)))
    for c in range(K):
        for a in range(4):
            if npig[c][a] == 0:
                continue
            for mi, max_det in enumerate(MAX_DETS):
                sc, dtm, dtig = [], [], []
                for scores, labels, rank, matched, ignored in per_image:
                    idx = np.nonzero((np.asarray(labels) == c) & (np.asarray(rank) < min(max_det, MAX_DETS[-1])))[0]
                    idx = idx[np.argsort(np.asarray(rank)[idx], kind="mergesort")]
                    sc.append(np.asarray(scores)[idx])
                    dtm.append(np.asarray(matched)[a][:, idx].reshape(T, -1))
                    dtig.append(np.asarray(ignored)[a][:, idx].reshape(T, -1))
                sc = np.concatenate(sc) if sc else np.zeros(0)
                dtm = np.concatenate(dtm, axis=1).astype(bool) if dtm else np.zeros((T, 0), dtype=bool)
                dtig = np.concatenate(dtig, axis=1).astype(bool) if dtig else np.zeros((T, 0), dtype=bool)
                inds = np.argsort(-sc, kind="mergesort")
                dtm, dtig = dtm[:, inds], dtig[:, inds]
                tps = np.logical_and(dtm, np.logical_not(dtig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig[c][a]
                    pr = (tp / (fp + tp + EPS)).tolist()
                    q = np.zeros(R)
                    recall[t, c, a, mi] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    for ri, pi in enumerate(np.searchsorted(rc, REC_THRS, side="left")):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[t, :, c, a, mi] = q
    return precision, recall


def summarize(precision, recall, iou_thrs, classes_with_gt):
    """COCOeval.summarize's twelve numbers under torchmetrics' names, plus the per-class AP / AR@100."""
    iou_thrs = np.asarray(iou_thrs)

    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if len(s) else -1.0

    def ap(area, thr=None):
        s = precision if thr is None else precision[np.where(np.isclose(iou_thrs, thr))[0]]
        return mean(s[:, :, :, AREA_LBL.index(area), 2])

    def ar(area, mi):
        return mean(recall[:, :, AREA_LBL.index(area), mi])

    return {
        "map": ap("all"), "map_50": ap("all", 0.5), "map_75": ap("all", 0.75),
        "map_small": ap("small"), "map_medium": ap("medium"), "map_large": ap("large"),
        "mar_1": ar("all", 0), "mar_10": ar("all", 1), "mar_100": ar("all", 2),
        "mar_small": ar("small", 2), "mar_medium": ar("medium", 2), "mar_large": ar("large", 2),
        "map_per_class": {int(c): mean(precision[:, :, c, 0, 2]) for c in classes_with_gt},
        "mar_100_per_class": {int(c): mean(recall[:, c, 0, 2]) for c in classes_with_gt},
    }


def clustered(rng, n_img, nc=6):
    """tests/test_map_gpu.py's clustered detections with ground-truth sides log-uniform in [8, 300] px
    (all three COCO size classes populated) and a jitter sigma of 0.08 of the side (IoUs spread over
    0.5 .. 0.95); scores have exact ties."""
    preds, targets = [], []
    for _ in range(n_img):
        k = int(rng.integers(0, 9))
        c = rng.uniform(40, 600, (k, 2))
        wh = np.exp(rng.uniform(np.log(8), np.log(300), (k, 2)))
        gb = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
        gl = rng.integers(0, nc, k)
        boxes, scores, labels = [], [], []
        for j in range(k):
            m = int(rng.integers(0, 40))
            jit = rng.normal(0, 0.08, (m, 4)) * np.tile(wh[j], 2)
            boxes.append(gb[j] + jit)
            scores.append(np.round(rng.beta(2, 5, m) * 16) / 16)          # exact ties
            labels.append(np.where(rng.random(m) < 0.85, gl[j], rng.integers(0, nc, m)))
        fp = int(rng.integers(0, 30))
        boxes.append(rng.uniform(0, 640, (fp, 4)).cumsum(1)[:, [0, 1, 2, 3]] % 640)
        scores.append(rng.random(fp))
        labels.append(rng.integers(0, nc, fp))
        b = np.concatenate(boxes).astype(np.float32).reshape(-1, 4)
        b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 1)
        preds.append({"boxes": b, "scores": np.concatenate(scores).astype(np.float32),
                      "labels": np.concatenate(labels).astype(np.int64)})
        targets.append({"boxes": gb.reshape(-1, 4), "labels": gl.astype(np.int64)})
    return preds, targets


def coco_eval(preds, targets, iou_thrs=None):
    """preds / targets: lists of dicts of numpy arrays ('boxes' xyxy, 'scores', 'labels').
    -> dict: per_image [(rank, matched, ignored, gt_ignore)], precision, recall, npig, summary."""
    iou_thrs = IOU_THRS if iou_thrs is None else np.asarray(iou_thrs, dtype=np.float64)
    flags, acc_in, top = [], [], 0
    for p, t in zip(preds, targets):
        for lab in (p["labels"], t["labels"]):
            if len(lab):
                top = max(top, int(np.max(lab)) + 1)
    K = max(top, 1)
    npig = np.zeros((K, 4), dtype=np.int64)
    for p, t in zip(preds, targets):
        rank, matched, ignored, gt_ignore = evaluate_image(p["boxes"], p["scores"], p["labels"], t["boxes"],
                                                           t["labels"], iou_thrs)
        flags.append((rank, matched, ignored, gt_ignore))
        acc_in.append((np.asarray(p["scores"]), np.asarray(p["labels"]).astype(np.int64), rank, matched, ignored))
        for j, c in enumerate(np.asarray(t["labels"]).astype(np.int64)):
            for a in range(4):
                npig[c, a] += 0 if gt_ignore[a, j] else 1
    precision, recall = accumulate_flags(acc_in, npig, K, len(iou_thrs))
    with_gt = [c for c in range(K) if npig[c, 0] > 0]
    return {"per_image": flags, "precision": precision, "recall": recall, "npig": npig,
            "summary": summarize(precision, recall, iou_thrs, with_gt)}
