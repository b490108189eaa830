"""numpy restatement of the test-time-augmentation pieces (yms.tta; csrc/tta.hip and
yms_det_finalize_vote in csrc/detect.hip) -- TEST INFRASTRUCTURE ONLY.

* ``view_sizes`` / ``trim_rows``: the size and row-range rules, restated from their definitions.
* ``merge``: each view's rows [a0, a1) through its flip and its frames, fp32 operation by operation
  (as detect_ref.unmap is), views in call order; scores copied as bits.
* ``finalize_vote``: detect_ref.finalize's selection and outputs; the box of each emitted row is the
  score-weighted mean, in float64, of the live rows of its NMS label whose overlap with it -- the
  fp32 expression of oracle/nms_ref.c -- exceeds the threshold, rounded once to fp32, then un-mapped.
  A weight sum that is 0 or not finite leaves the row's own box.

Candidates, NMS and the selection come from detect_ref."""
from __future__ import annotations

import math

import numpy as np

import detect_ref as R

F32 = np.float32


def view_sizes(size, scales, stride=32):
    H, W = size
    return [(int(math.ceil(H * s / stride)) * stride, int(math.ceil(W * s / stride)) * stride) for s in scales]


def trim_rows(sizes, strides):
    out = []
    for v, s in enumerate(sizes):
        H, W = (s, s) if isinstance(s, int) else s
        rows = [(H // st) * (W // st) for st in strides]
        a0, a1 = 0, sum(rows)
        if len(sizes) >= 2:
            if v == 0:
                a1 -= rows[-1]
            if v == len(sizes) - 1:
                a0 += rows[0]
        out.append((a0, a1))
    return out


def merge(preds, frames, sizes, flips, rows=None):
    """preds[v] [n, A_v, 4+nc], frames[v] [n, 6], sizes[v] (H, W), flips[v] -> [n, sum rows, 4+nc]."""
    if rows is None:
        rows = [(0, p.shape[1]) for p in preds]
    parts = []
    with np.errstate(all="ignore"):
        for p, f, (H, W), fl, (a0, a1) in zip(preds, frames, sizes, flips, rows):
            p = np.asarray(p, F32)[:, a0:a1]
            f = np.asarray(f, F32)
            o = p.copy()
            gx, gy, px, py = (f[:, k][:, None] for k in range(4))
            x = (F32(W) - p[..., 0]).astype(F32) if fl & 1 else p[..., 0]
            y = (F32(H) - p[..., 1]).astype(F32) if fl & 2 else p[..., 1]
            o[..., 0] = ((x - px).astype(F32) / gx).astype(F32)
            o[..., 1] = ((y - py).astype(F32) / gy).astype(F32)
            o[..., 2] = (p[..., 2] / gx).astype(F32)
            o[..., 3] = (p[..., 3] / gy).astype(F32)
            parts.append(o)
    return np.concatenate(parts, 1)


def ovr(bi, b):
    """oracle/nms_ref.c's fp32 overlap of box bi [4] with boxes b [m, 4]."""
    with np.errstate(all="ignore"):
        iarea = ((bi[2] - bi[0]).astype(F32) * (bi[3] - bi[1]).astype(F32)).astype(F32)
        area = ((b[:, 2] - b[:, 0]).astype(F32) * (b[:, 3] - b[:, 1]).astype(F32)).astype(F32)
        w = np.fmax(F32(0), (np.fmin(bi[2], b[:, 2]) - np.fmax(bi[0], b[:, 0])).astype(F32))
        h = np.fmax(F32(0), (np.fmin(bi[3], b[:, 3]) - np.fmax(bi[1], b[:, 1])).astype(F32))
        inter = (w * h).astype(F32)
        return (inter / ((iarea + area).astype(F32) - inter).astype(F32)).astype(F32)


def members(cand, i, iou, agnostic):
    """Live rows that vote for row i."""
    m = cand["count"]
    lab = np.zeros(m, np.int32) if agnostic else cand["label"][:m]
    with np.errstate(invalid="ignore"):
        return np.nonzero((lab == lab[i]) & (ovr(cand["boxes"][i], cand["boxes"][:m]).astype(np.float64) > iou))[0]


def vote_box(cand, i, iou, agnostic):
    js = members(cand, i, iou, agnostic)
    w = cand["score"][js].astype(np.float64)
    with np.errstate(all="ignore"):
        sw = w.sum()
        if sw == 0 or not np.isfinite(sw):
            return cand["boxes"][i].copy()
        return ((w[:, None] * cand["boxes"][js].astype(np.float64)).sum(0) / sw).astype(F32)


def finalize_vote(cand, kept, max_det, iou, agnostic, frame=None):
    """-> det [max_det, 6], anchor [max_det], count, rows (the emitted candidate rows) of one image."""
    sc = cand["score"][kept]
    order = np.lexsort((kept, -sc.view(np.uint32).astype(np.int64)))[:max_det]
    rows = kept[order]
    m = len(rows)
    det = np.zeros((max_det, 6), F32)
    det[:, 5] = -1
    anchor = np.full(max_det, -1, np.int32)
    b = np.stack([vote_box(cand, i, iou, agnostic) for i in rows]) if m else np.zeros((0, 4), F32)
    det[:m, :4] = R.unmap(b, frame) if frame is not None else b
    det[:m, 4] = cand["score"][rows]
    det[:m, 5] = cand["label"][rows]
    anchor[:m] = cand["anchor"][rows]
    return det, anchor, m, rows


def detect_vote(pred, conf=0.25, iou=0.45, multi_label=False, agnostic=False, classes=None, max_det=300,
                max_nms=30000, frames=None):
    """detect_ref.detect with the voting finalize; the extra key ``members`` holds, per image, the
    member count of each kept row (in kept order) and ``kept`` the kept count."""
    pred = np.asarray(pred, F32)
    out = {"det": [], "anchor": [], "count": [], "candidates": [], "kept": [], "cand": [], "members": []}
    for b in range(pred.shape[0]):
        cand = R.candidates(pred[b], conf, multi_label, classes, max_nms)
        kept = R.nms_rows(cand, iou, agnostic)
        det, anchor, m, _ = finalize_vote(cand, kept, max_det, iou, agnostic, None if frames is None else frames[b])
        out["det"].append(det)
        out["anchor"].append(anchor)
        out["count"].append(m)
        out["candidates"].append(cand["total"])
        out["kept"].append(len(kept))
        out["cand"].append(cand)
        out["members"].append(np.asarray([len(members(cand, i, iou, agnostic)) for i in kept], np.int64))
    for k in ("det", "anchor"):
        out[k] = np.stack(out[k])
    for k in ("count", "candidates", "kept"):
        out[k] = np.asarray(out[k], np.int32)
    return out
