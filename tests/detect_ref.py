"""numpy restatement of the COCO-protocol detect (yms.ops.detect; csrc/detect.hip) -- TEST
INFRASTRUCTURE ONLY.  Plain fp32 numpy, per image, in the order the contract states it:

1. candidates: multi-label = every (anchor a, class c) with score > conf (NaN never, +inf does);
   best-class = per anchor the pair yms_nms_prep picks (``pick16``) when its score > conf.  A pair
   whose class is not in ``classes`` is dropped (best-class: the arg-max first, the filter after).
   Box = (cx - w/2, cy - h/2, cx + w/2, cy + h/2) in fp32.
2. cap: the first K by (score descending, anchor ascending, class ascending), stored as rows in
   ascending a * nc + c; unused rows zero with label / anchor -1.
3. NMS: per class (agnostic: all live rows as one class) through oracle.nms.nms, as it is.
4. finalize: kept rows by (score descending, row ascending), the first max_det; with a frame
   (gain_x, gain_y, pad_x, pad_y, w0, h0) each coordinate is min(max((v - pad) / gain, 0), w0 | h0)
   with a separately rounded fp32 subtraction and division.

The tie rules are this package's; torchvision and ultralytics leave them to their sorts, and neither
is installed: parity with ultralytics is UNPINNED."""
from __future__ import annotations

import numpy as np

from oracle import nms as onms

F32 = np.float32


def pick16(scores):
    """yms_nms_prep's pick for scores [A, nc] -> (best [A] fp32, label [A]): 16 lanes, lane s walks
    classes s, s + 16, ... (the first unconditionally, then strictly greater), and the lanes combine
    by xor shuffles 8, 4, 2, 1 (greater, or equal with the lower class); lane 0 holds the result.
    Restated lane by lane because a NaN score makes the combination depend on the lanes."""
    A, nc = scores.shape
    best = np.full((A, 16), -np.inf, F32)
    bl = np.full((A, 16), 0x7fffffff, np.int64)
    seen = np.zeros((A, 16), bool)
    lanes = np.arange(16)
    for c0 in range(0, nc, 16):
        c = c0 + lanes
        ok = c < nc
        v = np.zeros((A, 16), F32)
        v[:, ok] = scores[:, c[ok]]
        with np.errstate(invalid="ignore"):
            take = ok[None, :] & (~seen | (v > best))
        best = np.where(take, v, best)
        bl = np.where(take, c[None, :], bl)
        seen |= ok[None, :]
    for off in (8, 4, 2, 1):
        ob, ol = best[:, lanes ^ off], bl[:, lanes ^ off]
        with np.errstate(invalid="ignore"):
            take = (ob > best) | ((ob == best) & (ol < bl))
        best = np.where(take, ob, best)
        bl = np.where(take, ol, bl)
    return best[:, 0].astype(F32), bl[:, 0]


def xyxy(p):
    """(cx, cy, w, h) rows -> xyxy, fp32 operation by operation."""
    p = np.asarray(p, F32)
    cx, cy, w, h = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    two = F32(2)
    return np.stack([cx - w / two, cy - h / two, cx + w / two, cy + h / two], 1).astype(F32)


def candidates(p, conf, multi_label, classes, K):
    """One image p [A, 4+nc] -> dict(boxes [K,4], score [K], label [K], anchor [K], count, total)."""
    p = np.asarray(p, F32)
    A, nc = p.shape[0], p.shape[1] - 4
    conf = F32(conf)
    s = p[:, 4:]
    mask = None
    if classes is not None:
        mask = np.zeros(nc, bool)
        mask[list(classes)] = True
    with np.errstate(invalid="ignore"):
        if multi_label:
            ok = s > conf
            if mask is not None:
                ok &= mask[None, :]
            a_idx, c_idx = np.nonzero(ok)                     # row-major: ascending a * nc + c
            sc = s[a_idx, c_idx]
        else:
            best, bl = pick16(s)
            ok = best > conf
            if mask is not None:
                ok &= mask[np.where(ok, bl, 0)]
            a_idx = np.nonzero(ok)[0]
            c_idx = bl[a_idx]
            sc = best[a_idx]
    total = len(sc)
    if total > K:
        # positive floats order as their bit patterns
        order = np.lexsort((c_idx, a_idx, -sc.view(np.uint32).astype(np.int64)))[:K]
        order = np.sort(order)                                # back to ascending a * nc + c
        a_idx, c_idx, sc = a_idx[order], c_idx[order], sc[order]
    m = len(sc)
    out = {"boxes": np.zeros((K, 4), F32), "score": np.zeros(K, F32), "label": np.full(K, -1, np.int32),
           "anchor": np.full(K, -1, np.int32), "count": m, "total": total}
    out["boxes"][:m] = xyxy(p[:, :4])[a_idx]
    out["score"][:m] = sc
    out["label"][:m] = c_idx
    out["anchor"][:m] = a_idx
    return out


def nms_rows(cand, iou, agnostic):
    """Kept row ids (ascending) of one image's candidate rows."""
    m = cand["count"]
    lab = np.zeros(m, np.int32) if agnostic else cand["label"][:m]
    kept = []
    for c in np.unique(lab):
        rows = np.nonzero(lab == c)[0]
        kept.append(rows[onms.nms(cand["boxes"][rows], cand["score"][rows], iou)])
    return np.sort(np.concatenate(kept)) if kept else np.zeros(0, np.int64)


def unmap(boxes, frame):
    """[m, 4] xyxy fp32 through a frame (gain_x, gain_y, pad_x, pad_y, w0, h0), fp32 op by op."""
    f = np.asarray(frame, F32)
    b = np.asarray(boxes, F32)
    out = np.empty_like(b)
    for k, (g, pd, hi) in enumerate(((f[0], f[2], f[4]), (f[1], f[3], f[5]), (f[0], f[2], f[4]), (f[1], f[3], f[5]))):
        out[:, k] = np.fmin(np.fmax(((b[:, k] - pd).astype(F32) / g).astype(F32), F32(0)), hi)
    return out


def finalize(cand, kept, max_det, frame=None):
    """-> det [max_det, 6], anchor [max_det], count of one image."""
    sc = cand["score"][kept]
    order = np.lexsort((kept, -sc.view(np.uint32).astype(np.int64)))[:max_det]
    rows = kept[order]
    m = len(rows)
    det = np.zeros((max_det, 6), F32)
    det[:, 5] = -1
    anchor = np.full(max_det, -1, np.int32)
    b = cand["boxes"][rows]
    det[:m, :4] = unmap(b, frame) if frame is not None else b
    det[:m, 4] = cand["score"][rows]
    det[:m, 5] = cand["label"][rows]
    anchor[:m] = cand["anchor"][rows]
    return det, anchor, m


def detect(pred, conf=0.25, iou=0.45, multi_label=False, agnostic=False, classes=None, max_det=300,
           max_nms=30000, frames=None):
    """pred [n, A, 4+nc] -> dict of stacked arrays: det [n, max_det, 6], anchor, count, candidates
    (uncapped), kept (the NMS's kept count) and ``cand`` (the per-image candidate stage outputs)."""
    pred = np.asarray(pred, F32)
    out = {"det": [], "anchor": [], "count": [], "candidates": [], "kept": [], "cand": []}
    for b in range(pred.shape[0]):
        cand = candidates(pred[b], conf, multi_label, classes, max_nms)
        kept = nms_rows(cand, iou, agnostic)
        det, anchor, m = finalize(cand, kept, max_det, None if frames is None else frames[b])
        out["det"].append(det)
        out["anchor"].append(anchor)
        out["count"].append(m)
        out["candidates"].append(cand["total"])
        out["kept"].append(len(kept))
        out["cand"].append(cand)
    for k in ("det", "anchor"):
        out[k] = np.stack(out[k])
    for k in ("count", "candidates", "kept"):
        out[k] = np.asarray(out[k], np.int32)
    return out
