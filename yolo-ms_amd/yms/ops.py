"""Functional HIP ops outside the module graph: torchvision-compatible NMS, the
reference's batched post-process (train.py:63-113 / tools/test.py:166-218), the opt-in
COCO-protocol post-process around the same NMS (``detect``) and the standalone DFL integral.
GPU tensors only; every call goes through libyms.so."""
from __future__ import annotations

import ctypes
import os
import threading

import torch

from . import _lib as L


def _cuda(*ts):
    for t in ts:
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("yms: ops run on ROCm GPU tensors only (no CPU fallback)")


def dfl(x, ch=16):
    """DFL (components.py:186-191): x [B, 4*ch, A] -> [B, 4, A]."""
    _cuda(x)
    b, c, a = x.shape
    if c != 4 * ch:
        raise RuntimeError(f"yms: DFL expects {4 * ch} channels, got {c}")
    xc = x.contiguous()
    out = torch.empty((b, 4, a), dtype=x.dtype, device=x.device)
    L.call("yms_dfl", L.dtype_code(x.dtype), b, a, ch, xc.data_ptr(), out.data_ptr(), L.stream_ptr(x.device))
    return out


_TLS = threading.local()


def _nms_ws(dev, B, A, nc, iou):
    """NMS scratch reused across calls, one buffer per (host thread, device, stream): one
    yms_nms_classwise call is a chain of launches on its stream (memset, route / sort, greedy,
    compact), so two threads sharing a stream would interleave their chains over one buffer
     -- a thread's own calls on a stream are ordered, so its buffer is safe to reuse.
    The cache lives in thread-local storage and goes with the thread."""
    # graph NMS (csrc/head_nms.hip) runs on segments of at least YMS_NMS_GRAPH_MIN boxes (default
    # 2048, 0 = off, at least 32, the C side's rule); without it the workspace leaves out the graph
    # kernels' suppressee lists (~530 B per anchor) and every segment takes the other exact routes
    gmin = int(os.environ.get("YMS_NMS_GRAPH_MIN", "2048"))
    full = iou >= 0.0 and gmin > 0 and A >= max(gmin, 32)
    nbytes = (L.lib().yms_nms_ws_bytes if full else L.lib().yms_nms_ws_bytes_min)(B, A, nc)
    return _cached_ws("nms_ws", dev, nbytes), nbytes


def _cached_ws(slot, dev, nbytes):
    """The calling thread's scratch buffer `slot` for (device, current stream), grown on demand."""
    cache = getattr(_TLS, slot, None)
    if cache is None:
        cache = {}
        setattr(_TLS, slot, cache)
    key = (dev.index, L.stream_ptr(dev))
    ws = cache.get(key)
    if ws is None or ws.numel() < nbytes:
        if len(cache) >= 8:            # a thread cycling through many streams: keep a few
            cache.pop(next(iter(cache)))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        cache[key] = ws
    return ws


def nms(boxes, scores, iou_threshold):
    """torchvision.ops.nms(boxes [N,4] xyxy, scores [N], iou) -> int64 keep (score-descending)."""
    _cuda(boxes, scores)
    n = boxes.shape[0]
    dev = boxes.device
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=dev)
    b = boxes.detach().float().contiguous()
    s = scores.detach().float().contiguous()
    keep = torch.empty(n, dtype=torch.int64, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    ws, wsb = _nms_ws(dev, 1, n, 1, float(iou_threshold))
    L.call("yms_nms_single", n, b.data_ptr(), s.data_ptr(), ctypes.c_double(float(iou_threshold)),
           keep.data_ptr(), cnt.data_ptr(), ws.data_ptr(), wsb, L.stream_ptr(dev))
    return keep[:int(cnt.item())]


def batched_nms_indices(pred, conf_thresh=0.25, iou_thresh=0.45):
    """Class-wise NMS for a batch of decoded predictions [B, A, 4+nc] (fp32).

    Returns (boxes_xyxy [B,A,4], scores [B,A], keep_idx [B,A] int64, keep_lbl [B,A] int32,
    counts [B] int32): for image b the first counts[b] entries of keep_idx/keep_lbl are
    the kept anchors, ordered by class ascending then score descending -- the order the
    reference's per-class loop concatenates them in (train.py:85-101)."""
    _cuda(pred)
    B, A, no = pred.shape
    nc = no - 4
    dev = pred.device
    p = pred.detach().float().contiguous()
    st = L.stream_ptr(dev)
    bxy = torch.empty((B, A, 4), dtype=torch.float32, device=dev)
    score = torch.empty((B, A), dtype=torch.float32, device=dev)
    label = torch.empty((B, A), dtype=torch.int32, device=dev)
    L.call("yms_nms_prep", B, A, nc, p.data_ptr(), ctypes.c_float(float(conf_thresh)), bxy.data_ptr(),
           score.data_ptr(), label.data_ptr(), st)
    keep = torch.empty((B, A), dtype=torch.int64, device=dev)
    klbl = torch.empty((B, A), dtype=torch.int32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    ws, wsb = _nms_ws(dev, B, A, nc, float(iou_thresh))
    L.call("yms_nms_classwise", B, A, nc, bxy.data_ptr(), score.data_ptr(), label.data_ptr(),
           ctypes.c_double(float(iou_thresh)), keep.data_ptr(), klbl.data_ptr(), counts.data_ptr(),
           ws.data_ptr(), wsb, st)
    return bxy, score, keep, klbl, counts


def postprocess(pred, conf_thresh=0.25, iou_thresh=0.45):
    """Per image {'boxes' [K,4] xyxy, 'scores' [K], 'labels' [K] int64} -- the dicts the
    reference builds for torchmetrics (train.py:103-113)."""
    bxy, score, keep, klbl, counts = batched_nms_indices(pred, conf_thresh, iou_thresh)
    cnt = counts.cpu().tolist()
    out = []
    for b, k in enumerate(cnt):
        idx = keep[b, :k]
        out.append({"boxes": bxy[b].index_select(0, idx), "scores": score[b].index_select(0, idx),
                    "labels": klbl[b, :k].long()})
    return out


# ------------------------------------------------------------------------------------------
# COCO-protocol detect (csrc/detect.hip): candidates -> NMS -> finalize, no host sync
# ------------------------------------------------------------------------------------------
MAX_NMS_LIMIT, MAX_DET_LIMIT, MAX_CLASSES = 65536, 1024, 1024
_MASKS = {}


class Detections:
    """detect()'s result, all on the device and padded to max_det rows per image (rows beyond
    counts[b] are zero with label / anchor -1): boxes [B, max_det, 4] fp32 xyxy, scores [B, max_det],
    labels and anchors [B, max_det] int32, counts [B] int32, candidates [B] int32 (the image's
    candidates before the max_nms cap)."""
    __slots__ = ("boxes", "scores", "labels", "anchors", "counts", "candidates")

    def __init__(self, boxes, scores, labels, anchors, counts, candidates):
        self.boxes, self.scores, self.labels, self.anchors = boxes, scores, labels, anchors
        self.counts, self.candidates = counts, candidates

    def to_list(self):
        """The one host sync: per image {'boxes' [k, 4], 'scores' [k], 'labels' [k] int64}, what
        yms.metrics.MeanAveragePrecision.update takes."""
        return [{"boxes": self.boxes[b, :k], "scores": self.scores[b, :k], "labels": self.labels[b, :k].long()}
                for b, k in enumerate(self.counts.cpu().tolist())]


def _class_mask(dev, nc, classes):
    """Device uint8 [nc] mask of the class subset, cached so that a repeated call copies nothing."""
    key = (dev.index, nc, classes)
    m = _MASKS.get(key)
    if m is None:
        if len(_MASKS) >= 64:
            _MASKS.pop(next(iter(_MASKS)))
        host = torch.zeros(nc, dtype=torch.uint8)
        host[list(classes)] = 1
        m = _MASKS[key] = host.to(dev)
    return m


def detect(pred, conf=0.25, iou=0.45, *, multi_label=False, agnostic=False, classes=None, max_det=300,
           max_nms=30000, frames=None, vote=False):
    """The post-process of the published YOLOv8 / YOLO-MS AP protocol on decoded predictions
    [B, A, 4+nc] (fp32; (cx, cy, w, h) in input pixels + class scores) -> :class:`Detections`.

    Candidates are every (anchor, class) with score > conf (``multi_label``) or each anchor's best
    class (ties to the lower class) when it is > conf; ``classes`` keeps a subset (in best-class mode
    after the arg-max, as ultralytics filters).  At most ``max_nms`` candidates per image go to the
    NMS, by (score descending, anchor ascending, class ascending); the NMS is class-wise, or
    class-agnostic with ``agnostic``; at most ``max_det`` detections come out, by (score descending,
    candidate row ascending, rows being in ascending anchor * nc + class order).  ``frames``: a
    [B, 6] device tensor (gain_x, gain_y, pad_x, pad_y, w0, h0) -- or yms.data's Frames -- maps the
    boxes back to each original image, min(max((v - pad) / gain, 0), w0 | h0); boxes wholly in the
    padding stay, with zero area.  ``vote`` (ultralytics' merge=True, the companion of yms.tta's view
    merge): each detection's box becomes, before that un-map, the score-weighted mean of the candidate
    rows of its NMS class (agnostic: of all) whose IoU with it -- the NMS's own fp32 expression --
    exceeds ``iou``, summed in float64 and rounded once; a detection whose weights sum to 0 or to a
    non-finite number keeps its box.  Scores, labels, anchors and the selection do not change.  These tie rules are this package's; ultralytics leaves ties to
    its sort (parity UNPINNED).  No host synchronisation; ``Detections.to_list()`` is the one sync."""
    _cuda(pred)
    if pred.dim() != 3 or pred.shape[2] < 5 or pred.shape[0] < 1 or pred.shape[1] < 1:
        raise ValueError(f"yms: detect expects [B, A, 4+nc] predictions, got {tuple(pred.shape)}")
    B, A, no = pred.shape
    nc = no - 4
    conf, iou = float(conf), float(iou)
    if not conf >= 0.0:
        raise ValueError("yms: detect needs conf >= 0 (scores are ordered by their bit patterns)")
    if not 1 <= int(max_nms) <= MAX_NMS_LIMIT:
        raise ValueError(f"yms: max_nms must be in 1..{MAX_NMS_LIMIT}")
    if not 1 <= int(max_det) <= MAX_DET_LIMIT:
        raise ValueError(f"yms: max_det must be in 1..{MAX_DET_LIMIT}")
    if nc > MAX_CLASSES or A * nc >= 2 ** 31:
        raise ValueError(f"yms: detect handles at most {MAX_CLASSES} classes and A * nc < 2^31")
    dev = pred.device
    mask = None
    if classes is not None:
        classes = tuple(sorted({int(c) for c in classes}))
        if any(c < 0 or c >= nc for c in classes):
            raise ValueError(f"yms: classes must be a subset of [0, {nc})")
        mask = _class_mask(dev, nc, classes)
    if frames is not None:
        frames = getattr(frames, "tensor", frames)
        _cuda(frames)
        if tuple(frames.shape) != (B, 6) or frames.dtype != torch.float32 or frames.device != dev:
            raise ValueError("yms: frames must be a [B, 6] fp32 tensor on the predictions' device")
        frames = frames.contiguous()
    max_det = int(max_det)
    # no image has more candidates than pairs: rows beyond that would only ever be fill
    K = min(int(max_nms), A * nc if multi_label else A)
    p = pred.detach().float().contiguous()
    st = L.stream_ptr(dev)
    i32 = dict(dtype=torch.int32, device=dev)
    cbox = torch.empty((B, K, 4), dtype=torch.float32, device=dev)
    cscore = torch.empty((B, K), dtype=torch.float32, device=dev)
    clabel = torch.empty((B, K), **i32)
    canchor = torch.empty((B, K), **i32)
    ccount = torch.empty(B, **i32)
    ctotal = torch.empty(B, **i32)
    wsb = L.lib().yms_det_ws_bytes(B, A, nc, K)
    ws = _cached_ws("det_ws", dev, wsb)
    L.call("yms_det_candidates", B, A, nc, p.data_ptr(), ctypes.c_float(conf), int(bool(multi_label)), L.ptr(mask),
           K, cbox.data_ptr(), cscore.data_ptr(), clabel.data_ptr(), canchor.data_ptr(), ccount.data_ptr(),
           ctotal.data_ptr(), ws.data_ptr(), wsb, st)
    # class-agnostic: every live row is class 0 of one class; the true labels stay in clabel
    nlabel, nnc = (clabel.clamp(max=0), 1) if agnostic else (clabel, nc)
    keep = torch.empty((B, K), dtype=torch.int64, device=dev)
    kcount = torch.empty(B, **i32)
    nws, nwsb = _nms_ws(dev, B, K, nnc, iou)
    L.call("yms_nms_classwise", B, K, nnc, cbox.data_ptr(), cscore.data_ptr(), nlabel.data_ptr(),
           ctypes.c_double(iou), keep.data_ptr(), None, kcount.data_ptr(), nws.data_ptr(), nwsb, st)
    det = torch.empty((B, max_det, 6), dtype=torch.float32, device=dev)
    danchor = torch.empty((B, max_det), **i32)
    dcount = torch.empty(B, **i32)
    if vote:
        L.call("yms_det_finalize_vote", B, K, max_det, cbox.data_ptr(), cscore.data_ptr(), clabel.data_ptr(),
               canchor.data_ptr(), keep.data_ptr(), kcount.data_ptr(), L.ptr(frames), ccount.data_ptr(),
               nlabel.data_ptr(), ctypes.c_double(iou), det.data_ptr(), danchor.data_ptr(), dcount.data_ptr(), st)
    else:
        L.call("yms_det_finalize", B, K, max_det, cbox.data_ptr(), cscore.data_ptr(), clabel.data_ptr(),
               canchor.data_ptr(), keep.data_ptr(), kcount.data_ptr(), L.ptr(frames), det.data_ptr(),
               danchor.data_ptr(), dcount.data_ptr(), st)
    return Detections(det[..., :4], det[..., 4], det[..., 5].to(torch.int32), danchor, dcount, ctotal)
