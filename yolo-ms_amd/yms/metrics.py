"""Detection mAP on the MI355X path, standing in for
``torchmetrics.detection.MeanAveragePrecision(box_format='xyxy', iou_type='bbox', ...)``.

``iou_thresholds=[0.5]`` is the reference's validation metric, read as ``map_50``
(yolov8/tools/train.py:41-47, 146, 152-153): ``update()`` runs the detection <-> ground-truth
matching on the GPU (``yms_map_match``, one wave per image) and ``compute()`` the per-class
precision / recall accumulation and 101-point interpolation in the native host code
(``yms_map_accumulate``).

Any other setting -- ``iou_thresholds=None`` is COCO's 0.50:0.05:0.95 -- is the full COCOeval
summary on boxes: ``update()`` matches every (threshold, area range) pair in one launch
(``yms_map_match_coco`` / ``_gt``: up to 16 thresholds x all / small / medium / large with COCOeval's ignore
rules), ``compute()`` fills COCOeval's precision[T][101][K][4][3] and recall[T][K][4][3] tables on
the host (``yms_map_accumulate_coco``, maxDets 1 / 10 / 100) and averages them into AP, AP50, AP75,
APs/m/l and AR@1/10/100, ARs/m/l.

``CocoEvaluator`` is the same COCO summary kept on the device from ``yms.ops.detect``'s padded
``Detections`` to the tables: ``update()`` matches straight into epoch buffers without a host
synchronisation (``yms_map_match_coco_fixed`` / ``_gt``), ``compute()`` sorts and accumulates on the GPU
(``yms_map_accumulate_coco_dev``, bit-identical tables) and reads the result back once.

Ground truths may carry COCO's two per-annotation fields, under torchmetrics' key names ``iscrowd`` and
``area`` in a target dict, or as ``gt_crowd`` / ``gt_area`` of ``CocoEvaluator.update``
(``yms.data.COCODetection.eval_annotations`` delivers both).  The rules are COCOeval's evaluateImg /
computeIoU:
  * ``area`` (on COCO the mask's area) decides whether a ground truth is small / medium / large; without it
    the area is w*h of the box.  A detection's own area is always w*h.
  * a crowd ground truth (``iscrowd`` nonzero) is ignore in every area range and never counts as a ground
    truth; its IoU with a detection is intersection / detection area; any number of detections may match
    it, and a detection matched to one is neither a true nor a false positive.  A match with an in-range
    ground truth always wins over one with an ignored ground truth.
Without the two fields every result is bit-identical to what it was before they existed.  The reference's
``[0.5]`` mode reads only the 'all' range, so ``area`` has no effect there, and it refuses crowd ground
truths (use the COCO mode).

COCOeval semantics throughout.  What is pinned: bit-for-bit parity with the restatements
oracle/map_ref.py, tests/cocoeval_ref.py and tests/cocoeval_crowd_ref.py.  What is not: pycocotools and
torchmetrics themselves, which are not installed here; ``coco_results`` turns detections into COCO's
result dicts so that the same detections can be handed to either."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib as L

MAX_THRESHOLDS = 16
N_AREAS = 4                  # all, small, medium, large
MAX_DETS = (1, 10, 100)


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a.size else None


def _host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


_AREA_EDGES = (0.0, 1024.0, 9216.0, 1e10)      # every bound COCOeval's area ranges compare against


def _box_area_f32(boxes):
    """w*h of fp32 xyxy boxes as an fp32 ``area``: the default of a target without one among targets that
    have it.  The kernels compare the double product when no area is given, so a product that only the
    rounding to fp32 puts onto a range bound is moved one step back to its own side of it."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    p = (b[:, 2] - b[:, 0]).astype(np.float64) * (b[:, 3] - b[:, 1]).astype(np.float64)
    with np.errstate(over="ignore"):
        f = p.astype(np.float32)
    for e in _AREA_EDGES:
        off = (f == np.float32(e)) & (p != e)
        f[off] = np.nextafter(f[off], np.where(p[off] > e, np.inf, -np.inf).astype(np.float32))
    return f


def _gt_fields(targets, counts):
    """The targets' optional ``iscrowd`` / ``area`` -> (per-target uint8 arrays or None when no target has
    the key, per-target fp32 arrays or None); a target without a key the others have gets the defaults
    (not crowd, w*h)."""
    crowd = area = None
    if any("iscrowd" in t for t in targets):
        crowd = [(_host(t["iscrowd"]).reshape(-1) != 0).astype(np.uint8) if "iscrowd" in t else np.zeros(k, np.uint8)
                 for t, k in zip(targets, counts)]
    if any("area" in t for t in targets):
        area = [_host(t["area"]).astype(np.float32).reshape(-1) if "area" in t else _box_area_f32(_host(t["boxes"]))
                for t in targets]
    for name, field in (("iscrowd", crowd), ("area", area)):
        if field is not None and any(len(f) != k for f, k in zip(field, counts)):
            raise ValueError(f"a target's {name} must have one entry per label")
    return crowd, area


class MeanAveragePrecision:
    def __init__(self, box_format="xyxy", iou_type="bbox", iou_thresholds=None, **_ignored):
        if box_format != "xyxy" or iou_type != "bbox":
            raise ValueError("yms.metrics.MeanAveragePrecision implements box_format='xyxy', iou_type='bbox'")
        if iou_thresholds is None:
            thr = np.linspace(.5, .95, int(np.round((.95 - .5) / .05)) + 1, endpoint=True)
        else:
            thr = np.asarray(list(iou_thresholds), dtype=np.float64).reshape(-1)
        if not 1 <= thr.size <= MAX_THRESHOLDS:
            raise ValueError(f"yms.metrics.MeanAveragePrecision takes 1 to {MAX_THRESHOLDS} iou_thresholds")
        if not (np.all(thr > 0) and np.all(thr <= 1) and np.all(np.diff(thr) > 0)):
            raise ValueError("iou_thresholds must be increasing values in (0, 1]")
        self.iou_thresholds = thr
        # the reference's setting keeps its own kernel, accumulation and result keys
        self._coco = not (iou_thresholds is not None and list(iou_thresholds) == [0.5])
        self.reset()

    def reset(self):
        self._scores, self._labels, self._image, self._tp, self._kept = [], [], [], [], []
        self._rank, self._matched, self._ignored, self._glabels, self._gignore = [], [], [], [], []
        self._ngt = {}
        self._n_images = 0

    def to(self, device):      # torchmetrics-style no-op (state lives on the host)
        return self

    def update(self, preds, targets):
        if len(preds) != len(targets):
            raise ValueError("preds and targets must have the same length")
        if not preds:
            return
        dev = next((p["boxes"].device for p in preds if isinstance(p["boxes"], torch.Tensor)), None)
        if dev is None or dev.type != "cuda":
            raise RuntimeError("yms: mAP matching runs on ROCm GPU tensors only (no CPU fallback)")
        db = torch.cat([p["boxes"].reshape(-1, 4).float() for p in preds]).contiguous()
        ds = torch.cat([p["scores"].reshape(-1).float() for p in preds]).contiguous()
        dl = torch.cat([p["labels"].reshape(-1).to(torch.int32) for p in preds]).contiguous()
        gb = torch.cat([t["boxes"].reshape(-1, 4).float().to(dev) for t in targets]).contiguous()
        gl = torch.cat([t["labels"].reshape(-1).to(torch.int32).to(dev) for t in targets]).contiguous()
        nd = [int(p["scores"].numel()) for p in preds]
        ng = [int(t["labels"].numel()) for t in targets]
        doff = torch.tensor(np.concatenate([[0], np.cumsum(nd)]), dtype=torch.int32, device=dev)
        goff = torch.tensor(np.concatenate([[0], np.cumsum(ng)]), dtype=torch.int32, device=dev)
        n = int(sum(nd))
        D = max(n, 1)
        image = np.repeat(np.arange(self._n_images, self._n_images + len(preds), dtype=np.int32), nd)
        crowd, area = _gt_fields(targets, ng)
        if not self._coco and crowd is not None and any(c.any() for c in crowd):
            raise ValueError("yms: iou_thresholds=[0.5] is the reference's metric and cannot score crowd ground "
                             "truths; "
                             "construct MeanAveragePrecision in the COCO mode (iou_thresholds=None, or any other "
                             "list) to evaluate targets with nonzero iscrowd")
        if self._coco:
            up = lambda xs, dt: torch.from_numpy(np.concatenate([np.zeros(0, dt)] + xs)).to(dev)
            gcr = up(crowd, np.uint8) if crowd is not None else None
            gar = up(area, np.float32) if area is not None else None
            G = max(int(sum(ng)), 1)
            matched = torch.zeros(N_AREAS, D, dtype=torch.int16, device=dev)
            ignored = torch.zeros(N_AREAS, D, dtype=torch.int16, device=dev)
            gign = torch.zeros(G, dtype=torch.uint8, device=dev)
            rank = torch.empty(2 * D, dtype=torch.int32, device=dev)
            thr = self.iou_thresholds
            args = (len(preds), n, L.ptr(db) if n else None, L.ptr(ds) if n else None,
                    L.ptr(dl) if n else None, doff.data_ptr(), L.ptr(gb) if gb.numel() else None,
                    L.ptr(gl) if gl.numel() else None, goff.data_ptr(), int(thr.size), _hp(thr), matched.data_ptr(),
                    ignored.data_ptr(), gign.data_ptr(), rank.data_ptr(), max(ng) if ng else 0)
            if gcr is None and gar is None:
                L.call("yms_map_match_coco", *args, L.stream_ptr(dev))
            else:
                L.call("yms_map_match_coco_gt", *args, L.ptr(gcr) if gcr is not None and gcr.numel() else None,
                       L.ptr(gar) if gar is not None and gar.numel() else None, L.stream_ptr(dev))
            self._scores.append(ds.cpu().numpy())
            self._labels.append(dl.cpu().numpy())
            self._rank.append(rank[:n].cpu().numpy())
            self._matched.append(matched[:, :n].cpu().numpy().view(np.uint16))
            self._ignored.append(ignored[:, :n].cpu().numpy().view(np.uint16))
            self._glabels.append(gl.cpu().numpy())
            self._gignore.append(gign[:int(sum(ng))].cpu().numpy())
            self._image.append(image)
            self._n_images += len(preds)
            return
        tp = torch.zeros(D, dtype=torch.uint8, device=dev)
        kept = torch.zeros(D, dtype=torch.uint8, device=dev)
        rank = torch.empty(D, dtype=torch.int32, device=dev)
        L.call("yms_map_match", len(preds), L.ptr(db) if db.numel() else None, L.ptr(ds) if ds.numel() else None,
               L.ptr(dl) if dl.numel() else None, doff.data_ptr(), L.ptr(gb) if gb.numel() else None,
               L.ptr(gl) if gl.numel() else None, goff.data_ptr(), tp.data_ptr(), kept.data_ptr(), rank.data_ptr(),
               max(ng) if ng else 0, L.stream_ptr(dev))
        self._scores.append(ds.cpu().numpy())
        self._labels.append(dl.cpu().numpy())
        self._tp.append(tp[:n].cpu().numpy())
        self._kept.append(kept[:n].cpu().numpy())
        self._image.append(image)
        for c in gl.cpu().numpy().tolist():
            self._ngt[c] = self._ngt.get(c, 0) + 1
        self._n_images += len(preds)

    def compute(self):
        if self._coco:
            return self._compute_coco()
        cat = (lambda xs, dt: np.ascontiguousarray(np.concatenate(xs).astype(dt)) if xs else np.zeros(0, dt))
        sc, lb = cat(self._scores, np.float32), cat(self._labels, np.int32)
        im, tp, kp = cat(self._image, np.int32), cat(self._tp, np.uint8), cat(self._kept, np.uint8)
        ncls = max([int(lb.max()) + 1 if lb.size else 0] + [c + 1 for c in self._ngt] + [1])
        ngt = np.zeros(ncls, dtype=np.int32)
        for c, k in self._ngt.items():
            if c >= 0:
                ngt[c] = k
        ap = np.zeros(ncls, dtype=np.float64)
        m = np.zeros(1, dtype=np.float64)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None
        L.check(L.lib().yms_map_accumulate(int(sc.size), p(sc), p(lb), p(im), p(tp), p(kp), ncls, p(ngt), p(ap), p(m)),
                "yms_map_accumulate")
        per = {c: float(ap[c]) for c in range(ncls) if ngt[c] > 0}
        mv = torch.tensor(float(m[0]), dtype=torch.float64)
        return {"map": mv, "map_50": mv.clone(), "map_per_class": per}

    def tables(self):
        """COCOeval's ``eval['precision']`` [T, 101, K, 4, 3] and ``eval['recall']`` [T, K, 4, 3] (float64,
        -1 for cells without a non-ignored ground truth) and the per-(class, area) count of those."""
        if not self._coco:
            raise RuntimeError("yms: the precision / recall tables belong to the COCO mode (iou_thresholds != [0.5])")
        cat = (lambda xs, dt: np.ascontiguousarray(np.concatenate(xs).astype(dt)) if xs else np.zeros(0, dt))
        sc, lb = cat(self._scores, np.float32), cat(self._labels, np.int32)
        im, rk = cat(self._image, np.int32), cat(self._rank, np.int32)
        cat2 = (lambda xs: np.ascontiguousarray(np.concatenate(xs, axis=1)) if xs
                else np.zeros((N_AREAS, 0), np.uint16))
        mt, ig = cat2(self._matched), cat2(self._ignored)
        gl, gi = cat(self._glabels, np.int32), cat(self._gignore, np.uint8)
        K = max([int(lb.max()) + 1 if lb.size else 0, int(gl.max()) + 1 if gl.size else 0, 1])
        npig = np.zeros((K, N_AREAS), dtype=np.int32)
        ok = gl >= 0
        for a in range(N_AREAS):
            np.add.at(npig[:, a], gl[ok & (((gi >> a) & 1) == 0)], 1)
        T = int(self.iou_thresholds.size)
        precision = np.empty((T, 101, K, N_AREAS, len(MAX_DETS)), dtype=np.float64)
        recall = np.empty((T, K, N_AREAS, len(MAX_DETS)), dtype=np.float64)
        L.check(L.lib().yms_map_accumulate_coco(int(sc.size), _hp(sc), _hp(lb), _hp(im), _hp(rk), _hp(mt), _hp(ig), T,
                                                K, _hp(npig), _hp(precision), _hp(recall)),
                "yms_map_accumulate_coco")
        return precision, recall, npig

    def _compute_coco(self):
        precision, recall, npig = self.tables()
        thr = self.iou_thresholds

        def mean(s):
            s = s[s > -1]
            return float(np.mean(s)) if s.size else -1.0

        def ap(area=0, iou=None):
            s = precision
            if iou is not None:
                s = s[np.isclose(thr, iou)]
            return mean(s[:, :, :, area, 2])

        def ar(area=0, md=2):
            return mean(recall[:, :, area, md])

        f = lambda v: torch.tensor(v, dtype=torch.float64)
        classes = [c for c in range(npig.shape[0]) if npig[c, 0] > 0]
        return {
            "map": f(ap()), "map_50": f(ap(iou=0.5)), "map_75": f(ap(iou=0.75)),
            "map_small": f(ap(1)), "map_medium": f(ap(2)), "map_large": f(ap(3)),
            "mar_1": f(ar(md=0)), "mar_10": f(ar(md=1)), "mar_100": f(ar(md=2)),
            "mar_small": f(ar(1)), "mar_medium": f(ar(2)), "mar_large": f(ar(3)),
            "map_per_class": {c: mean(precision[:, :, c, 0, 2]) for c in classes},
            "mar_100_per_class": {c: mean(recall[:, c, 0, 2]) for c in classes},
            "classes": torch.tensor(np.unique(np.concatenate(
                [np.zeros(0, np.int32)] + self._labels + self._glabels)).astype(np.int32)),
        }


_SUMMARY_KEYS = ("map", "map_50", "map_75", "map_small", "map_medium", "map_large",
                 "mar_1", "mar_10", "mar_100", "mar_small", "mar_medium", "mar_large")
MAX_DET_LIMIT, MAX_GT_LIMIT, MAX_CLASSES = 1024, 2048, 4096


class CocoEvaluator:
    """COCO AP (the summary of ``MeanAveragePrecision``'s COCO mode) without leaving the device.

    ``update(detections, gt_boxes, gt_labels, gt_counts)`` takes ``yms.ops.detect``'s
    :class:`~yms.ops.Detections` (or a (boxes [B, max_det, 4], scores [B, max_det], labels [B, max_det],
    counts [B]) tuple) and padded device ground truths ([B, G, 4] fp32 xyxy, [B, G] int, [B] int; see
    :meth:`pad_targets`), and matches them into epoch buffers of ``max_det`` rows per image: no host
    synchronisation, no ``.cpu()``; the buffers double when they are full (decided from the shapes).
    ``max_det`` is fixed by the first call; images are numbered in call order.  ``compute()`` runs the
    device accumulation and reads the summary back once.  ``num_classes`` fixes the tables' class axis:
    labels outside [0, num_classes) take no part."""

    def __init__(self, num_classes, iou_thresholds=None, capacity_images=1024):
        if not 1 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError(f"yms.metrics.CocoEvaluator takes 1 to {MAX_CLASSES} classes")
        if iou_thresholds is None:
            thr = np.linspace(.5, .95, int(np.round((.95 - .5) / .05)) + 1, endpoint=True)
        else:
            thr = np.asarray(list(iou_thresholds), dtype=np.float64).reshape(-1)
        if not 1 <= thr.size <= MAX_THRESHOLDS:
            raise ValueError(f"yms.metrics.CocoEvaluator takes 1 to {MAX_THRESHOLDS} iou_thresholds")
        if not (np.all(thr > 0) and np.all(thr <= 1) and np.all(np.diff(thr) > 0)):
            raise ValueError("iou_thresholds must be increasing values in (0, 1]")
        if int(capacity_images) < 1:
            raise ValueError("capacity_images must be at least 1")
        self.num_classes = int(num_classes)
        self.iou_thresholds = np.ascontiguousarray(thr)
        self.capacity_images = int(capacity_images)
        self._dev = None
        self._buf = None             # (score, label, rank, matched [4, cap], ignored [4, cap])
        self._cap = 0                # rows
        self._order = None
        self.reset()

    def reset(self):
        """Start a new epoch: the buffers and max_det stay, the counters are zeroed (on the device)."""
        self._n_images = 0
        self._exact = False          # set by an update with gt_crowd / gt_area: compute() then sums as numpy does
        if self._dev is not None:
            self._npig.zero_()
            self._gt_seen.zero_()
        else:
            self._max_det = None

    def to(self, device):      # torchmetrics-style no-op (state lives where the first update's tensors do)
        return self

    @staticmethod
    def pad_targets(targets, device, flags=False):
        """[{'boxes' [k, 4], 'labels' [k]}, ...] (numpy arrays or tensors) -> (gt_boxes [B, G, 4] fp32,
        gt_labels [B, G] int32 padded with -1, gt_counts [B] int32) on ``device``, G = the largest k.
        Host work and one upload (tensors already on a device are read back first).
        With ``flags=True`` the targets' optional 'iscrowd' [k] and 'area' [k] come along: the return is
        (gt_boxes, gt_labels, gt_counts, gt_crowd [B, G] uint8, gt_area [B, G] fp32), padded with 0, a
        target without a key getting the defaults (not crowd, w*h) -- still one upload."""
        host = _host
        bs = [host(t["boxes"]).astype(np.float32).reshape(-1, 4) for t in targets]
        ls = [host(t["labels"]).astype(np.int32).reshape(-1) for t in targets]
        B = len(targets)
        G = max([len(l) for l in ls] + [0])
        boxes = np.zeros((B, G, 4), np.float32)
        labels = np.full((B, G), -1, np.int32)
        counts = np.zeros(B, np.int32)
        for i, (b, l) in enumerate(zip(bs, ls)):
            if len(b) != len(l):
                raise ValueError("a target's boxes and labels must have the same length")
            boxes[i, :len(l)], labels[i, :len(l)], counts[i] = b, l, len(l)
        nb, nl = B * G * 4, B * G
        if not flags:
            packed = np.concatenate([boxes.view(np.int32).reshape(-1), labels.reshape(-1), counts])
            d = torch.from_numpy(packed).to(device)
            return d[:nb].view(torch.float32).view(B, G, 4), d[nb:nb + nl].view(B, G), d[nb + nl:]
        cs, ars = _gt_fields(targets, counts.tolist())
        crowd = np.zeros((nl + 3) // 4 * 4, np.uint8)               # [B, G] bytes, the tail padded to a whole int32
        area = np.zeros((B, G), np.float32)
        for i in range(B):
            k = counts[i]
            crowd[i * G:i * G + k] = cs[i] if cs is not None else 0
            area[i, :k] = ars[i] if ars is not None else _box_area_f32(bs[i])
        packed = np.concatenate([boxes.view(np.int32).reshape(-1), labels.reshape(-1), counts,
                                 area.view(np.int32).reshape(-1), crowd.view(np.int32)])
        d = torch.from_numpy(packed).to(device)
        na = nb + nl + B
        gt_crowd = d[na + nl:].view(torch.uint8)[:nl].view(B, G) if nl else d.new_zeros((B, G), dtype=torch.uint8)
        return (d[:nb].view(torch.float32).view(B, G, 4), d[nb:nb + nl].view(B, G), d[nb + nl:na], gt_crowd,
                d[na:na + nl].view(torch.float32).view(B, G))

    def _reserve(self, dev, rows):
        """Epoch buffers for at least `rows` rows: doubled (from capacity_images) and copied on the device."""
        if self._dev is None:
            self._dev = dev
            self._npig = torch.zeros((self.num_classes, N_AREAS), dtype=torch.int32, device=dev)
            self._gt_seen = torch.zeros(self.num_classes, dtype=torch.int32, device=dev)
        elif dev != self._dev:
            raise ValueError("yms: CocoEvaluator.update got tensors on another device than its first call")
        if rows <= self._cap:
            return
        cap = max(self._cap, self.capacity_images * self._max_det)
        while cap < rows:
            cap *= 2
        new = (torch.empty(cap, dtype=torch.float32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
               torch.empty(cap, dtype=torch.int32, device=dev), torch.empty((N_AREAS, cap), dtype=torch.int16, device=dev),
               torch.empty((N_AREAS, cap), dtype=torch.int16, device=dev))
        used = self._n_images * self._max_det
        if self._buf is not None and used:
            for o, n in zip(self._buf, new):
                n[..., :used].copy_(o[..., :used])
        self._buf, self._cap = new, cap

    def update(self, detections, gt_boxes, gt_labels, gt_counts, gt_crowd=None, gt_area=None):
        """``gt_crowd`` [B, G] (nonzero = a crowd ground truth) and ``gt_area`` [B, G] (the annotations' area)
        are COCOeval's iscrowd and area (module docstring), each optional; ``pad_targets(..., flags=True)``
        builds both."""
        if isinstance(detections, (tuple, list)):
            boxes, scores, labels, counts = detections
        else:
            boxes, scores, labels, counts = detections.boxes, detections.scores, detections.labels, detections.counts
        for t in (boxes, scores, labels, counts, gt_boxes, gt_labels, gt_counts) + \
                tuple(x for x in (gt_crowd, gt_area) if x is not None):
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
                raise RuntimeError("yms: CocoEvaluator runs on ROCm GPU tensors only (no CPU fallback)")
        if boxes.dim() != 3 or boxes.shape[2] != 4:
            raise ValueError(f"yms: detections' boxes must be [B, max_det, 4], got {tuple(boxes.shape)}")
        B, M = int(boxes.shape[0]), int(boxes.shape[1])
        if tuple(scores.shape) != (B, M) or tuple(labels.shape) != (B, M) or tuple(counts.shape) != (B,):
            raise ValueError("yms: detections' scores / labels must be [B, max_det] and counts [B]")
        if gt_labels.dim() != 2 or gt_labels.shape[0] != B or tuple(gt_boxes.shape) != (B, gt_labels.shape[1], 4) \
                or tuple(gt_counts.shape) != (B,):
            raise ValueError("yms: ground truths must be padded to gt_boxes [B, G, 4], gt_labels [B, G], gt_counts [B]")
        G = int(gt_labels.shape[1])
        for name, t in (("gt_crowd", gt_crowd), ("gt_area", gt_area)):
            if t is not None and tuple(t.shape) != (B, G):
                raise ValueError(f"yms: {name} must be [B, G] like gt_labels, got {tuple(t.shape)}")
        if self._max_det is None:
            if not 1 <= M <= MAX_DET_LIMIT:
                raise ValueError(f"yms: max_det must be in 1..{MAX_DET_LIMIT}")
            self._max_det = M
        elif M != self._max_det:
            raise ValueError(f"yms: max_det is {self._max_det} since the first update, got {M}")
        if B == 0:
            return
        dev = boxes.device
        i32 = torch.int32
        db = boxes.detach().to(torch.float32).contiguous()
        ds = scores.detach().to(torch.float32).contiguous()
        dl = labels.to(i32).contiguous()
        dc = counts.to(i32).contiguous()
        gb = gt_boxes.detach().to(torch.float32).contiguous()
        gl = gt_labels.to(i32).contiguous()
        gc = gt_counts.to(i32).contiguous()
        row0 = self._n_images * M
        self._reserve(dev, row0 + B * M)
        if self._order is None or self._order.numel() < B * M:
            self._order = torch.empty(B * M, dtype=i32, device=dev)
        score, label, rank, matched, ignored = self._buf
        thr = self.iou_thresholds
        args = (B, M, db.data_ptr(), ds.data_ptr(), dl.data_ptr(), dc.data_ptr(), G,
                gb.data_ptr() if G else None, gl.data_ptr() if G else None, gc.data_ptr(), int(thr.size), _hp(thr),
                self.num_classes, self._cap, row0, score.data_ptr(), label.data_ptr(), rank.data_ptr(),
                matched.data_ptr(), ignored.data_ptr(), self._npig.data_ptr(), self._order.data_ptr())
        if gt_crowd is None and gt_area is None:
            L.call("yms_map_match_coco_fixed", *args, L.stream_ptr(dev))
        else:
            gcr = gar = None
            if gt_crowd is not None:     # the kernel tests != 0 itself: one byte per ground truth goes in as it is
                gcr = gt_crowd if gt_crowd.dtype == torch.uint8 else \
                    gt_crowd.view(torch.uint8) if gt_crowd.dtype == torch.bool else (gt_crowd != 0).to(torch.uint8)
                gcr = gcr.contiguous()
            if gt_area is not None:
                gar = gt_area.detach().to(torch.float32).contiguous()
            self._exact = True
            L.call("yms_map_match_coco_fixed_gt", *args, L.ptr(gcr) if G else None, L.ptr(gar) if G else None,
                   L.stream_ptr(dev))
        if G:     # classes with a ground truth of any size, crowd or not, for `classes`
            live = (torch.arange(G, device=dev).unsqueeze(0) < gc.unsqueeze(1)) & (gl >= 0) & (gl < self.num_classes)
            self._gt_seen.scatter_add_(0, gl.clamp(0, self.num_classes - 1).reshape(-1).long(),
                                       live.reshape(-1).to(i32))
        self._n_images += B

    def _tables_dev(self):
        """The device accumulate -> (precision, recall) device tensors."""
        T, K = int(self.iou_thresholds.size), self.num_classes
        dev = self._dev if self._dev is not None else torch.device("cuda", torch.cuda.current_device())
        if self._dev is None:
            self._reserve(dev, 0)
        n_rows = self._n_images * (self._max_det or 0)
        precision = torch.empty((T, 101, K, N_AREAS, len(MAX_DETS)), dtype=torch.float64, device=dev)
        recall = torch.empty((T, K, N_AREAS, len(MAX_DETS)), dtype=torch.float64, device=dev)
        wsb = L.lib().yms_map_accumulate_coco_dev_ws_bytes(n_rows, T, K)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        buf = self._buf if n_rows else (None,) * 5
        L.call("yms_map_accumulate_coco_dev", n_rows, self._cap, *[L.ptr(b) for b in buf], T, K,
               self._npig.data_ptr(), precision.data_ptr(), recall.data_ptr(), ws.data_ptr(), wsb, L.stream_ptr(dev))
        return precision, recall

    def tables(self):
        """COCOeval's ``eval['precision']`` [T, 101, K, 4, 3], ``eval['recall']`` [T, K, 4, 3] and the
        per-(class, area) count of non-ignored ground truths, as numpy arrays."""
        precision, recall = self._tables_dev()
        return precision.cpu().numpy(), recall.cpu().numpy(), self._npig.cpu().numpy()

    def compute(self):
        """The summary of ``MeanAveragePrecision``'s COCO mode, read back in one host read.  An epoch without
        gt_crowd / gt_area reduces the tables on the device, as it always has (its means differ from numpy's
        by the order of summation, within 1e-10).  An epoch that was given either field brings the maxDets-100
        precision slice and the recall table back instead (T * K * (101 * 4 + 12) doubles) and averages them
        on the host in numpy's order, equal bit for bit to ``MeanAveragePrecision`` on the same inputs."""
        precision, recall = self._tables_dev()
        T, K, thr = int(self.iou_thresholds.size), self.num_classes, self.iou_thresholds
        n_rows = self._n_images * (self._max_det or 0)
        det_seen = torch.zeros(K, dtype=torch.int32, device=precision.device)
        if n_rows:
            lab = self._buf[1][:n_rows]
            det_seen.scatter_add_(0, lab.clamp(0, K - 1).long(), ((lab >= 0) & (lab < K)).to(torch.int32))
        flags = [self._npig[:, 0].to(torch.float64), (self._gt_seen + det_seen).to(torch.float64)]
        if self._exact:
            vals, ap_c, ar_c, with_gt, seen = self._summary_host(precision, recall, flags)
        else:
            vals, ap_c, ar_c, with_gt, seen = self._summary_dev(precision, recall, flags)
        out = {k: torch.tensor(float(v), dtype=torch.float64) for k, v in zip(_SUMMARY_KEYS, vals)}
        classes = [c for c in range(K) if with_gt[c] > 0]
        out["map_per_class"] = {c: float(ap_c[c]) for c in classes}
        out["mar_100_per_class"] = {c: float(ar_c[c]) for c in classes}
        out["classes"] = torch.tensor(np.nonzero(seen > 0)[0].astype(np.int32))
        return out

    def _summary_dev(self, precision, recall, flags):
        """masked float64 means on the device -> one vector -> the host"""
        K, thr = self.num_classes, self.iou_thresholds
        zero = torch.zeros((), dtype=torch.float64, device=precision.device)

        def mean(s, dims):
            m = s > -1
            cnt = m.sum(dims)
            return torch.where(cnt > 0, torch.where(m, s, zero).sum(dims) / cnt.clamp(min=1), zero - 1.0)

        def ap(area=0, iou=None):
            s = precision
            if iou is not None:
                s = s[np.nonzero(np.isclose(thr, iou))[0].tolist()]
            return mean(s[:, :, :, area, 2], (0, 1, 2))

        def ar(area=0, md=2):
            return mean(recall[:, :, area, md], (0, 1))

        parts = [torch.stack([ap(), ap(iou=0.5), ap(iou=0.75), ap(1), ap(2), ap(3), ar(md=0), ar(md=1), ar(md=2),
                              ar(1), ar(2), ar(3)]),
                 mean(precision[:, :, :, 0, 2], (0, 1)), mean(recall[:, :, 0, 2], (0,))] + flags
        host = torch.cat(parts).cpu().numpy()                        # the one host read
        return np.split(host, [12, 12 + K, 12 + 2 * K, 12 + 3 * K])

    def _summary_host(self, precision, recall, flags):
        """the summary's table slices -> the host -> MeanAveragePrecision._compute_coco's numpy means"""
        T, K, thr = int(self.iou_thresholds.size), self.num_classes, self.iou_thresholds
        parts = [precision[..., 2].reshape(-1), recall.reshape(-1)] + flags
        host = torch.cat(parts).cpu().numpy()                        # the one host read
        n_p, n_r = T * 101 * K * N_AREAS, T * K * N_AREAS * len(MAX_DETS)
        prec, rec, with_gt, seen = np.split(host, [n_p, n_p + n_r, n_p + n_r + K])
        prec, rec = prec.reshape(T, 101, K, N_AREAS), rec.reshape(T, K, N_AREAS, len(MAX_DETS))

        def mean(s):
            s = s[s > -1]
            return float(np.mean(s)) if s.size else -1.0

        def ap(area=0, iou=None):
            s = prec if iou is None else prec[np.isclose(thr, iou)]
            return mean(s[:, :, :, area])

        def ar(area=0, md=2):
            return mean(rec[:, :, area, md])

        vals = [ap(), ap(iou=0.5), ap(iou=0.75), ap(1), ap(2), ap(3), ar(md=0), ar(md=1), ar(md=2), ar(1), ar(2), ar(3)]
        return (vals, [mean(prec[:, :, c, 0]) for c in range(K)], [mean(rec[:, c, 0, 2]) for c in range(K)],
                with_gt, seen)



def coco_results(detections, image_ids, label2cat=None):
    """``yms.ops.detect``'s :class:`~yms.ops.Detections` (or a (boxes [B, max_det, 4] xyxy, scores, labels,
    counts [B]) tuple) -> COCO's result list [{'image_id', 'category_id', 'bbox': [x, y, w, h], 'score'}], image b
    under ``image_ids[b]``, label l under ``label2cat[l]`` (a dict or sequence, e.g.
    ``COCODetection.label2cat``; None keeps the label).  One host read.  This is what ``COCO.loadRes`` and the
    evaluation servers take, so the same detections can be scored by pycocotools itself."""
    if isinstance(detections, (tuple, list)):
        boxes, scores, labels, counts = detections
    else:
        boxes, scores, labels, counts = detections.boxes, detections.scores, detections.labels, detections.counts
    B, M = int(boxes.shape[0]), int(boxes.shape[1])
    if len(image_ids) != B:
        raise ValueError(f"yms: coco_results got {len(image_ids)} image_ids for {B} images")
    f64 = lambda t: t.detach().to(torch.float64).reshape(-1)
    wh = boxes[..., 2:].float() - boxes[..., :2].float()                   # fp32, as the matching converts xyxy
    host = torch.cat([f64(boxes[..., :2]), f64(wh), f64(scores), f64(labels), f64(counts)]).cpu().numpy()
    xy, wh, sc, lb, cn = np.split(host, np.cumsum([B * M * 2, B * M * 2, B * M, B * M]))
    xy, wh = xy.reshape(B, M, 2), wh.reshape(B, M, 2)
    sc, lb = sc.reshape(B, M), lb.reshape(B, M).astype(np.int64)
    out = []
    for b in range(B):
        for d in range(min(max(int(cn[b]), 0), M)):
            lab = int(lb[b, d])
            out.append({"image_id": image_ids[b], "category_id": lab if label2cat is None else label2cat[lab],
                        "bbox": [float(xy[b, d, 0]), float(xy[b, d, 1]), float(wh[b, d, 0]), float(wh[b, d, 1])],
                        "score": float(sc[b, d])})
    return out
